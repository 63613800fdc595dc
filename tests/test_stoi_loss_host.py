"""The STOI / ESTOI criteria on the host: the differentiable restatement (tests/stoi_loss_ref.py) against
oracle/stoi.py and against finite differences, the zero convention, the threshold clearance the GPU tests rely on,
the C ABI of libbrever_stoi_loss.so (header, exports, refusals) and the registry keys. No GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

import stoi_loss_ref as R
from brever_amd import hip, stoi
from oracle.stoi import stoi as oracle_stoi

# every (fs, n) the GPU tests use, with the kept / all frame counts of the recipe
GPU_CASES = {(16000, 24000): (75, 116), (16000, 17777): (58, 85), (16000, 16000): (50, 77),
             (16000, 6000): (20, 28), (8000, 12000): (76, 116), (10000, 16000): (79, 123)}


def _direction(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def _fd(clean, est, fs, extended, v, h):
    up = float(R.stoi(clean, est + h*v, fs, extended))
    dn = float(R.stoi(clean, est - h*v, fs, extended))
    return (up - dn)/(2*h)


# -- the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extended', [False, True])
@pytest.mark.parametrize('fs,n', [(16000, 24000), (16000, 17777), (10000, 16000), (10000, 11111), (8000, 12000),
                                  (8000, 9001)])
def test_restatement_value_equals_the_oracle(fs, n, extended):
    clean, est = R.signals(fs, n)
    want = oracle_stoi(clean, est, fs, extended=extended)
    got = float(R.stoi(clean, est, fs, extended))
    print(fs, n, extended, f'|restatement - oracle| = {abs(got - want):.3e}')
    assert 0.1 < want < 1.0
    assert abs(got - want) <= 1e-12


def test_restatement_short_signal_is_the_oracles_constant():
    clean, est = R.signals(16000, 6000)
    for extended in (False, True):
        assert oracle_stoi(clean, est, 16000, extended=extended) == 1e-5
        value, grad = R.value_and_grad(clean, est, 16000, extended)
        assert value == 1e-5 and not grad.any()


@pytest.mark.parametrize('extended', [False, True])
@pytest.mark.parametrize('fs,n', [(16000, 16000), (10000, 16000), (8000, 12000)])
def test_restatement_gradient_equals_central_differences(fs, n, extended):
    clean, est = R.signals(fs, n)
    _, grad = R.value_and_grad(clean, est, fs, extended)
    v = _direction(n)
    want = _fd(clean, est, fs, extended, v, 1e-6)
    got = float(grad @ v)
    print(fs, n, extended, f'autograd {got:.9e} central differences {want:.9e} rel {abs(got - want)/abs(want):.3e}')
    assert abs(got - want) <= 1e-6*abs(want)


@pytest.mark.parametrize('extended', [False, True])
def test_zero_stretch_has_a_finite_gradient(extended):
    fs, n = 10000, 16000
    lo, hi = R.ZERO_STRETCH
    clean, est = R.signals(fs, n)
    est[lo:hi] = 0.0
    _, grad = R.value_and_grad(clean, est, fs, extended)
    assert np.isfinite(grad).all()
    v = _direction(n)
    v[lo - 256:hi + 256] = 0.0                    # no frame that holds a zeroed sample is moved
    want = _fd(clean, est, fs, extended, v, 1e-6)
    got = float(grad @ v)
    print(extended, f'autograd {got:.9e} central differences {want:.9e}')
    assert abs(got - want) <= 1e-6*abs(want)


def test_no_frame_is_near_the_selection_threshold():
    """The condition under which fp32 kernels and the fp64 restatement select the same frames: no frame's energy
    within 0.05 dB of max - 40 (a 256-term fp32 energy sum errs by about 1e-5 dB)."""
    for (fs, n), (kept, total) in GPU_CASES.items():
        e = R.frame_energies(R.signals(fs, n)[0], fs)
        margin = np.abs(e.max() - 40.0 - e)
        print(fs, n, f'kept {int((e.max() - 40.0 - e < 0).sum())} / {len(e)}, closest {margin.min():.3f} dB')
        assert (int((e.max() - 40.0 - e < 0).sum()), len(e)) == (kept, total)
        assert margin.min() > 0.05
    assert (R.BATCH_FS, R.BATCH_LENGTHS, R.SINGLE_CASES) == (16000, (24000, 17777, 16000, 6000),
                                                             ((8000, 12000), (10000, 16000)))


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_sl_version', 'brv_sl_last_error', 'brv_sl_segment_backward', 'brv_sl_bands_backward',
           'brv_sl_fold_frames', 'brv_sl_compact_backward', 'brv_sl_resample_backward'}
KERNEL_CALLS = sorted(EXPORTS - {'brv_sl_version', 'brv_sl_last_error'})


def test_header_parses_and_every_export_resolves():
    with open(stoi.HEADER_PATH) as f:
        table = hip.parse_header(f.read())
    assert set(table) == EXPORTS == set(stoi.SIGNATURES)
    lib = stoi.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        if name in KERNEL_CALLS:
            assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr, name
    assert lib.brv_sl_version() >= 100
    assert not any(n.startswith('brv_sl_') for n in hip.SIGNATURES)
    assert not hasattr(hip.lib(), 'brv_sl_version')


def _arg_names(name):
    with open(stoi.HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    args = re.search(name + r'\s*\(([^)]*)\)', text).group(1)
    return [a.split()[-1].lstrip('*') for a in args.split(',')]


def _args(name, fill):
    """Arguments a call would accept: every pointer ``fill``, ncols 2, every other number 1, no stream."""
    _, argtypes = stoi.SIGNATURES[name]
    names = _arg_names(name)
    return [None if i == len(argtypes) - 1 else fill if t is hip._c_ptr else 2 if names[i] == 'ncols' else 1
            for i, t in enumerate(argtypes)]


@pytest.mark.parametrize('name', KERNEL_CALLS)
def test_every_export_refuses_null_and_negative(name):
    lib = stoi.lib()
    _, argtypes = stoi.SIGNATURES[name]
    names = _arg_names(name)
    buf = ctypes.create_string_buffer(64)            # never read: each call below is refused on the host
    assert getattr(lib, name)(*_args(name, None)) == -1
    null_msg = lib.brv_sl_last_error()
    assert null_msg and b'null' in null_msg
    for i, t in enumerate(argtypes[:-1]):
        if t is hip._c_ptr:
            args = _args(name, buf)
            args[i] = None
            assert getattr(lib, name)(*args) == -1, (name, names[i])
            assert lib.brv_sl_last_error() == null_msg
            continue
        args = _args(name, buf)
        args[i] = -1
        assert getattr(lib, name)(*args) == -1, (name, names[i])
        msg = lib.brv_sl_last_error()
        assert msg and msg != null_msg and b'requires' in msg, (name, names[i], msg)
        args[i] = 0
        if names[i] not in ('extended', 'clip', 'bin0', 'n_pre_remove'):         # (0 is a value these take)
            assert getattr(lib, name)(*args) == -1, (name, names[i])
    with pytest.raises(RuntimeError, match=name):
        stoi.call(name, *_args(name, None))


# -- the registry ------------------------------------------------------------------------------------------------
def test_criteria_resolve_without_a_device():
    from brever_amd.criterion import CriterionRegistry, EstoiLoss, StoiLoss, init_criterion
    assert {'stoi', 'estoi', 'snr', 'sisnr', 'mse', 'multiresyu'} <= set(CriterionRegistry.keys())
    a, b = init_criterion('stoi'), init_criterion('estoi', fs=8000)
    assert isinstance(a, StoiLoss) and (a.fs, a.extended) == (16000, False)
    assert isinstance(b, EstoiLoss) and (b.fs, b.extended) == (8000, True)
    with pytest.raises(ValueError):
        StoiLoss(fs=0)
    with pytest.raises(RuntimeError, match='ROCm device'):
        a(torch.zeros(1, 4000), torch.zeros(1, 4000), torch.tensor([4000]))
