"""The BSS-eval SDR on the host: the two fp64 formulations of tests/sdr_ref.py against each other (the *reference
spread* of DESIGN.md 5k), the closed-form gradient against autograd, the numbers the gradient cap of the GPU tests
rests on, the C ABI of libbrever_sdr.so (header, exports, refusals) and the registry keys. No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import sdr_ref as R
from brever_amd import hip, sdr
from sdr_ref import FORWARD_BOUND, GRAD_CAP, GRAD_FLOOR, REF_SPREAD

VARIANTS = [(kind, db) for kind in R.KINDS for db in R.NOISE_DB]


def _rel(a, b):
    return float(np.linalg.norm(a - b)/np.linalg.norm(b))


# -- the restatements --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,L', R.CASES)
def test_formulations_agree_and_gradient_is_the_autograd_one(T, L):
    spread = grad_err = floor = 0.0
    misaligned = np.inf
    for kind, db in VARIANTS:
        s, x = R.signals(kind, T, db)
        va, ha = R.sdr_lstsq(s, x, L)
        vb, hb, q, E, cond = R.sdr_toeplitz(s, x, L)
        assert np.isfinite(va) and np.isfinite(vb) and EPS_CLEAR(q, E)
        g = R.grad_closed(s, x, L)
        ga = R.grad_autograd(s, x, L)
        shifted = np.concatenate([[0.0], hb[:-1]])
        e = (abs(va - vb), _rel(g, ga), _rel(g.astype(np.float32).astype(np.float64), g),
             _rel(R.grad_closed(s, x, L, h=shifted), g))
        print(f'T {T} L {L} {kind} {db:.0f} dB: sdr {va:.4f} |a - b| {e[0]:.2e} dB cond(R) {cond:.2e} '
              f'gradient closed vs autograd {e[1]:.2e} fp32 floor {e[2]:.2e} one-tap misalignment {e[3]:.2e}')
        spread, grad_err, floor, misaligned = max(spread, e[0]), max(grad_err, e[1]), max(floor, e[2]), \
            min(misaligned, e[3])
    print(f'T {T} L {L}: spread {spread:.2e} dB, gradient {grad_err:.2e}, floor {floor:.2e}, '
          f'misalignment {misaligned:.2e}')
    # (a) against (b) is held to the bound the GPU gets against (a): the recorded spread times 8
    assert spread <= FORWARD_BOUND == 8*REF_SPREAD
    # autograd goes through the least-squares solve of an operator with cond(S) = sqrt(cond(R)) <= 1.3e3, and the
    # 40 dB rows amplify a relative error of E - q by 1e4: 1e-8 is four orders above fp64 and two below the cap
    assert grad_err <= 1e-8
    assert floor <= GRAD_FLOOR and 16*GRAD_FLOOR <= GRAD_CAP <= 1e-2*misaligned


def EPS_CLEAR(q, E):
    """Neither floor is active on the accuracy cases."""
    return q > R.EPS*E and E - q > R.EPS*E


def test_load_diag_and_the_conventions_of_the_reference():
    s, x = R.signals('ar2', 700, 40.0)
    va, _ = R.sdr_lstsq(s, x, 64, load_diag=1e-3)
    vb, _, q, E, cond = R.sdr_toeplitz(s, x, 64, load_diag=1e-3)
    v0 = R.sdr_toeplitz(s, x, 64)[0]
    print(f'load_diag 1e-3: (a) {va:.9f} (b) {vb:.9f} unloaded {v0:.9f} cond {cond:.2e}')
    assert abs(va - vb) <= FORWARD_BOUND and abs(vb - v0) > 1e-3
    # lags from T on are exactly 0
    r, b = R.lags(s[:20], x[:20], 32)
    assert not r[20:].any() and not b[20:].any() and r[19] == s[0]*s[19]
    # degenerate rows
    z = np.zeros(50)
    for a, c in ((z, x[:50]), (s[:50], z)):
        assert np.isnan(R.sdr_lstsq(a, c, 8)[0]) and np.isnan(R.sdr_toeplitz(a, c, 8)[0])
        assert not R.grad_closed(a, c, 8).any()
    # the floors: q = E sits at the floor of the denominator, q = 0 at that of the numerator
    assert R._ratio(3.0, 3.0) == 10*np.log10(2.0**52) and R._ratio(0.0, 3.0) == -10*np.log10(2.0**52)


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_sdr_version', 'brv_sdr_last_error', 'brv_sdr_max_filter_length', 'brv_sdr_chunk',
           'brv_sdr_workspace_bytes', 'brv_sdr_forward', 'brv_sdr_backward'}


def test_header_parses_and_every_export_resolves():
    with open(sdr.HEADER_PATH) as f:
        table = hip.parse_header(f.read())
    assert set(table) == EXPORTS == set(sdr.SIGNATURES)
    lib = sdr.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    for name in ('brv_sdr_forward', 'brv_sdr_backward'):
        restype, argtypes = table[name]
        assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr, name
    assert table['brv_sdr_forward'][1][6] is ctypes.c_float
    assert lib.brv_sdr_version() >= 100
    assert lib.brv_sdr_max_filter_length() == sdr.MAX_FILTER_LENGTH == 512
    assert lib.brv_sdr_chunk() == R.CHUNK
    # the limits and the flag bits are the header's macros, and the library was compiled from the same ones
    constants = sdr._LIB.constants
    assert constants == {'BRV_SDR_MAX_FILTER_LENGTH': 512, 'BRV_SDR_CHUNK': 2048, 'BRV_SDR_FLAG_NO_REFERENCE': 1,
                         'BRV_SDR_FLAG_NO_ESTIMATE': 2, 'BRV_SDR_FLAG_BAD_PIVOT': 4,
                         'BRV_SDR_FLAG_NUMERATOR_FLOOR': 8, 'BRV_SDR_FLAG_DENOMINATOR_FLOOR': 16}
    assert constants['BRV_SDR_MAX_FILTER_LENGTH'] == sdr.MAX_FILTER_LENGTH == lib.brv_sdr_max_filter_length()
    assert constants['BRV_SDR_CHUNK'] == lib.brv_sdr_chunk()
    assert (sdr.NO_REFERENCE, sdr.NO_ESTIMATE, sdr.BAD_PIVOT, sdr.NUMERATOR_FLOOR, sdr.DENOMINATOR_FLOOR) == \
        tuple(constants['BRV_SDR_FLAG_' + name] for name in (
            'NO_REFERENCE', 'NO_ESTIMATE', 'BAD_PIVOT', 'NUMERATOR_FLOOR', 'DENOMINATOR_FLOOR')) == (1, 2, 4, 8, 16)
    assert sdr.DEGENERATE == 7
    assert not any(n.startswith('brv_sdr_') for n in hip.SIGNATURES)
    assert not hasattr(hip.lib(), 'brv_sdr_version')


def _forward_args(buf, **over):
    a = dict(x=buf, y=buf, lengths=buf, rows=1, stride=8, filter_length=4, load_diag=0.0, workspace=buf, sdr=buf,
             h=buf, q=buf, e=buf, flags=buf, stream=None)
    a.update(over)
    return list(a.values())


def _backward_args(buf, **over):
    a = dict(x=buf, y=buf, lengths=buf, h=buf, q=buf, e=buf, flags=buf, grad_rows=buf, rows=1, stride=8,
             filter_length=4, dx=buf, stream=None)
    a.update(over)
    return list(a.values())


def test_refusals_carry_a_message():
    lib = sdr.lib()
    buf = ctypes.create_string_buffer(64)            # never read: each call below is refused on the host
    for make, fn, pointers in ((_forward_args, lib.brv_sdr_forward,
                                ('x', 'y', 'lengths', 'workspace', 'sdr', 'h', 'q', 'e', 'flags')),
                               (_backward_args, lib.brv_sdr_backward,
                                ('x', 'y', 'lengths', 'h', 'q', 'e', 'flags', 'grad_rows', 'dx'))):
        for p in pointers:
            assert fn(*make(buf, **{p: None})) == -1, p
            msg = lib.brv_sdr_last_error()
            assert msg and b'null' in msg and p.encode() in msg
        for over in (dict(filter_length=0), dict(filter_length=-1), dict(filter_length=513), dict(rows=0),
                     dict(rows=65536), dict(stride=0), dict(stride=-1)):
            assert fn(*make(buf, **over)) == -1, over
            msg = lib.brv_sdr_last_error()
            assert msg and b'requires' in msg and b'filter_length <= 512' in msg, over
    for ld in (-1e-3, float('nan'), float('inf')):
        assert lib.brv_sdr_forward(*_forward_args(buf, load_diag=ld)) == -1
        assert b'load_diag' in lib.brv_sdr_last_error()
    assert lib.brv_sdr_workspace_bytes(1, 8, 513) == -1 and b'requires' in lib.brv_sdr_last_error()
    assert lib.brv_sdr_workspace_bytes(3, 2*R.CHUNK + 1, 512) == 3*3*(2*512 + 1)*8
    with pytest.raises(RuntimeError, match='brv_sdr_forward failed with status -1: null'):
        sdr.call('brv_sdr_forward', *_forward_args(buf, x=None))


def test_python_refuses_cpu_tensors_and_bad_options():
    from brever_amd.criterion import SdrLoss
    from brever_amd.metrics import MetricRegistry
    x, y, n = torch.zeros(1, 400), torch.zeros(1, 400), torch.tensor([400])
    with pytest.raises(RuntimeError, match='ROCm device'):
        SdrLoss()(x, y, n)
    with pytest.raises(RuntimeError, match='ROCm device'):
        MetricRegistry.get('sdr')(x, y, lengths=n)
    with pytest.raises(RuntimeError, match='ROCm device'):
        sdr.forward(x, y, n)
    for bad in (dict(filter_length=0), dict(filter_length=513), dict(filter_length=2.5), dict(load_diag=-1.0),
                dict(load_diag=float('nan'))):
        with pytest.raises(ValueError, match='filter_length|load_diag'):
            SdrLoss(**bad)
        with pytest.raises(ValueError, match='filter_length|load_diag'):
            MetricRegistry.get('sdr')(x, y, **bad)


# -- the registry ------------------------------------------------------------------------------------------------
def test_registry_keys():
    import inspect
    from brever_amd.criterion import CriterionRegistry, SdrLoss, init_criterion
    from brever_amd.metrics import MetricRegistry, metric_available
    assert 'sdr' in CriterionRegistry.keys() and 'sdr' in MetricRegistry.keys() and metric_available('sdr')
    a, b = init_criterion('sdr'), init_criterion('sdr', filter_length=32, load_diag=1e-3)
    assert isinstance(a, SdrLoss) and (a.filter_length, a.load_diag) == (512, 0.0)
    assert (b.filter_length, b.load_diag) == (32, 1e-3)
    params = inspect.signature(MetricRegistry.get('sdr')).parameters
    assert list(params) == ['x', 'y', 'lengths', 'filter_length', 'load_diag']
    assert (params['lengths'].default, params['filter_length'].default, params['load_diag'].default) == \
        (None, 512, 0.0)
