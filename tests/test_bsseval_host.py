"""BSS-eval SIR / SAR on the host: the two fp64 formulations of tests/bsseval_ref.py against each other on every row
the GPU test uses (the *reference spread* of DESIGN.md 5p) with the condition of every system, the NumPy restatement
of the kernel's recursion against (a), the C ABI of the second header of libbrever_sdr.so (exports, refusals), the
registry keys and the ``score`` helper. No GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import bsseval_ref as R
from brever_amd import bsseval, hip, sdr
from bsseval_ref import COND_LIMIT, FORWARD_BOUND, REF_SPREAD


# -- the restatements --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=lambda c: '-'.join(map(str, c)))
def test_formulations_agree_on_every_row_of_the_gpu_test(case):
    J, S, T, L = case
    ld = R.case_load(case)
    spread = recursion = 0.0
    for kind, db in R.case_rows(case):
        s, x, a = R.reference(case, kind, db)
        *b, cond = R.tables_gram(s, x, L, ld)
        *lev, _ = R.tables_gram(s, x, L, ld, solver='levinson')
        e = max(float(np.abs(a[i] - b[i]).max()) for i in range(3))
        r = max(float(np.abs(a[i] - lev[i]).max()) for i in range(3))
        print(f'{case} ld {ld} {kind} {db:.0f} dB: sir {a[1][0, 0]:.4f} sar {a[2][0]:.4f} |a - b| {e:.2e} dB '
              f'|a - recursion| {r:.2e} dB cond(G) {cond:.2e}')
        assert all(np.isfinite(t).all() for t in a)
        # the condition of the inputs: what the bound rests on
        assert cond <= COND_LIMIT, (kind, db, cond)
        spread, recursion = max(spread, e), max(recursion, r)
    print(f'{case}: spread {spread:.2e} dB, recursion {recursion:.2e} dB, bound {FORWARD_BOUND:.2e} dB')
    assert spread <= REF_SPREAD and FORWARD_BOUND == 8*REF_SPREAD
    # the recursion of the kernel, restated in NumPy, stays inside the bound the GPU is held to
    assert recursion <= FORWARD_BOUND


def test_the_low_pass_pair_runs_loaded_only():
    s, x = R.lowpass_pair(1500)
    R_, _ = R.block_lags(s, x, 32)
    unloaded, loaded = np.linalg.cond(R.gram(R_)), np.linalg.cond(R.gram(R_, R.LOAD))
    a = R.tables_lstsq(s, x, 32, R.LOAD)
    *b, _ = R.tables_gram(s, x, 32, R.LOAD)
    *lev, _ = R.tables_gram(s, x, 32, R.LOAD, solver='levinson')
    e = max(float(np.abs(a[i] - b[i]).max()) for i in range(3))
    r = max(float(np.abs(b[i] - lev[i]).max()) for i in range(3))
    print(f'low-pass pair: cond {unloaded:.2e} unloaded, {loaded:.2e} loaded; |a - b| {e:.2e} |b - recursion| {r:.2e}')
    # (unloaded, its condition grows with T and L and is printed only: the pair is never scored unloaded)
    assert loaded <= COND_LIMIT and loaded < unloaded
    assert e <= FORWARD_BOUND and r <= FORWARD_BOUND


def test_conventions_of_the_reference():
    s, x = R.signals('corr', 2, 2, 400, 40.0)
    sdr_, sir, sar = R.tables_lstsq(s, x, 16)
    # unloaded: q1 <= qJ <= E, so SAR >= every SDR of the estimate, and SDR[e][j] < SIR[e][j]
    assert (sar[:, None] >= sdr_).all() and (sir > sdr_).all()
    # the SDR column is that of the single-reference restatement
    import sdr_ref
    for e in range(2):
        for j in range(2):
            assert abs(sdr_[e, j] - sdr_ref.sdr_lstsq(s[j], x[e], 16)[0]) <= 1e-9
    # the brute-force permutation: the largest sum, the smallest among equals, the identity on a NaN
    assert R.best_permutation(np.array([[0.0, 5.0], [5.0, 0.0]]), 2) == (1, 0)
    assert R.best_permutation(np.array([[1.0, 1.0], [1.0, 1.0]]), 2) == (0, 1)
    assert R.best_permutation(np.array([[0.0, 5.0], [np.nan, 0.0]]), 2) == (0, 1)
    assert R.best_permutation(np.array([[0.0, 1.0, 9.0], [9.0, 0.0, 1.0], [1.0, 9.0, 0.0]]), 3) == (2, 0, 1)
    # S < J: only the first S columns are targets
    assert R.best_permutation(np.array([[0.0, 1.0, 50.0], [1.0, 0.0, 50.0]]), 2) == (1, 0)


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_bss_max_references', 'brv_bss_workspace_bytes', 'brv_bss_eval'}
SDR_EXPORTS = {'brv_sdr_version', 'brv_sdr_last_error', 'brv_sdr_max_filter_length', 'brv_sdr_chunk',
               'brv_sdr_workspace_bytes', 'brv_sdr_forward', 'brv_sdr_backward'}


def test_header_parses_and_every_export_resolves():
    with open(bsseval.HEADER_PATH) as f:
        text = f.read()
    table = hip.parse_header(text)
    assert {n for n in table if n.startswith('brv_bss_')} == EXPORTS
    assert set(table) == EXPORTS | {'brv_sdr_last_error'} == set(bsseval.SIGNATURES)
    assert bsseval.LIB_PATH == sdr.LIB_PATH
    lib = bsseval.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    restype, argtypes = table['brv_bss_eval']
    assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr and argtypes[8] is ctypes.c_float
    assert lib.brv_bss_max_references() == bsseval.MAX_REFERENCES == 4 and bsseval.MIN_REFERENCES == 2
    assert hip.parse_constants(text) == {
        'BRV_BSS_MIN_REFERENCES': 2, 'BRV_BSS_MAX_REFERENCES': 4, 'BRV_BSS_MAX_FILTER_LENGTH': 512,
        'BRV_BSS_FLAG_NO_REFERENCE': 1, 'BRV_BSS_FLAG_BAD_PIVOT': 4, 'BRV_BSS_FLAG_NO_ESTIMATE': 2,
        'BRV_BSS_FLAG_SAR_NUMERATOR_FLOOR': 8, 'BRV_BSS_FLAG_SAR_DENOMINATOR_FLOOR': 16,
        'BRV_BSS_FLAG_SIR_NUMERATOR_FLOOR': 32, 'BRV_BSS_FLAG_SIR_DENOMINATOR_FLOOR': 64}
    # the degenerate bits mean what they mean in brever_sdr.h
    assert (bsseval.NO_REFERENCE, bsseval.NO_ESTIMATE, bsseval.BAD_PIVOT) == \
        (sdr.NO_REFERENCE, sdr.NO_ESTIMATE, sdr.BAD_PIVOT)


def test_the_table_of_brever_sdr_h_is_unchanged():
    with open(sdr.HEADER_PATH) as f:
        assert set(hip.parse_header(f.read())) == SDR_EXPORTS == set(sdr.SIGNATURES)
    assert sdr.lib().brv_sdr_version() >= 100


def _args(buf, **over):
    a = dict(x=buf, s=buf, lengths=buf, items=1, estimates=1, references=2, stride=8, filter_length=4, load_diag=0.0,
             permute=1, workspace=buf, sdr=buf, sir=buf, sar=buf, perm=buf, sdr_table=buf, sir_table=buf,
             item_flags=buf, estimate_flags=buf, stream=None)
    a.update(over)
    return list(a.values())


def test_refusals_carry_a_message():
    lib = bsseval.lib()
    buf = ctypes.create_string_buffer(64)            # never read: each call below is refused on the host
    for p in ('x', 's', 'lengths', 'workspace', 'sdr', 'sir', 'sar', 'perm', 'sdr_table', 'sir_table', 'item_flags',
              'estimate_flags'):
        assert lib.brv_bss_eval(*_args(buf, **{p: None})) == -1, p
        msg = lib.brv_sdr_last_error()
        assert msg and b'null' in msg and p.encode() in msg
    for over in (dict(references=1), dict(references=5), dict(estimates=3), dict(estimates=0),
                 dict(references=4, estimates=5), dict(filter_length=0), dict(filter_length=513), dict(items=0),
                 dict(items=65536), dict(stride=0)):
        assert lib.brv_bss_eval(*_args(buf, **over)) == -1, over
        msg = lib.brv_sdr_last_error()
        assert msg and b'requires' in msg and b'2 <= references <= 4' in msg and b'estimates <= references' in msg \
            and b'filter_length <= 512' in msg, over
        shape = {k: over.get(k, d) for k, d in (('items', 1), ('estimates', 1), ('references', 2), ('stride', 8),
                                                ('filter_length', 4))}
        assert lib.brv_bss_workspace_bytes(*shape.values()) == -1 and b'requires' in lib.brv_sdr_last_error()
    for ld in (-1e-3, float('nan'), float('inf')):
        assert lib.brv_bss_eval(*_args(buf, load_diag=ld)) == -1
        assert b'load_diag' in lib.brv_sdr_last_error()
    assert lib.brv_bss_workspace_bytes(1, 1, 2, 8, 4) > 0
    with pytest.raises(RuntimeError, match='brv_bss_eval failed with status -1: null'):
        bsseval.call('brv_bss_eval', *_args(buf, x=None))


def test_python_refuses_cpu_tensors_and_bad_arguments():
    x, s = torch.zeros(2, 1, 400), torch.zeros(2, 2, 400)
    with pytest.raises(RuntimeError, match='ROCm device'):
        bsseval.bss_eval(x, s)
    for est, ref in ((x, torch.zeros(2, 1, 400)), (x, torch.zeros(2, 5, 400)), (torch.zeros(2, 3, 400), s),
                     (x, torch.zeros(3, 2, 400)), (x, torch.zeros(2, 2, 399)), (x[0], s)):
        with pytest.raises(ValueError, match='references|estimates'):
            bsseval.bss_eval(est, ref)
    for bad in (dict(filter_length=0), dict(filter_length=513), dict(load_diag=-1.0)):
        with pytest.raises(ValueError, match='filter_length|load_diag'):
            bsseval.bss_eval(x, s, **bad)


# -- the registry and the helper ---------------------------------------------------------------------------------
def test_registry_keys_and_noise_is_required():
    from brever_amd.metrics import MetricRegistry, metric_available
    for name in ('sir', 'sar'):
        assert name in MetricRegistry.keys() and metric_available(name)
        params = inspect.signature(MetricRegistry.get(name)).parameters
        assert list(params) == ['x', 'y', 'lengths', 'noise', 'filter_length', 'load_diag']
        assert (params['lengths'].default, params['noise'].default, params['filter_length'].default,
                params['load_diag'].default) == (None, None, 512, 0.0)
        with pytest.raises(ValueError, match=f"'{name}' metric needs a second reference.*noise"):
            MetricRegistry.get(name)(torch.zeros(2, 400), torch.zeros(2, 400))
        with pytest.raises(RuntimeError, match='ROCm device'):
            MetricRegistry.get(name)(torch.zeros(2, 400), torch.zeros(2, 400), noise=torch.zeros(2, 400))
        with pytest.raises(ValueError, match='filter_length'):
            MetricRegistry.get(name)(torch.zeros(2, 400), torch.zeros(2, 400), noise=torch.zeros(2, 400),
                                     filter_length=513)
    # the existing key keeps its signature
    assert list(inspect.signature(MetricRegistry.get('sdr')).parameters) == \
        ['x', 'y', 'lengths', 'filter_length', 'load_diag']


def test_score_passes_noise_only_to_the_metrics_that_take_it(monkeypatch):
    from brever_amd import metrics
    calls = []

    def plain(x, y, lengths=None):
        calls.append(('plain', x, y, lengths))
        return 1.0

    def with_noise(x, y, lengths=None, noise=None, filter_length=512):
        calls.append(('with_noise', x, y, lengths, noise))
        return 2.0

    stubs = {'plain': plain, 'with_noise': with_noise}
    monkeypatch.setattr(metrics.MetricRegistry, 'get', lambda name: stubs[name])
    x, target, mixture, n = torch.ones(2, 8), torch.full((2, 8), 3.0), torch.full((2, 8), 5.0), torch.tensor([8, 6])
    assert metrics.score('plain', x, target, n, mixture=mixture) == 1.0
    assert metrics.score('plain', x, target, n) == 1.0
    assert metrics.score('with_noise', x, target, n, mixture=mixture) == 2.0
    (k0, x0, y0, n0), (k1, *_), (k2, x2, y2, n2, noise) = calls
    assert (k0, k1, k2) == ('plain', 'plain', 'with_noise')
    assert x0 is x and y0 is target and n0 is n and x2 is x and y2 is target and n2 is n
    assert torch.equal(noise, mixture - target)
    with pytest.raises(ValueError, match='needs the mixture'):
        metrics.score('with_noise', x, target, n)
