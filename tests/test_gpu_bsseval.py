"""BSS-eval SDR / SIR / SAR on the GPU (brever_amd/bsseval.py; csrc/sdr/bsseval.cuh) against the fp64 restatements
of tests/bsseval_ref.py.

Signals are the recipe of ``bsseval_ref.signals`` (white, AR(2) or a correlated pair of references; every estimate a
4-tap filtering of its target plus 0.3 times the other references plus noise at 0 and 40 dB), rounded to fp32 before
both sides see them. The three tables are compared in dB against formulation (a), the explicit least squares, and
held to ``FORWARD_BOUND``: the reference spread (the largest |(a) - (b)| over the rows, tests/test_bsseval_host.py)
times 8. The case with ``T + L - 1 < J L`` has a singular joint system and runs with ``load_diag = 1e-3`` on both
sides (``bsseval_ref.case_load``). Measured on an MI355X: DESIGN.md 5p.
"""
import numpy as np
import pytest
import torch

import bsseval_ref as R
from bsseval_ref import FLOOR_DB, FORWARD_BOUND

pytestmark = pytest.mark.gpu


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda:0')


def _eval(dev, s, x, lengths=None, **kw):
    """``bss_eval`` of float64 host arrays ``s (B, J, T)``, ``x (B, S, T)``; every field back on the CPU."""
    from brever_amd.bsseval import bss_eval
    out = bss_eval(torch.tensor(x, dtype=torch.float32).to(dev), torch.tensor(s, dtype=torch.float32).to(dev),
                   None if lengths is None else torch.as_tensor(lengths).to(dev), **kw)
    assert all(t.dtype == torch.float64 for t in (out.sdr, out.sir, out.sar, out.sdr_table, out.sir_table))
    assert out.perm.dtype == torch.int64 and out.item_flags.dtype == out.estimate_flags.dtype == torch.int32
    return type(out)(*(t.cpu() for t in out))


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return all(torch.equal(_bits(u) if u.dtype == torch.float64 else u, _bits(v) if v.dtype == torch.float64 else v)
               for u, v in zip(a, b))


def _check_perm(out, S):
    """The assignment is the brute force on the GPU's own table, and the outputs are the table's entries at it."""
    for b in range(out.perm.shape[0]):
        p = R.best_permutation(out.sir_table[b].numpy(), S)
        assert tuple(out.perm[b].tolist()) == p, (b, out.perm[b], p)
        for e in range(S):
            assert _bits(out.sdr[b, e]) == _bits(out.sdr_table[b, e, p[e]])
            assert _bits(out.sir[b, e]) == _bits(out.sir_table[b, e, p[e]])


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: '-'.join(map(str, c)))
def test_tables_match_the_least_squares_restatement(case):
    from brever_amd.metrics import MetricRegistry
    dev = _cuda()
    J, S, T, L = case
    ld = R.case_load(case)
    rows = R.case_rows(case)
    refs = [R.reference(case, kind, db) for kind, db in rows]
    s, x = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    out = _eval(dev, s, x, filter_length=L, load_diag=ld)
    worst = 0.0
    for b, ((kind, db), (_, _, (sdr_a, sir_a, sar_a))) in enumerate(zip(rows, refs)):
        e = [float(np.abs(got.numpy() - want).max()) for got, want in (
            (out.sdr_table[b], sdr_a), (out.sir_table[b], sir_a), (out.sar[b], sar_a))]
        print(f'{case} ld {ld} {kind} {db:.0f} dB: |gpu - (a)| sdr {e[0]:.2e} sir {e[1]:.2e} sar {e[2]:.2e} dB')
        worst = max(worst, *e)
    print(f'{case}: worst {worst:.2e} dB, bound {FORWARD_BOUND:.2e} dB')
    assert not out.item_flags.any() and not out.estimate_flags.any()
    assert worst <= FORWARD_BOUND
    _check_perm(out, S)
    # SDR[e][j] has the bits of the sdr metric on the row (x_e, s_j)
    xs = torch.as_tensor(x, dtype=torch.float32).to(dev)
    ss = torch.as_tensor(s, dtype=torch.float32).to(dev)
    for e in range(S):
        for j in range(J):
            single = MetricRegistry.get('sdr')(xs[:, e], ss[:, j], filter_length=L, load_diag=ld).cpu()
            assert torch.equal(_bits(single), _bits(out.sdr_table[:, e, j])), (e, j)


def test_the_low_pass_pair_with_loading_matches_the_dense_solve():
    dev = _cuda()
    s, x = R.lowpass_pair(1500)
    *b, cond = R.tables_gram(s, x, 32, R.LOAD)
    out = _eval(dev, s[None], x[None], filter_length=32, load_diag=R.LOAD)
    e = [float(np.abs(got.numpy() - want).max()) for got, want in (
        (out.sdr_table[0], b[0]), (out.sir_table[0], b[1]), (out.sar[0], b[2]))]
    print(f'low-pass pair, load_diag 1e-3, cond {cond:.2e}: |gpu - (b)| sdr {e[0]:.2e} sir {e[1]:.2e} sar {e[2]:.2e}')
    assert max(e) <= FORWARD_BOUND and not out.item_flags.any()


def test_permutations():
    dev = _cuda()
    # S = 2: the estimates handed over in swapped order
    case = (2, 2, R.CHUNK, 64)
    s, x, _ = R.reference(case, 'white', 40.0)
    straight = _eval(dev, s[None], x[None], filter_length=64)
    swapped = _eval(dev, s[None], x[None, ::-1].copy(), filter_length=64)
    _check_perm(swapped, 2)
    assert swapped.perm.tolist() == [[1, 0]] and straight.perm.tolist() == [[0, 1]]
    for name in ('sdr', 'sir', 'sar'):
        assert torch.equal(_bits(getattr(swapped, name)), _bits(getattr(straight, name).flip(1))), name
    fixed = _eval(dev, s[None], x[None, ::-1].copy(), filter_length=64, permute=False)
    assert fixed.perm.tolist() == [[0, 1]] and torch.equal(_bits(fixed.sir_table), _bits(swapped.sir_table))
    assert torch.equal(_bits(fixed.sir[0]), _bits(fixed.sir_table[0].diagonal()))
    # S = 3: a cyclic shift
    case = (3, 3, 3000, 33)
    s, x, _ = R.reference(case, 'ar2', 0.0)
    shifted = _eval(dev, s[None], x[None, [1, 2, 0]], filter_length=33)
    _check_perm(shifted, 3)
    assert shifted.perm.tolist() == [[1, 2, 0]]
    # an exact tie: two identical estimates have identical rows in the table, and the smaller p wins
    s, x, _ = R.reference((2, 2, R.CHUNK, 64), 'corr', 0.0)
    tie = _eval(dev, s[None], np.stack([x[1], x[1]])[None], filter_length=64)
    assert torch.equal(_bits(tie.sir_table[0, 0]), _bits(tie.sir_table[0, 1])) and tie.perm.tolist() == [[0, 1]]
    # S < J: only the first S references are targets, however well the interferer matches
    s, x, _ = R.reference((4, 2, 1500, 64), 'white', 40.0)
    x2 = np.stack([x[0], R._f32(s[3] + 0.01*s[1])])
    out = _eval(dev, s[None], x2[None], filter_length=64)
    _check_perm(out, 2)
    assert out.sir_table[0, 1, 3] > out.sir_table[0, 1, :2].max() + 20 and out.perm.tolist() == [[0, 1]]


def test_estimates_inside_the_span_sit_on_the_floors():
    dev = _cuda()
    T, L = 1500, 64
    s, _ = R.signals('white', 2, 1, T, 0.0, seed=5)
    s = np.round(s*2.0**12)/2.0**12                # s_0 + s_1 is exact in fp32, and every lag is exact in fp64
    s[:, T - 8:] = 0.0                             # a filtering of up to 8 taps ends inside the T samples
    mix = s[0] + s[1]
    # a filtering by powers of two, one tap or several: x is exact in fp32 and lies in the span, so E - qJ is rounding
    # of the recursion alone and has to stay below the floor eps E = 2 ulp of E (with one tap C[0] is exact and it is 0)
    for taps in ((0.5,), (0.5, 0.0, 0.0, 0.25), (0.25, 0.5, -0.125, 1.0, 0.0, 0.5)):
        x = np.convolve(mix, taps)[:T]
        assert np.array_equal(x, R._f32(x))
        out = _eval(dev, s[None], x[None, None], filter_length=L)
        print(f'x = fir{taps} (s_0 + s_1): sar {out.sar.item():.12f} floor {FLOOR_DB:.12f} '
              f'flags {out.estimate_flags.item()}')
        assert abs(out.sar.item() - FLOOR_DB) <= 1e-9
    # any other filtering is rounded to fp32, which leaves 2^-50 / 3 of E outside the span: at least 140 dB
    x = R._f32(np.convolve(mix, (0.7, -0.3, 0.2, 0.1, 0.05))[:T])
    out = _eval(dev, s[None], x[None, None], filter_length=L)
    print(f'x = fir(0.7, -0.3, 0.2, 0.1, 0.05) (s_0 + s_1): sar {out.sar.item():.3f}')
    assert out.sar.item() >= 140.0
    # x = s_0 exactly: nothing of s_1, nothing outside the span; SDR on its own floor as for x = 0.5 s
    for kind in ('white', 'corr'):
        s, _ = R.signals(kind, 2, 1, T, 0.0, seed=6)
        out = _eval(dev, s[None], s[None, :1], filter_length=L)
        print(f'x = s_0 ({kind}): sdr {out.sdr.item():.6f} sir {out.sir.item():.6f} sar {out.sar.item():.6f}')
        for v in (out.sdr, out.sir, out.sar):
            assert abs(v.item() - FLOOR_DB) <= 1e-9
        assert np.isfinite(out.sdr_table.numpy()).all() and np.isfinite(out.sir_table.numpy()).all()


def test_ragged_batch_is_repeatable_and_items_do_not_see_each_other():
    from brever_amd import bsseval
    dev = _cuda()
    lengths = [1, 300, 2049, 3000, 4500]
    W, L = max(lengths), 64
    s, x = np.full((5, 2, W), 3e30), np.full((5, 2, W), 3e30)
    for b, n in enumerate(lengths):
        s[b, :, :n], x[b, :, :n] = R.signals(R.KINDS[b % 3], 2, 2, n, 40.0*(b % 2), seed=7)
    first = _eval(dev, s, x, lengths, filter_length=L)
    again = _eval(dev, s, x, lengths, filter_length=L)
    assert _same(first, again)
    for b, n in enumerate(lengths):
        alone = _eval(dev, s[b:b + 1, :, :n], x[b:b + 1, :, :n], filter_length=L)
        assert _same([t[b:b + 1] for t in first], alone), b
    # T = 1: R(0) = s s^T has rank 1
    assert first.item_flags.tolist() == [bsseval.BAD_PIVOT, 0, 0, 0, 0]
    assert torch.isnan(first.sir_table[0]).all() and torch.isnan(first.sar[0]).all()
    assert torch.isfinite(first.sir_table[1:]).all() and torch.isfinite(first.sar[1:]).all()
    assert torch.isfinite(first.sdr_table[1:]).all() and first.perm[0].tolist() == [0, 1]


def test_degenerate_signals_stay_inside_their_item():
    from brever_amd import bsseval
    dev = _cuda()
    T, L = 700, 33
    s, x = (np.stack(a) for a in zip(*[R.signals('white', 2, 2, T, 40.0, seed=10 + b) for b in range(3)]))
    clean = _eval(dev, s, x, filter_length=L)
    s[1, 1] = 0.0                                   # a silent reference
    x[2, 0] = 0.0                                   # a silent estimate
    out = _eval(dev, s, x, filter_length=L)
    assert _same([t[:1] for t in out], [t[:1] for t in clean])
    assert out.item_flags.tolist() == [0, bsseval.NO_REFERENCE, 0]
    assert torch.isnan(out.sir_table[1]).all() and torch.isnan(out.sar[1]).all() and out.perm[1].tolist() == [0, 1]
    assert torch.isfinite(out.sdr_table[1, :, 0]).all() and torch.isnan(out.sdr_table[1, :, 1]).all()
    assert out.estimate_flags[2].tolist() == [bsseval.NO_ESTIMATE, 0]
    assert torch.isnan(out.sir_table[2, 0]).all() and torch.isnan(out.sar[2, 0])
    assert torch.isnan(out.sdr_table[2, 0]).all()
    assert torch.equal(_bits(out.sir_table[2, 1]), _bits(clean.sir_table[2, 1]))
    assert torch.equal(_bits(out.sar[2, 1]), _bits(clean.sar[2, 1])) and out.perm[2].tolist() == [0, 1]


def test_sir_sar_sdr_through_the_registry():
    from brever_amd.metrics import MetricRegistry, score
    dev = _cuda()
    case = (2, 1, 3000, 512)
    rows = R.case_rows(case)[:3]
    refs = [R.reference(case, kind, db) for kind, db in rows]
    f32 = lambda a: torch.as_tensor(np.stack(a), dtype=torch.float32).to(dev)      # noqa: E731
    target, other, x = f32([r[0][0] for r in refs]), f32([r[0][1] for r in refs]), f32([r[1][0] for r in refs])
    lengths = torch.tensor([3000, 3000, 3000], device=dev)
    got = {name: MetricRegistry.get(name)(x, target, lengths=lengths, noise=other) for name in ('sir', 'sar')}
    got['sdr'] = MetricRegistry.get('sdr')(x, target, lengths=lengths)
    for i, (_, _, (sdr_a, sir_a, sar_a)) in enumerate(refs):
        for name, want in (('sdr', sdr_a[0, 0]), ('sir', sir_a[0, 0]), ('sar', sar_a[0])):
            assert got[name].dtype == torch.float64 and got[name].shape == (3,)
            assert abs(got[name][i].item() - want) <= FORWARD_BOUND, (i, name)
            kw = {} if name == 'sdr' else dict(noise=other[i])
            single = MetricRegistry.get(name)(x[i], target[i], **kw)
            assert isinstance(single, float) and np.float64(single).tobytes() == got[name][i].cpu().numpy().tobytes()
    # the helper: noise = mixture - target
    mixture = target + other
    for name in ('sdr', 'sir', 'sar'):
        kw = {} if name == 'sdr' else dict(noise=mixture - target)
        direct = MetricRegistry.get(name)(x, target, lengths=lengths, **kw)
        assert torch.equal(_bits(score(name, x, target, lengths, mixture=mixture).cpu()), _bits(direct.cpu())), name
    # (B, K, L) noise: a third reference that the estimate does not contain leaves SIR and SAR finite
    extra = torch.stack([other, other.flip(-1)], dim=1)
    more = MetricRegistry.get('sar')(x, target, lengths=lengths, noise=extra, filter_length=64)
    assert more.shape == (3,) and torch.isfinite(more).all()
    # the input column of sar: a mixture scored against its own two components is in their span. On the white rows
    # cond(G) is about 20, so qJ carries a few times 20 x 2^-52 of E, and fp32 rounding of mixture - target 2^-50
    sar_in = score('sar', mixture, target, lengths, mixture=mixture)
    print(f'sar of the mixture itself: {sar_in.tolist()}')
    assert [kind for kind, _ in rows[:2]] == ['white', 'white'] and (sar_in[:2] >= 140.0).all()


def test_trainer_logs_sir_and_sar_as_validation_metrics(tmp_path):
    """init_model.py -> train_model.py with ``--val_metrics sir,sar`` (``BreverTrainer.compute_metrics`` hands the
    mixture to ``metrics.score``) -> test_model.py, which is unchanged and scores ``sdr``."""
    from helpers import run_entry_points
    _, losses, scores = run_entry_points(
        tmp_path, 'ffnn', model_args=['--hidden_layers', '64'],
        trainer_args=['--epochs', '1', '--val_period', '1', '--batch_size', '8', '--val_metrics', 'sir,sar'],
        train='synthetic:8:1.0', val='synthetic:2:1.0', test='synthetic:3:1.0', metrics=('sdr',))
    print(f"val sir {losses['metrics_sir']} sar {losses['metrics_sar']}; sdr [mixture, 1, (input, output)]:\n{scores}")
    assert np.isfinite(losses['metrics_sir']).all() and np.isfinite(losses['metrics_sar']).all()
    assert scores.shape == (3, 1, 2) and np.isfinite(scores).all()
