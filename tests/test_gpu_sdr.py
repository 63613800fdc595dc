"""The BSS-eval SDR on the GPU (brever_amd/sdr.py; csrc/sdr/sdr.hip): the ``sdr`` metric and the ``sdr`` criterion
against the fp64 restatements of tests/sdr_ref.py.

Signals are the recipe of ``sdr_ref.signals`` (white, AR(2), low-pass; a 4-tap filtering of the reference plus noise
at 0 and 40 dB), rounded to fp32 before both sides see them. The forward is compared in dB against formulation (a)
and held to ``FORWARD_BOUND``: the reference spread (the largest |(a) - (b)| over the cases) times 8. Gradients are
rel-L2 against the closed form in fp64 and held to ``GRAD_CAP`` (sdr_ref.py: 16 fp32 rounding floors, five orders
below a one-tap misalignment of ``h``). The correlation kernel's chunk length is ``sdr_ref.CHUNK`` = 2048 samples.
Measured on an MI355X (every case is in DESIGN.md 5k): forward <= 2.48e-10 dB (bound 6.0e-10), gradient 2.4e-8 - 2.9e-8
(cap 1e-6).
"""
import functools
import os
import random

import numpy as np
import pytest
import torch

import sdr_ref as R
from sdr_ref import FORWARD_BOUND, GRAD_CAP

pytestmark = pytest.mark.gpu

VARIANTS = [(kind, db) for kind in R.KINDS for db in R.NOISE_DB]
# a non-uniform upstream gradient, one entry per variant
UPSTREAM = (1.0, 0.5, 2.0, -1.5, 0.25, 3.0)
FLOOR_DB = 10*np.log10(2.0**52)


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda:0')


def _rel(a, b):
    return float(np.linalg.norm(a - b)/np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _case(T, L, load_diag=0.0):
    """``(y (6, T), x (6, T), sdr of (a), closed-form gradient of -SDR)`` over VARIANTS, float64 on the CPU."""
    y, x = (np.stack(a) for a in zip(*[R.signals(kind, T, db) for kind, db in VARIANTS]))
    value = np.array([R.sdr_lstsq(y[i], x[i], L, load_diag)[0] for i in range(len(VARIANTS))])
    grad = np.stack([R.grad_closed(y[i], x[i], L, load_diag) for i in range(len(VARIANTS))])
    return y, x, value, grad


def _run(dev, y, x, lengths, L, load_diag=0.0, upstream=None):
    """Metric (fp64), loss (fp32) and gradient of ``sum(upstream * loss)`` on the GPU."""
    from brever_amd.criterion import init_criterion
    from brever_amd.metrics import MetricRegistry
    yg = torch.as_tensor(y, dtype=torch.float32).to(dev)
    xg = torch.as_tensor(x, dtype=torch.float32).to(dev).requires_grad_(True)
    n = torch.as_tensor(lengths).to(dev)
    metric = MetricRegistry.get('sdr')(xg.detach(), yg, lengths=n, filter_length=L, load_diag=load_diag)
    loss = init_criterion('sdr', filter_length=L, load_diag=load_diag)(xg, yg, n)
    w = torch.ones(len(lengths), device=dev) if upstream is None else torch.tensor(upstream, device=dev)
    grad, = torch.autograd.grad((loss*w).sum(), xg)
    assert metric.dtype == torch.float64 and loss.dtype == torch.float32 and grad.dtype == torch.float32
    return metric.cpu(), loss.detach().cpu(), grad.cpu()


def _check_case(dev, T, L, load_diag=0.0):
    y, x, value, grad = _case(T, L, load_diag)
    metric, loss, got = _run(dev, y, x, [T]*len(VARIANTS), L, load_diag, UPSTREAM)
    err = np.abs(metric.numpy() - value)
    for i, (kind, db) in enumerate(VARIANTS):
        e_grad = _rel(got[i].double().numpy(), UPSTREAM[i]*grad[i])
        print(f'T {T} L {L} ld {load_diag} {kind} {db:.0f} dB: sdr {value[i]:.6f} |gpu - (a)| {err[i]:.2e} dB '
              f'gradient rel-L2 {e_grad:.2e}')
        assert err[i] <= FORWARD_BOUND, (kind, db, err[i])
        assert e_grad <= GRAD_CAP, (kind, db, e_grad)
    assert torch.equal(loss, (-metric).float())
    return metric


@pytest.mark.parametrize('T,L', R.CASES)
def test_value_and_gradient_match_the_fp64_restatement(T, L):
    """(700, 512) puts the halo beyond the row, (300, 512) has T < L, L = 1 and L = 33 leave the 8-lag tiles ragged,
    2047 / 2048 / 2049 sit around the chunk length, 3000 and 16000 are no multiples of it; 16000 sums 8 chunks."""
    _check_case(_cuda(), T, L)


def test_load_diag_matches_the_reference_with_the_same_loading():
    dev = _cuda()
    ld = float(np.float32(1e-3))                   # the loading travels as a C float: this is what enters R
    loaded = _check_case(dev, 3000, 512, ld)
    y, x, _, _ = _case(3000, 512, ld)
    b = np.array([R.sdr_toeplitz(y[i], x[i], 512, ld)[0] for i in range(len(VARIANTS))])
    assert np.abs(loaded.numpy() - b).max() <= FORWARD_BOUND
    plain, _, _ = _run(dev, y, x, [3000]*len(VARIANTS), 512)
    assert (plain - loaded).abs().min() > 1e-4                          # the loading does act


def test_lags_beyond_the_length_are_exactly_zero():
    """T = 300 < L = 512 through the library itself: the only chunk's partial lags are the lags, against np.dot to
    a few ulps of r[0], and exactly 0 from lag T on."""
    from brever_amd import hip, sdr
    dev = _cuda()
    T, L, W = 300, 512, 333
    s, x = R.signals('ar2', T, 40.0)
    yg = torch.full((1, W), 1e30, device=dev)
    xg = torch.full((1, W), -1e30, device=dev)
    yg[0, :T], xg[0, :T] = torch.from_numpy(s).float().to(dev), torch.from_numpy(x).float().to(dev)
    n = torch.tensor([T], device=dev)
    nbytes = sdr.lib().brv_sdr_workspace_bytes(1, W, L)
    assert nbytes == (2*L + 1)*8
    f64 = dict(dtype=torch.float64, device=dev)
    ws = torch.full((2*L + 1,), float('nan'), **f64)
    out = [torch.empty(1, **f64), torch.empty(1, L, **f64), torch.empty(1, **f64), torch.empty(1, **f64),
           torch.empty(1, dtype=torch.int32, device=dev)]
    sdr.call('brv_sdr_forward', xg, yg, n, 1, W, L, 0.0, ws, *out, hip.stream())
    ws = ws.cpu().numpy()
    r, b = R.lags(s, x, L)
    assert not ws[T:L].any() and not ws[L + T:2*L].any()
    assert np.abs(ws[:L] - r).max() <= 1e-13*r[0] and np.abs(ws[L:2*L] - b).max() <= 1e-13*r[0]
    assert abs(ws[2*L] - np.dot(x, x)) <= 1e-13*np.dot(x, x)
    assert int(out[4][0]) == 0 and abs(float(out[0][0]) - R.sdr_lstsq(s, x, L)[0]) <= FORWARD_BOUND


RAGGED = (1, 300, R.CHUNK + 1, 3000, 4500)


def _ragged():
    W = max(RAGGED)
    y = np.full((len(RAGGED), W), 3e30)
    x = np.full((len(RAGGED), W), -7e29)
    for i, n in enumerate(RAGGED):
        y[i, :n], x[i, :n] = R.signals(R.KINDS[i % 3], n, 40.0*(i % 2), seed=3)
    return y, x


def test_ragged_batch_is_bitwise_the_rows_alone_and_repeatable():
    dev = _cuda()
    y, x = _ragged()
    up = (1.0, -2.0, 0.5, 3.0, 0.25)
    first = _run(dev, y, x, RAGGED, 512, upstream=up)
    again = _run(dev, y, x, RAGGED, 512, upstream=up)
    for a, b in zip(first, again):
        assert torch.equal(a, b)                                        # bit for bit, forward and backward
    metric, loss, grad = first
    assert torch.isfinite(metric).all() and torch.isfinite(grad).all()
    for i, n in enumerate(RAGGED):
        assert not grad[i, n:].any()                                    # exactly zero beyond the length
        m1, l1, g1 = _run(dev, y[i:i + 1, :n], x[i:i + 1, :n], [n], 512, upstream=up[i:i + 1])
        assert torch.equal(m1[0], metric[i]) and torch.equal(l1[0], loss[i]), (n, m1, metric[i])
        assert torch.equal(g1[0], grad[i, :n]), n


def test_degenerate_rows_and_the_floor():
    dev = _cuda()
    T, W, L = 1000, 1200, 64
    s, e = R.signals('lowpass', T, 0.0, seed=5)
    y = np.full((3, W), 1e30)
    x = np.full((3, W), 1e30)
    y[0, :T], x[0, :T] = 0.0, e                     # a reference that is zero inside the length
    y[1, :T], x[1, :T] = s, 0.0                     # an all-zero estimate
    y[2, :T], x[2, :T] = s, 0.5*s                   # E - q = 0: the floor of the denominator
    metric, loss, grad = _run(dev, y, x, [T]*3, L, upstream=(2.0, 3.0, 1.5))
    assert torch.isnan(metric[:2]).all() and not loss[:2].any() and not grad[:2].any()
    assert abs(float(metric[2]) - FLOOR_DB) <= 1e-9 and float(loss[2]) == -float(np.float32(float(metric[2])))
    assert torch.isfinite(grad[2]).all() and not grad[2, T:].any()
    # the denominator's term is dropped: -(10/ln 10) 2 s_target / q with s_target = s/2 and q = r[0]/4
    want = 1.5*(-R.K10*4.0*s/np.dot(s, s))
    assert _rel(grad[2, :T].double().numpy(), want) <= GRAD_CAP


def test_middle_axes_take_the_mean_and_half_precision_is_widened():
    from brever_amd.criterion import init_criterion
    dev = _cuda()
    y, x, _, _ = _case(3000, 32)
    crit = init_criterion('sdr', filter_length=32)
    y2 = torch.from_numpy(np.stack([y[:3], y[3:]], 1)).float().to(dev)            # (3, 2, T)
    x2 = torch.from_numpy(np.stack([x[:3], x[3:]], 1)).float().to(dev)
    n = torch.tensor([3000, 2500, 1700], device=dev)
    up = torch.tensor([1.0, -0.5, 2.0], device=dev)
    xg = x2.clone().requires_grad_(True)
    loss = crit(xg, y2, n)
    grad, = torch.autograd.grad((loss*up).sum(), xg)
    assert loss.shape == (3,) and grad.shape == x2.shape
    rows = []
    for s in range(2):
        xs = x2[:, s].clone().requires_grad_(True)
        ls = crit(xs, y2[:, s], n)
        gs, = torch.autograd.grad((ls*up).sum(), xs)
        rows.append(ls)
        assert torch.equal(grad[:, s], 0.5*gs)                          # a power of two: bit for bit
    mean = 0.5*(rows[0].double() + rows[1].double())
    largest = max(float(rows[0].detach().abs().max()), float(rows[1].detach().abs().max()))
    assert (loss.double() - mean).abs().max() <= 2.0**-22*largest                 # fp32 roundings of the three
    for b, m in enumerate(n.tolist()):
        assert not grad[b, :, m:].any()
    # bf16 / fp16 estimates are widened; the gradient comes back in the input's type, the rounded fp32 one
    for dtype in (torch.bfloat16, torch.float16):
        xh = x2.to(dtype)
        x32 = xh.float().requires_grad_(True)
        g32, = torch.autograd.grad(crit(x32, y2, n).sum(), x32)
        x16 = xh.clone().requires_grad_(True)
        l16 = crit(x16, y2, n)
        g16, = torch.autograd.grad(l16.sum(), x16)
        assert l16.dtype == torch.float32 and g16.dtype == dtype
        assert torch.equal(g16, g32.to(dtype)) and g16.float().abs().sum() > 0


def test_metric_batched_equals_one_by_one():
    """The form of test_gpu.py::test_metrics_batched_equals_one_by_one at a tenth of its sizes; here bit for bit."""
    import torch.nn.functional as F
    from brever_amd.metrics import MetricRegistry
    dev = _cuda()
    torch.manual_seed(42)
    lengths = torch.randint(1600, 4800, (2,))
    targets = [torch.randn(int(n)) for n in lengths]
    batched_targets = torch.stack([F.pad(t, (0, 4800 - t.shape[-1])) for t in targets])
    batched_inputs = batched_targets + 0.5*torch.randn(*batched_targets.shape)
    inputs = [x[..., :n] for x, n in zip(batched_inputs, lengths)]
    metric = MetricRegistry.get('sdr')
    batched = metric(batched_inputs.to(dev), batched_targets.to(dev), lengths=lengths.to(dev)).cpu()
    single = [metric(x.to(dev), y.to(dev)) for x, y in zip(inputs, targets)]
    assert all(isinstance(v, float) for v in single)
    assert torch.equal(batched, torch.tensor(single, dtype=torch.float64)), (batched, single)
    assert ((batched > 4.0) & (batched < 12.0)).all()                   # 6 dB of noise, some of it forgiven


SMALL = ['--filters', '64', '--filter_length', '16', '--bottleneck_channels', '32', '--hidden_channels', '64',
         '--skip_channels', '32', '--layers', '2', '--repeats', '2']


def test_entry_points_train_and_score_on_sdr(tmp_path):
    """init_model.py --criterion sdr -> train_model.py for one epoch -> test_model.py --metrics sdr at the smallest
    synthetic sizes of the other script tests: finite loss, changed parameters, finite scores."""
    from helpers import run_entry_points
    from brever_amd.config import get_config
    from brever_amd.models import ModelRegistry
    _cuda()
    model_dir, losses, scores = run_entry_points(
        tmp_path, 'convtasnet', model_args=['--criterion', 'sdr', *SMALL],
        trainer_args=['--epochs', '1', '--val_period', '1', '--batch_size', '4', '--val_metrics', 'sdr'],
        train='synthetic:8:0.5', val='synthetic:2:0.5', test='synthetic:3:0.5', metrics=('sdr', 'snr'))
    assert losses['train_loss'].shape[0] == 1 and np.isfinite(losses['train_loss']).all()
    assert np.isfinite(losses['val_loss']).all() and np.isfinite(losses['metrics_sdr']).all()
    assert scores.shape == (3, 2, 2) and np.isfinite(scores).all()
    cfg = get_config(os.path.join(model_dir, 'config.yaml'))
    assert cfg.model.criterion == 'sdr'
    random.seed(cfg.seed)
    np.random.seed(cfg.seed)
    torch.manual_seed(cfg.seed)
    initial = ModelRegistry.get(cfg.arch)(**cfg.model.to_dict()).state_dict()
    trained = torch.load(os.path.join(model_dir, 'checkpoints', 'last.ckpt'), map_location='cpu',
                         weights_only=False)['model']
    changed = [k for k in initial if not torch.equal(initial[k].cpu(), trained[k].cpu())]
    assert changed and all(torch.isfinite(v).all() for v in trained.values() if v.is_floating_point())
