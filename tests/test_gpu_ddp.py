"""Data parallelism of the models that are not Conv-TasNet, and `bench.py`'s N > 1 code, on the one GPU of the box.

The reference wraps any model in DistributedDataParallel (brever/training.py:62-63); here every model that owns a
flat gradient hands it to `GradSynchronizer.__call__` once per step (brever_amd/parallel.py). Two gloo ranks share
cuda:0 (gloo moves CUDA tensors through the host), each on half of a batch; the check is a single process that
computes the two half-batch gradients itself, averages them and takes the same optimizer step. (Not "the union
batch": DCCRN's batch norms use per-rank statistics, as in the reference -- no SyncBN.)
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _spawn(worker, make_args, nprocs):
    """mp.spawn with a fresh rendezvous port per attempt: the port `_free_port` found can be taken again before rank 0
    listens on it (seen once in a full run: 'failed to listen on any local network address', EADDRINUSE)."""
    import torch.multiprocessing as mp
    for attempt in range(3):
        try:
            mp.spawn(worker, args=make_args(_free_port()), nprocs=nprocs, join=True)
            return
        except Exception as e:       # noqa: BLE001 (ProcessRaisedException carries the child's traceback as text)
            if attempt == 2 or not any(k in str(e) for k in ('failed to listen', 'EADDRINUSE', 'Address already in use')):
                raise


def _build(kind, dev, hooks):
    if kind == 'dccrn':
        from brever_amd.models.dccrn import DCCRN
        prev = DCCRN._fused_adam
        if hooks:             # a model without the flat buffer: GradSynchronizer installs per-parameter hooks
            DCCRN._fused_adam = False
        try:                  # (the class attribute is restored whatever construction does: ADVICE r5)
            net = DCCRN(channels=[8, 16, 32, 32], lstm_channels=32).to(dev)
        finally:
            DCCRN._fused_adam = prev
        if hooks:
            net._fused_adam = False
        n = 12000
    else:
        from brever_amd.models import TFGridNet
        net = TFGridNet(n_fft=32, stride=16, n_layers=2, lstm_hidden_units=16, attn_n_head=2,
                        attn_approx_qk_dim=34, emb_dim=8).to(dev)
        n = 4000
    g = torch.Generator().manual_seed(9)
    batch = 0.1*torch.randn(4, 2, 2, n, generator=g)
    batch = batch.mean(dim=2) if kind == 'dccrn' else batch           # (B, 2, L) | (B, 2, 2, L)
    batch = batch.to(dev)
    lengths = torch.tensor([n, n - 500, n - 100, n - 900], device=dev)
    return net, batch, lengths


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def _rank_worker(rank, world, port, out_dir, kind, amp, hooks):
    import torch.distributed as dist
    from brever_amd.parallel import GradSynchronizer, broadcast_parameters
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    dev = torch.device('cuda', 0)
    torch.manual_seed(100 + rank)                   # different init per rank until the broadcast
    net, batch, lengths = _build(kind, dev, hooks)
    broadcast_parameters(net)
    sync = GradSynchronizer(net)
    assert sync.flat_model == (not hooks)
    scaler = torch.amp.GradScaler('cuda', enabled=False)
    lo, hi = 2*rank, 2*rank + 2
    seen = []
    if not hooks:
        inner = net._grad_sync

        def spy(flat):
            scale = inner(flat)
            seen.append(flat.detach().clone()*scale)
            return scale
        net._grad_sync = spy
    if kind == 'dccrn' and amp and not hooks:
        import brever_amd.models.dccrn as D
        assert D._WGRAD_SIDE                        # the side stream is on: the case ADVICE r4 (high) is about
    for step in range(2):
        net.train_step(batch[lo:hi], lengths[lo:hi], amp, scaler)
        if hooks and step == 0:     # (the hooks left the mean in the .grad tensors)
            seen = [torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()]
    n_params = sum(1 for _ in net.parameters())
    torch.save({'params': _flat(net).cpu(), 'grad0': seen[0].cpu(), 'calls': sync.calls, 'n_params': n_params},
               os.path.join(out_dir, f'r{rank}.pt'))
    dist.destroy_process_group()


def _rel(a, b):
    return float((a.double() - b.double()).norm()/b.double().norm())


@pytest.mark.parametrize('kind,amp,hooks', [('dccrn', True, False), ('dccrn', False, False), ('tfgridnet', True, False),
                                            ('tfgridnet', False, False), ('dccrn', True, True)])
def test_two_ranks_equal_the_mean_of_the_half_batch_gradients(tmp_path, kind, amp, hooks):
    """VERDICT r4 item 2 / ADVICE r4 (high). DCCRN `use_amp` runs with its weight gradients on the side stream; the
    `hooks` case is the same model WITHOUT a flat buffer (per-parameter all-reduce from inside backward): the side
    stream must switch itself off there."""
    _spawn(_rank_worker, lambda port: (2, port, str(tmp_path), kind, amp, hooks), 2)
    r0, r1 = torch.load(tmp_path/'r0.pt'), torch.load(tmp_path/'r1.pt')
    assert torch.equal(r0['params'], r1['params'])              # the ranks stay in lock-step
    if hooks:
        assert r0['calls'] == 2*r0['n_params']                  # one collective per parameter and step
    else:
        assert r0['calls'] == 2                                  # ONE collective per step
    dev = torch.device('cuda', 0)
    torch.manual_seed(100)
    net, batch, lengths = _build(kind, dev, hooks)
    scaler = torch.amp.GradScaler('cuda', enabled=False)
    first = None
    for _ in range(2):
        halves = []
        for lo in (0, 2):
            net.zero_grad(set_to_none=True)
            net.loss(batch[lo:lo + 2], lengths[lo:lo + 2], amp).backward()
            if kind == 'dccrn':
                import brever_amd.models.dccrn as D
                D._join_side(dev)
            halves.append(torch.cat([p.grad.reshape(-1) for p in net.parameters()]))
        mean = 0.5*(halves[0] + halves[1])
        first = mean if first is None else first
        o = 0
        for p in net.parameters():
            p.grad = mean[o:o + p.numel()].view_as(p).clone()
            o += p.numel()
        # the optimizer step of `update` without its backward pass
        clip = 5.0 if kind == 'dccrn' else net.grad_clip
        from brever_amd.optim import FlatAdam
        if isinstance(net.optimizer, FlatAdam):
            net.optimizer.step(max_norm=clip)
        else:
            torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
            net.optimizer.step()
    # two passes over the same data are not bitwise equal (atomics in the split reductions: up to 3e-3 of a tensor
    # between two identical passes, tests/test_gpu_cconv.py); a race (unwritten weight gradients), a sum instead of a
    # mean or a missing tensor is O(0.1 .. 1)
    print(kind, amp, hooks, 'grad', _rel(r0['grad0'], first.cpu()), 'params', _rel(r0['params'], _flat(net).cpu()))
    assert _rel(r0['grad0'], first.cpu()) <= 5e-3
    assert _rel(r0['params'], _flat(net).cpu()) <= 1e-3


def _run_bench(extra, env_extra=None, nproc=1, single=False):   # (`single`: no process group, as the driver's N = 1 run)
    env = dict(os.environ, BRV_DIST_TIMEOUT_S='300', **(env_extra or {}))
    if nproc > 1:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={nproc}',
               '--master-addr', '127.0.0.1', '--master-port', str(_free_port())]
    else:
        cmd = [sys.executable]
        env['MASTER_PORT'] = str(_free_port())
    cmd += [os.path.join(ROOT, 'bench.py'), '--gpus', str(nproc), '--steps', '3', '--warmup', '3',
            '--no-cpu-baseline', '--no-fp32-path'] + extra
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]                  # rank 0 prints ONE line
    return json.loads(lines[0])


def test_bench_world_one_rccl_runs_every_distributed_branch():
    """bench.py's N > 1 code (process group, broadcast, bucketed all-reduce, exposed-time
    reduce, batch-count check, rank-0 JSON) on RCCL with one rank."""
    line = _run_bench(['--dist'])
    assert line['n_gpus'] == 1 and line['rccl_world_size'] == 1
    assert line['allreduce_buckets'] == 3 and line['allreduce_exposed_ms'] >= 0.0
    assert line['through_trainer']['batches_per_rank'] == 3 + 6
    assert line['value'] > 0 and line['roofline']['frac'] > 0


@pytest.mark.parametrize('forced', [False, True])
def test_bench_two_ranks_on_one_gpu(forced):
    """The same file under `torch.distributed.run` with two ranks sharing cuda:0 over gloo (what the driver's
    8-GPU job runs, minus RCCL), once through the single-all-reduce fallback branch."""
    line = _run_bench(['--dist-backend', 'gloo'], {'BRV_FORCE_AR_FALLBACK': '1'} if forced else None, nproc=2)
    assert line['n_gpus'] == 2 and line['rccl_world_size'] == 2
    assert line['config']['global_batch'] == 32 and line['config']['parallelism'] == 'dp2'
    assert line['through_trainer']['batches_per_rank'] == 3 + 6
    assert ('allreduce_fallback' in line) == forced
    assert line['allreduce_buckets'] == (1 if forced else 3)
    assert line['value_includes_h2d'] is False and line['through_trainer']['includes_h2d'] is True


def test_bench_single_process_line_carries_other_configs_repeats_and_clock(tmp_path):
    """the driver's own command (`bench.py --gpus 1`, no process group) reports BASELINE
    configs[3] (DCCRN bf16 train step) and configs[4] (SGMSE+ fp16 enhance, batch 1 and 8) beside the headline, a
    time-based warm-up, five repeat blocks and the device clocks around the timed region. `--dump-outputs` writes
    the loss, parameters and gradients of the timed step as float .npy files, 64 MB at most."""
    line = _run_bench(['--no-through-trainer', '--dump-outputs', str(tmp_path)], single=True)
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    import numpy as np
    dumped = {n: np.load(tmp_path/f'{n}.npy') for n in ('loss', 'params', 'grads')}
    assert sorted(p.name for p in tmp_path.iterdir()) == ['grads.npy', 'loss.npy', 'params.npy']
    assert sum(a.nbytes for a in dumped.values()) <= 64 << 20
    assert dumped['loss'].shape == () and dumped['loss'].dtype == np.float64
    assert dumped['params'].shape == dumped['grads'].shape == (4935217,)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in dumped.values())
    assert float(np.abs(dumped['grads']).max()) > 0
    assert line['dump_outputs']['arrays'] == {n: list(a.shape) for n, a in dumped.items()}
    assert line['n_gpus'] == 1 and 'rccl_world_size' not in line
    assert line['warmup'] == 3 and line['warmup_effective']['steps'] > 3
    assert line['warmup_effective']['seconds'] >= line['warmup_effective']['min_seconds_of_steady_steps']
    rep = line['value_repeats']
    assert rep['blocks'] == 5 and len(rep['ms_per_step']) == 5 and rep['min'] <= rep['median'] <= rep['max']
    assert set(line['clock']) >= {'before_timed_region', 'after_timed_region', 'after_repeats'}
    oc = line['other_configs']
    assert [c['dtype'] for c in oc] == ['bf16', 'fp16', 'fp16']
    assert [c['config']['global_batch'] for c in oc] == [16, 1, 8]
    for c in oc:
        assert c['value'] > 0 and c['ms_per_step'] > 0 and c['unit'] == 'utterances/s'
        assert c['roofline']['bound'] == 'mfma' and 0 < c['roofline']['frac'] < 1
        assert 'workload' in c['config'] and 'baseline_config' in c['config']
    assert line['other_configs_wall_s'] < 180
