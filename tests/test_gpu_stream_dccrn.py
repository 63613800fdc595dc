"""Streaming inference of DCCRN (brever_amd.streaming.DCCRNStreamer, csrc/dccrn_stream.hip) on the MI355X:
chunk-by-chunk output against the reference goldens and the offline ``enhance``, the lag, lengths at the
edges, stream independence, parameter changes, bf16, errors and the streaming script. Every test here
needs a real MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 128
FP32_BOUND = 1e-5


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()/(b.norm() + 1e-30))


def golden_model(golden_dir, prefix=''):
    from brever_amd.models import DCCRN
    g = np.load(os.path.join(golden_dir, 'dccrn.npz'))
    net = DCCRN(**json.loads(str(g[f'{prefix}config']))).to(_cuda())
    flat = torch.from_numpy(g[f'{prefix}params']).to(_cuda())
    o = 0
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
    # the running statistics of the goldens' eval outputs: the train-mode forward of x, then the train-mode
    # forward of the loss batch (the order the goldens were made in)
    net.train()
    with torch.no_grad():
        net(torch.from_numpy(g['x']).to(_cuda()))
        running = torch.cat([b.reshape(-1).float() for n, b in net.named_buffers() if 'running' in n]).cpu()
        assert torch.allclose(running, torch.from_numpy(g[f'{prefix}running']), rtol=1e-4, atol=1e-6)
        net.loss(torch.from_numpy(g['batch']).to(_cuda()), torch.from_numpy(g['lengths']).to(_cuda()), False)
    net.eval()
    return g, net


def seeded_model(seed=0, **kw):
    """A model whose batch norms are not the identity: perturbed affine values and running statistics."""
    from brever_amd.models import DCCRN
    from brever_amd.models.dccrn import ComplexBatchNorm2d
    torch.manual_seed(seed)
    net = DCCRN(**kw).to(_cuda())
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.weight.copy_(1 + 0.2*torch.randn(C, generator=g))
                m.bias.copy_(0.1*torch.randn(C, generator=g))
                m.running_mean.copy_(0.1*torch.randn(C, generator=g))
                m.running_var.copy_(0.5 + torch.rand(C, generator=g))
            elif isinstance(m, ComplexBatchNorm2d):
                C = m.num_features
                m.bias.copy_(0.1*torch.randn(2, C, generator=g))
                m.running_mean.copy_(0.1*torch.randn(2, C, generator=g))
    net.eval()
    return net


def stream(streamer, x, hop_counts, rest=True):
    """Stream (n, L) through fresh slots in chunks of ``hop_counts`` hops (cycled), flush; returns the output
    with the lag removed, (n, L)."""
    hop = streamer.hop
    n, L = x.shape
    ids = streamer.open(n)
    whole = L//hop*hop
    outs, i, j = [], 0, 0
    while i < whole:
        k = min(hop_counts[j % len(hop_counts)]*hop, whole - i)
        outs.append(streamer.process(x[:, i:i + k], ids))
        i += k
        j += 1
    outs.append(streamer.flush(ids, x[:, whole:] if L > whole and rest else None))
    streamer.close(ids)
    return torch.cat(outs, dim=-1)[..., streamer.lag:]


def chunkings(L, hop):
    rng = np.random.default_rng(7)
    return {'1': [1], '7': [7], 'mix': [int(v) for v in rng.integers(1, 12, size=40)], 'whole': [L//hop]}


def signal(n, L, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (0.3*torch.randn(n, L, generator=g)).to(_cuda())


@pytest.mark.parametrize('prefix', ['', 'cbn_'])
def test_fp32_stream_matches_reference_goldens(golden_dir, prefix):
    from brever_amd.streaming import DCCRNStreamer, enhance_streaming
    g, net = golden_model(golden_dir, prefix)
    x = torch.from_numpy(g['x']).to(_cuda())
    gold = torch.from_numpy(g[f'{prefix}out_eval'])
    s = DCCRNStreamer(net, max_streams=2)
    for name, counts in chunkings(x.shape[-1], s.hop).items():
        err = rel(stream(s, x, counts), gold)
        assert err <= 2e-4, (prefix, name, err)
    if not prefix:
        e = enhance_streaming(net, torch.stack([x, 0.5*x], dim=1), chunk_samples=3*HOP)
        assert e.shape == (2, x.shape[-1])
        assert rel(e, torch.from_numpy(g['enhance'])) <= 2e-4


@pytest.mark.parametrize('cbn', [False, True])
def test_fp32_stream_matches_enhance_default_width(cbn):
    from brever_amd.streaming import DCCRNStreamer
    net = seeded_model(1, use_complex_batchnorm=cbn)
    x = signal(2, 4*16000)
    with torch.no_grad():
        ref = net.enhance(x.unsqueeze(1), use_amp=False)
    s = DCCRNStreamer(net, max_streams=2)
    for name, counts in chunkings(x.shape[-1], s.hop).items():
        if cbn and name in ('7', 'mix'):
            continue
        err = rel(stream(s, x, counts), ref)
        assert err <= FP32_BOUND, (name, err)


def test_fp32_long_stream_stays_exact():
    from brever_amd.streaming import DCCRNStreamer
    net = seeded_model(2)
    x = signal(1, 60*16000, seed=5)
    with torch.no_grad():
        ref = net.enhance(x.unsqueeze(1), use_amp=False)
    s = DCCRNStreamer(net, max_streams=1)
    err = rel(stream(s, x, [2]), ref)             # 16 ms chunks
    assert err <= FP32_BOUND, err


@pytest.mark.parametrize('L', [641, 700, 1280, 1281, 20*HOP, 20*HOP + HOP - 1])
def test_lengths_at_the_edges(L):
    from brever_amd.streaming import DCCRNStreamer, enhance_streaming
    net = seeded_model(3)
    assert net.latency == 1280
    x = signal(2, L, seed=L)
    with torch.no_grad():
        ref = net.enhance(x.unsqueeze(1), use_amp=False)
    got = enhance_streaming(net, x.unsqueeze(1), chunk_samples=2*HOP)
    assert got.shape == ref.shape
    assert rel(got, ref) <= FP32_BOUND, rel(got, ref)
    if L == 641:
        s = DCCRNStreamer(net, max_streams=1)
        ids = s.open(1)
        s.process(x[:1, :5*HOP], ids)
        with pytest.raises(ValueError):
            s.flush(ids)                              # 640 samples: fewer than 7 STFT frames


def test_output_is_final_when_returned():
    from brever_amd.streaming import DCCRNStreamer
    net = seeded_model(4)
    L = 40*HOP + 17
    x = signal(1, L, seed=9)
    with torch.no_grad():
        ref = net.enhance(x.unsqueeze(1), use_amp=False)
    s = DCCRNStreamer(net, max_streams=1)
    assert s.lag == net.latency - HOP == 9*HOP
    ids = s.open(1)
    outs = []
    for j in range(1, 41):
        outs.append(s.process(x[:, (j - 1)*HOP:j*HOP], ids))
        y = torch.cat(outs, dim=-1)[0]
        assert bool((y[:min(j*HOP, s.lag)] == 0).all())
        if j*HOP > s.lag:
            got = y[s.lag:]
            assert rel(got, ref[0, :j*HOP - s.lag]) <= FP32_BOUND, (j, rel(got, ref[0, :j*HOP - s.lag]))
    tail = s.flush(ids, x[:, 40*HOP:])
    assert tail.shape == (1, s.lag + 17)
    full = torch.cat(outs + [tail], dim=-1)[0, s.lag:]
    assert rel(full, ref[0]) <= FP32_BOUND


def test_streams_are_independent_and_slots_reusable(golden_dir):
    from brever_amd.streaming import DCCRNStreamer
    _, net = golden_model(golden_dir)
    s = DCCRNStreamer(net, max_streams=6)
    L = 30*HOP
    x = signal(4, L, seed=11)
    alone = stream(s, x[:1], [3])
    rng = np.random.default_rng(1)
    ids = s.open(4)
    outs = {i: [] for i in range(4)}
    pos = 0
    while pos < L:
        k = 3*HOP
        order = list(rng.permutation(4))
        subset = order[:int(rng.integers(1, 5))]
        if 0 not in subset:
            subset.append(0)
        # every stream advances by the same hops in this round, in calls of shuffled subsets
        rest = [i for i in order if i not in subset]
        for group in (subset, rest):
            if not group:
                continue
            y = s.process(x[group, pos:pos + k], [ids[i] for i in group])
            for row, i in enumerate(group):
                outs[i].append(y[row:row + 1])
        pos += k
    tails = s.flush([ids[i] for i in range(4)])
    together = torch.cat(outs[0] + [tails[:1]], dim=-1)[..., s.lag:]
    assert torch.equal(together, alone)
    # reuse: a slot after close / open and after reset gives the fresh slot's bits
    s.close(ids)
    assert torch.equal(stream(s, x[:1], [3]), alone)
    ids = s.open(2)
    s.process(x[:2, :5*HOP], ids)
    s.reset(ids)
    outs = [s.process(x[:1, i:i + 3*HOP], ids[1:]) for i in range(0, L, 3*HOP)]
    outs.append(s.flush(ids[1:]))
    assert torch.equal(torch.cat(outs, dim=-1)[..., s.lag:], alone)


def test_parameter_changes_reach_new_streams():
    from brever_amd.streaming import DCCRNStreamer
    a, b = seeded_model(5), seeded_model(6)
    x = signal(1, 12*HOP + 5, seed=13)
    s = DCCRNStreamer(a, max_streams=1)
    ya = stream(s, x, [2])
    with torch.no_grad():
        assert rel(ya, a.enhance(x.unsqueeze(1))) <= FP32_BOUND
    a.load_state_dict(b.state_dict())                 # parameters and running buffers
    yb = stream(s, x, [2])
    with torch.no_grad():
        assert rel(yb, b.enhance(x.unsqueeze(1))) <= FP32_BOUND
    a.train()                                         # the streamer uses the running statistics anyway
    assert torch.equal(stream(s, x, [2]), yb)


def test_bf16_stream(golden_dir):
    from brever_amd.streaming import DCCRNStreamer
    g, net = golden_model(golden_dir)
    x = torch.from_numpy(g['x']).to(_cuda())
    err = rel(stream(DCCRNStreamer(net, max_streams=2, use_amp=True), x, [3]), torch.from_numpy(g['out_eval']))
    assert 0 < err <= 5e-3, err
    net = seeded_model(7)
    x = signal(2, 4*16000, seed=17)
    with torch.no_grad():
        ref = net.enhance(x.unsqueeze(1), use_amp=False)
        off16 = rel(net.enhance(x.unsqueeze(1), use_amp=True), ref)
    got = rel(stream(DCCRNStreamer(net, max_streams=2, use_amp=True), x, [4]), ref)
    assert got <= 1.5*off16, (got, off16)


def test_stream_errors(golden_dir):
    from brever_amd.streaming import DCCRNStreamer
    _, net = golden_model(golden_dir)
    s = DCCRNStreamer(net, max_streams=2)
    hop = s.hop
    ids = s.open(1)
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop + 1, device='cuda'), ids)
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop, device='cuda'), [1])          # never opened
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop, device='cuda'), [7])          # out of range
    with pytest.raises(ValueError):
        s.process(torch.zeros(2, hop, device='cuda'), ids + ids)    # duplicated
    with pytest.raises(ValueError):
        s.flush(ids, torch.zeros(1, hop, device='cuda'))            # not a partial hop
    s.close(ids)
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop, device='cuda'), ids)          # closed
    with pytest.raises(RuntimeError):
        s.open(3)
    ids = s.open(1)
    with pytest.raises(RuntimeError):
        s.process(torch.zeros(1, hop), ids)                         # CPU tensor


def test_stream_enhance_script(tmp_path):
    """scripts/stream_enhance.py on a freshly trained tiny DCCRN equals the offline enhancement of the same
    file to 16-bit quantisation."""
    from helpers import run_entry_points

    from brever_amd.config import get_config
    from brever_amd.data import audio_read, write_flac
    from brever_amd.models import ModelRegistry
    model_dir, _, _ = run_entry_points(
        tmp_path, 'dccrn', model_args=['--channels', '4,8,8,16,16,16', '--lstm_channels', '16'],
        trainer_args=['--epochs', '1', '--val_period', '1', '--batch_size', '4', '--val_metrics', 'snr'],
        metrics=('snr',))
    x = 0.2*np.random.default_rng(3).standard_normal(16000 + 77)
    src, dst = str(tmp_path/'in.flac'), str(tmp_path/'out.flac')
    write_flac(src, x, 16000)
    out = subprocess.run([sys.executable, 'scripts/stream_enhance.py', '-i', model_dir, src, dst],
                         capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'real-time factor' in out.stdout
    cfg = get_config(os.path.join(model_dir, 'config.yaml'))
    model = ModelRegistry.get(cfg.arch)(**cfg.model.to_dict()).cuda()
    state = torch.load(os.path.join(model_dir, 'checkpoints', 'last.ckpt'), map_location='cuda', weights_only=False)
    model.load_state_dict(state['model'])
    if 'ema' in state:
        from brever_amd.training import ExponentialMovingAverage
        ema = ExponentialMovingAverage(model.parameters(), decay=cfg.trainer.ema_decay)
        ema.load_state_dict(state['ema'])
        ema.copy_to()
    model.eval()
    with open(src, 'rb') as f:
        xin, fs = audio_read(f, src)
    xin = torch.as_tensor(xin, dtype=torch.float32).cuda()
    with torch.no_grad():
        ref = model.enhance(xin.reshape(1, -1).repeat(2, 1)).cpu().numpy()
    with open(dst, 'rb') as f:
        y, fs2 = audio_read(f, dst)
    assert fs2 == 16000 and y.shape == ref.shape
    assert np.abs(y - ref).max() <= 1.5/32768 + 1e-4*np.abs(ref).max()
