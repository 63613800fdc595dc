"""Streaming inference of the causal Conv-TasNet (brever_amd.streaming, csrc/ctn_stream.hip) on the
MI355X: chunk-by-chunk output against the reference goldens and the offline ``enhance``, stream
independence, parameter changes, bf16. Every test here needs a real MI355X."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEFAULT = dict(causal=True)          # 512 / 32 / 128 / 512 / 128, 8 x 3 blocks, P = 3


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()/(b.norm() + 1e-30))


def golden_model(golden_dir, tag):
    from brever_amd.models import ConvTasNet
    from oracle.convtasnet import OracleConvTasNet
    g = np.load(os.path.join(golden_dir, f'convtasnet_{tag}.npz'))
    cfg = json.loads(str(g['config']))
    oracle = OracleConvTasNet(**cfg)
    off = 0
    with torch.no_grad():
        for p in oracle.parameters():
            p.copy_(torch.from_numpy(g['params'][off:off + p.numel()]).view(p.shape))
            off += p.numel()
    net = ConvTasNet(**cfg)
    net.load_state_dict(oracle.state_dict())
    return g, net.to(_cuda())


def seeded_model(seed=0, **kw):
    from brever_amd.models import ConvTasNet
    torch.manual_seed(seed)
    return ConvTasNet(**kw).to(_cuda())


def stream(streamer, x, hop_counts, rest=True):
    """Stream (n, L) through fresh slots in chunks of ``hop_counts`` hops (cycled), flush; returns
    the output with the one-hop lag removed, (n, S, L)."""
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
    return torch.cat(outs, dim=-1)[..., hop:]


def chunkings(L, hop):
    rng = np.random.default_rng(7)
    return {'1': [1], '7': [7], 'mix': [int(v) for v in rng.integers(1, 12, size=40)], 'whole': [L//hop]}


@pytest.mark.parametrize('tag', ['causal', 'causal2'])
def test_fp32_stream_matches_reference_goldens(golden_dir, tag):
    from brever_amd.streaming import ConvTasNetStreamer
    g, net = golden_model(golden_dir, tag)
    x = torch.from_numpy(g['batch'])[:, 0].cuda()
    want = torch.from_numpy(g['output'])
    s = ConvTasNetStreamer(net, max_streams=4, use_amp=False)
    for name, hops in chunkings(x.shape[1], s.hop).items():
        got = stream(s, x, hops)
        assert got.shape == want.shape
        assert rel(got, want) <= 1e-5, name


@pytest.mark.parametrize('chunk', [16, 256])
def test_fp32_stream_matches_enhance_default_width(chunk):
    from brever_amd.streaming import enhance_streaming
    net = seeded_model(**DEFAULT)
    g = torch.Generator().manual_seed(3)
    x = (0.3*torch.randn(3, 1, 24000, generator=g)).cuda()
    want = net.enhance(x, use_amp=False)
    got = enhance_streaming(net, x, chunk_samples=chunk, use_amp=False)
    assert got.shape == want.shape
    assert rel(got, want) <= 1e-5


def test_fp32_long_stream_stays_exact():
    """60 s in 16 ms chunks: the carried fp64 statistics do not drift."""
    from brever_amd.streaming import enhance_streaming
    net = seeded_model(1, filters=128, bottleneck_channels=64, hidden_channels=128, skip_channels=64,
                       layers=8, repeats=1, causal=True)
    g = torch.Generator().manual_seed(4)
    fs = 16000
    x = (0.3*torch.randn(1, 1, 60*fs, generator=g)).cuda()
    want = net.enhance(x, use_amp=False)
    got = enhance_streaming(net, x, chunk_samples=256, use_amp=False)
    assert rel(got, want) <= 1e-5
    assert rel(got[..., -10*fs:], want[..., -10*fs:]) <= 1e-5


def test_streams_are_independent_and_slots_reusable(golden_dir):
    """Bitwise: a stream's output does not depend on the other streams of a call, on their order,
    or on what its slot held before."""
    from brever_amd.streaming import ConvTasNetStreamer
    _, net = golden_model(golden_dir, 'causal')
    hop = net.cfg.filter_length//2
    g = torch.Generator().manual_seed(5)
    sig = {k: (0.3*torch.randn(1, 20*hop, generator=g)).cuda() for k in 'ABCD'}
    F = 3

    def chunk(k, i):
        return sig[k][:, i*F*hop:(i + 1)*F*hop]

    # calls: lists of streams; every stream gets its chunks in order
    plan = [['A'], ['B', 'A'], ['A', 'C', 'B'], ['C'], ['B', 'C', 'A'], ['C', 'A', 'B']]
    s = ConvTasNetStreamer(net, max_streams=6)
    s.open(1)                                       # slot 0 idle all along
    slot = dict(zip('ABC', s.open(3)))
    got = {k: [] for k in 'ABC'}
    pos = {k: 0 for k in 'ABC'}
    for call in plan:
        ids = [slot[k] for k in call]
        x = torch.cat([chunk(k, pos[k]) for k in call])
        y = s.process(x, ids)
        for r, k in enumerate(call):
            got[k].append(y[r:r + 1])
            pos[k] += 1
    for k in 'ABC':
        alone = ConvTasNetStreamer(net, max_streams=1)
        i = alone.open(1)
        want = [alone.process(chunk(k, c), i) for c in range(pos[k])]
        assert torch.equal(torch.cat(got[k], -1), torch.cat(want, -1)), k
    # reuse: a closed-and-reopened slot and a reset slot behave like fresh ones
    s.close([slot['A']])
    (d,) = s.open(1)
    assert d == slot['A']
    s.reset([slot['B']])
    both = s.process(torch.cat([chunk('D', 0), chunk('D', 0)]), [d, slot['B']])
    fresh = ConvTasNetStreamer(net, max_streams=1)
    want = fresh.process(chunk('D', 0), fresh.open(1))
    assert torch.equal(both[0:1], want) and torch.equal(both[1:2], want)


def test_parameter_changes_reach_new_streams():
    from brever_amd.streaming import ConvTasNetStreamer, enhance_streaming
    cfg = dict(filters=64, filter_length=16, bottleneck_channels=32, hidden_channels=64, skip_channels=32,
               layers=4, repeats=2, causal=True)
    net = seeded_model(2, **cfg)
    g = torch.Generator().manual_seed(6)
    x = (0.3*torch.randn(2, 1, 4000, generator=g)).cuda()
    s = ConvTasNetStreamer(net, max_streams=2)
    before = stream(s, x[:, 0], [5])
    assert rel(before, net.enhance(x)) <= 1e-5
    # one FlatAdam step (fused train step: forward, SNR loss, backward, clip + Adam)
    batch = (0.3*torch.randn(2, 2, 4000, generator=g)).cuda()
    net.train_step(batch, torch.tensor([4000, 3000]).cuda(), False, None)
    after = stream(s, x[:, 0], [5])
    want = net.enhance(x)
    assert rel(after, want) <= 1e-5
    assert rel(before, want) > 1e-4
    # load_state_dict of another model
    other = seeded_model(9, **cfg)
    net.load_state_dict(other.state_dict())
    assert rel(stream(s, x[:, 0], [5]), other.enhance(x)) <= 1e-5
    assert rel(enhance_streaming(net, x, 80), other.enhance(x)) <= 1e-5


@pytest.mark.parametrize('tag', ['causal', 'causal2'])
def test_bf16_stream(golden_dir, tag):
    from brever_amd.streaming import ConvTasNetStreamer
    g, net = golden_model(golden_dir, tag)
    x = torch.from_numpy(g['batch'])[:, 0].cuda()
    s = ConvTasNetStreamer(net, max_streams=4, use_amp=True)
    offline = net.enhance(x.unsqueeze(1), use_amp=True)
    for name, hops in chunkings(x.shape[1], s.hop).items():
        got = stream(s, x, hops)
        assert rel(got, offline) <= 5e-3, name
        assert rel(got, torch.from_numpy(g['output'])) <= 2e-2, name


def test_bf16_stream_default_width():
    """At the default widths the streamed bf16 output is as close to fp32 as the offline bf16 path is
    (the two bf16 paths round at different points, so they are compared through the fp32 result)."""
    from brever_amd.streaming import enhance_streaming
    net = seeded_model(**DEFAULT)
    g = torch.Generator().manual_seed(8)
    x = (0.3*torch.randn(2, 1, 8000, generator=g)).cuda()
    want = net.enhance(x, use_amp=True)
    fp32 = net.enhance(x, use_amp=False)
    got = enhance_streaming(net, x, chunk_samples=256, use_amp=True)
    assert rel(got, want) <= 1e-2
    assert rel(got, fp32) <= 1.5*rel(want, fp32)


def test_stream_errors(golden_dir):
    from brever_amd.streaming import ConvTasNetStreamer
    _, net = golden_model(golden_dir, 'causal')
    s = ConvTasNetStreamer(net, max_streams=2)
    hop = s.hop
    ids = s.open(1)
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop + 1, device='cuda'), ids)
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop, device='cuda'), [1])          # never opened
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop, device='cuda'), [7])          # out of range
    with pytest.raises(ValueError):
        s.flush(ids, torch.zeros(1, hop, device='cuda'))            # not a partial hop
    s.close(ids)
    with pytest.raises(ValueError):
        s.process(torch.zeros(1, hop, device='cuda'), ids)          # closed
    with pytest.raises(RuntimeError):
        s.open(3)
    with pytest.raises(RuntimeError):
        s.open(1)
        s.process(torch.zeros(1, hop), [0])                         # CPU tensor
