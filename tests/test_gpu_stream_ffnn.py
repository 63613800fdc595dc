"""Streaming inference of FFNN (brever_amd.streaming.FFNNStreamer, csrc/ffnn_stream/) on the MI355X:
chunk-by-chunk output against the reference golden and the offline ``enhance``, the lag, the envelope at both
ends, the stack history, the cumulative normaliser and the feature kinds, stream independence, slots, parameter
changes, the default widths, errors and the streaming script. Every test here needs a real MI355X.

Measured on the MI355X (rel-L2): the golden model 1.8e-7 against the reference's output and
9.8e-8 against offline ``enhance`` in all four chunkings; 256 / 64 at the five lengths 4.8e-8 .. 7.9e-8; the
first six hops with five stacks 8.9e-8; cumulative normaliser 6.0e-8; logfbe + cubicpdf 1.7e-7; default widths
9.4e-8."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_BOUND = 2e-4          # test_ffnn_matches_reference: the offline path against the same golden
FP32_BOUND = 1e-5            # streamed against offline enhance (the bound of the DCCRN streaming test)


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()/(b.norm() + 1e-30))


@pytest.fixture(scope='module')
def golden(golden_dir):
    """(arrays, model at the golden's weights and statistics, its input on the device, offline enhance of it)."""
    from brever_amd.models import FFNN
    g = np.load(os.path.join(golden_dir, 'ffnn.npz'))
    dev = _cuda()
    net = FFNN(hidden_layers=[96, 80], dropout=0.0).to(dev)
    flat = torch.from_numpy(g['params']).to(dev)
    o = 0
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        net.normalization.set_statistics(torch.from_numpy(g['mean']).to(dev), torch.from_numpy(g['std']).to(dev))
    net.eval()
    x = torch.from_numpy(g['enhance_in']).to(dev)
    with torch.no_grad():
        offline = net.enhance(x)
    return g, net, x, offline


def seeded_model(seed=0, statistics=True, **kw):
    """A seeded FFNN in eval mode; a static normaliser gets statistics that are not the identity."""
    from brever_amd.models import FFNN
    torch.manual_seed(seed)
    net = FFNN(**kw).to(_cuda())
    if statistics and kw.get('normalization', 'static') == 'static':
        g = torch.Generator().manual_seed(100 + seed)
        R = net.ffnn.input_size
        net.normalization.set_statistics((-8 + 2*torch.randn(R, 1, generator=g)).to(_cuda()),
                                         (1.5 + torch.rand(R, 1, generator=g)).to(_cuda()))
    net.eval()
    return net


def signal(n, L, seed=1, channels=2):
    g = torch.Generator().manual_seed(seed)
    level = torch.logspace(0, -1, n).view(n, 1, 1)
    return (0.3*level*torch.randn(n, channels, L, generator=g)).to(_cuda())


def stream(streamer, x, hop_counts):
    """Stream (n, channels, L) through fresh slots in chunks of ``hop_counts`` hops (cycled), flush; returns
    the whole output, lag included: (n, lag + L)."""
    hop = streamer.hop
    n, L = x.shape[0], x.shape[-1]
    ids = streamer.open(n)
    whole = L//hop*hop
    outs, i, j = [], 0, 0
    while i < whole:
        k = min(hop_counts[j % len(hop_counts)]*hop, whole - i)
        outs.append(streamer.process(x[..., i:i + k], ids))
        i += k
        j += 1
    outs.append(streamer.flush(ids, x[..., whole:] if L > whole else None))
    streamer.close(ids)
    return torch.cat(outs, dim=-1)


def chunkings(L, hop):
    rng = np.random.default_rng(7)
    return {'1': [1], '7': [7], 'mix': [int(v) for v in rng.integers(1, 12, size=40)], 'whole': [L//hop]}


def offline(net, x):
    with torch.no_grad():
        return net.enhance(x)


@pytest.mark.parametrize('name', ['1', '7', 'mix', 'whole'])
def test_stream_matches_reference_golden_and_offline(golden, name):
    from brever_amd.streaming import FFNNStreamer
    g, net, x, off = golden
    assert x.shape == (2, 2, 8000)                    # 31 whole hops and 64 rest samples
    s = FFNNStreamer(net, max_streams=2)
    assert (s.hop, s.lag) == (256, 256)
    y = stream(s, x, chunkings(x.shape[-1], s.hop)[name])
    # the lag: exact zeros first, every sample owed afterwards
    assert y.shape == (2, 8000 + s.lag)
    assert bool((y[:, :s.lag] == 0).all())
    e_gold, e_off = rel(y[:, s.lag:], torch.from_numpy(g['enhance_out'])), rel(y[:, s.lag:], off)
    print(f'ffnn stream golden chunking {name}: vs reference {e_gold:.3e}, vs offline {e_off:.3e}')
    assert e_gold <= GOLDEN_BOUND, (name, e_gold)
    assert e_off <= FP32_BOUND, (name, e_off)


def test_enhance_streaming_picks_the_ffnn_streamer(golden):
    from brever_amd.streaming import enhance_streaming
    g, net, x, off = golden
    e = enhance_streaming(net, x, chunk_samples=3*256)
    assert e.shape == off.shape == (2, 8000)
    assert rel(e, torch.from_numpy(g['enhance_out'])) <= GOLDEN_BOUND
    e1 = enhance_streaming(net, x[0], chunk_samples=256)           # unbatched, as enhance takes it
    assert e1.shape == (8000,) and rel(e1, off[0]) <= FP32_BOUND


@pytest.mark.parametrize('L', [256 + 64*9, 256 + 64*9 - 1, 256 + 64*9 + 1, 100, 64*12])
def test_lag_of_three_hops_and_the_envelope_at_both_ends(L):
    """frame 256 / hop 64: lag 192 = 3 hops, one frame of a stream's first call does not exist offline, and the
    frames behind the last offline one are left out of the envelope at the end."""
    from brever_amd.streaming import FFNNStreamer
    net = seeded_model(1, stft_frame_length=256, stft_hop_length=64, mel_filters=24, stacks=2, hidden_layers=[40],
                       dropout=0.0)
    x = signal(3, L, seed=L)
    ref = offline(net, x)
    s = FFNNStreamer(net, max_streams=3)
    assert (s.hop, s.lag) == (64, 192)
    for counts in ([1], [5]):
        y = stream(s, x, counts)
        assert y.shape == (3, L + 192) and bool((y[:, :192] == 0).all())
        err = rel(y[:, 192:], ref)
        print(f'ffnn stream 256/64 L={L} chunks of {counts[0]}: vs offline {err:.3e}')
        assert err <= FP32_BOUND, (L, counts, err)


def test_stack_history_starts_as_copies_of_the_first_frame():
    from brever_amd.streaming import FFNNStreamer
    net = seeded_model(2, stacks=5, hidden_layers=[48], dropout=0.0)
    x = signal(1, 12*256, seed=3)
    ref = offline(net, x)
    s = FFNNStreamer(net, max_streams=1)
    y = stream(s, x, [1])[:, s.lag:]
    err = rel(y[:, :6*256], ref[:, :6*256])
    print(f'ffnn stream first six hops, stacks 5: vs offline {err:.3e}')
    assert err <= FP32_BOUND, err


@pytest.mark.parametrize('kw', [dict(normalization='cumulative', hidden_layers=[32]),
                                dict(features={'logfbe', 'cubicpdf'}, hidden_layers=[32])],
                         ids=['cumulative', 'logfbe+cubicpdf'])
def test_cumulative_normaliser_and_feature_kinds(kw):
    from brever_amd.streaming import FFNNStreamer
    net = seeded_model(3, dropout=0.0, **kw)
    x = signal(2, 40*256, seed=5)
    ref = offline(net, x)
    s = FFNNStreamer(net, max_streams=2)
    err = rel(stream(s, x, [1])[:, s.lag:], ref)
    print(f"ffnn stream {kw.get('normalization') or sorted(kw['features'])}: vs offline {err:.3e}")
    assert err <= FP32_BOUND, err


def test_streams_are_independent():
    from brever_amd.streaming import FFNNStreamer
    net = seeded_model(4, hidden_layers=[96, 80], dropout=0.0)
    L = 12*256
    x = signal(3, L, seed=11)
    s = FFNNStreamer(net, max_streams=5)
    alone = stream(s, x[:1], [2])
    ids = s.open(3)
    outs = []
    orders = [[0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 2], [1, 0, 2], [2, 1, 0]]
    for c, order in enumerate(orders):
        sl = slice(c*512, (c + 1)*512)
        y = s.process(x[order, :, sl], [ids[i] for i in order])
        outs.append(y[order.index(0)][None])
        if len(order) == 2:                            # stream 1 catches up in a call of its own
            s.process(x[1:2, :, sl], [ids[1]])
    outs.append(s.flush([ids[2], ids[0]])[1:2])
    assert torch.equal(torch.cat(outs, dim=-1), alone)


def test_reset_and_reopened_slots_start_fresh():
    from brever_amd.streaming import FFNNStreamer
    net = seeded_model(5, normalization='cumulative', hidden_layers=[32], dropout=0.0)
    x = signal(2, 9*256 + 17, seed=13)
    s = FFNNStreamer(net, max_streams=2)
    fresh = stream(s, x[:1], [2])
    ids = s.open(2)
    s.process(x[:, :, :5*256], ids)
    s.reset(ids[1:])
    outs = [s.process(x[:1, :, i:i + 512], ids[1:]) for i in range(0, 8*256, 512)]
    outs.append(s.process(x[:1, :, 8*256:9*256], ids[1:]))
    outs.append(s.flush(ids[1:], x[:1, :, 9*256:]))
    assert torch.equal(torch.cat(outs, dim=-1), fresh)
    s.close(ids)                                       # both slots hold old state: a reopened one carries nothing
    assert torch.equal(stream(s, x[:1], [2]), fresh)


def test_parameter_changes_take_effect_at_the_next_call():
    from brever_amd.streaming import FFNNStreamer
    net = seeded_model(6, hidden_layers=[64], dropout=0.5)
    net.train()                                        # dropout is never applied, whatever the mode says
    x = signal(1, 6*256 + 9, seed=17)
    s = FFNNStreamer(net, max_streams=2)
    a, b = s.open(2)
    xx = x.repeat(2, 1, 1)
    y0 = s.process(xx[:, :, :512], [a, b])
    assert torch.equal(y0[0], y0[1])
    last = [m for m in net.ffnn.module_list if isinstance(m, torch.nn.Linear)][-1]
    y1 = s.process(xx[:1, :, 512:1024], [a])
    with torch.no_grad():
        last.bias.mul_(3.0).add_(0.5)
    y1b = s.process(xx[1:, :, 512:1024], [b])
    assert not torch.equal(y1, y1b)
    y2 = s.process(xx[:1, :, 1024:1536], [a])
    with torch.no_grad():
        net.normalization.set_statistics(net.normalization.mean + 1.0, 2.0*net.normalization.std)
    y2b = s.process(xx[:1, :, 1024:1536].clone(), [b])
    assert not torch.equal(y2, y2b)
    s.close([a, b])
    net.eval()
    got = stream(s, x, [2])[:, s.lag:]
    assert rel(got, offline(net, x)) <= FP32_BOUND
    net.train()
    assert torch.equal(stream(s, x, [2])[:, s.lag:], got)


def test_default_widths():
    from brever_amd.streaming import FFNNStreamer
    net = seeded_model(7)                              # 384 -> 1024 -> 1024 -> 64
    x = signal(2, 3*256 + 100, seed=19)
    s = FFNNStreamer(net, max_streams=2)
    err = rel(stream(s, x, [3])[:, s.lag:], offline(net, x))
    print(f'ffnn stream default widths: vs offline {err:.3e}')
    assert err <= FP32_BOUND, err


def test_stream_errors(golden):
    from brever_amd.streaming import FFNNStreamer
    _, net, _, _ = golden
    s = FFNNStreamer(net, max_streams=2)
    hop = s.hop
    ids = s.open(1)
    z = lambda *shape: torch.zeros(*shape, device='cuda')            # noqa: E731
    with pytest.raises(ValueError, match='FFNN needs its channels'):
        s.process(z(1, hop), ids)
    with pytest.raises(ValueError, match='channels'):
        s.process(z(1, 1, hop), ids)                                 # one channel where the streamer keeps two
    with pytest.raises(ValueError, match='multiple of hop'):
        s.process(z(1, 2, hop + 1), ids)
    with pytest.raises(ValueError, match='not open'):
        s.process(z(1, 2, hop), [1])                                 # never opened
    with pytest.raises(ValueError, match='distinct'):
        s.process(z(2, 2, hop), ids + ids)
    with pytest.raises(ValueError, match='shorter than hop'):
        s.flush(ids, z(1, 2, hop))
    s.process(z(1, 2, hop), ids)
    s.flush(ids, z(1, 2, 5))
    with pytest.raises(ValueError, match='flushed'):
        s.process(z(1, 2, hop), ids)
    s.reset(ids)
    assert s.process(z(1, 2, hop), ids).shape == (1, hop)
    s.close(ids)
    with pytest.raises(ValueError, match='not open'):
        s.process(z(1, 2, hop), ids)                                 # closed
    with pytest.raises(RuntimeError):
        s.open(3)


def test_stream_enhance_script(tmp_path):
    """scripts/stream_enhance.py on a freshly initialised ffnn model directory and a 0.5 s stereo file."""
    import yaml

    from brever_amd.data import audio_read
    from brever_amd.models import FFNN
    model_dir = tmp_path/'model'
    (model_dir/'checkpoints').mkdir(parents=True)
    kw = dict(hidden_layers=[32, 32], mel_filters=32)
    with open(model_dir/'config.yaml', 'w') as f:
        yaml.safe_dump(dict(arch='ffnn', model=kw), f)
    torch.manual_seed(0)
    torch.save({'model': FFNN(**kw).state_dict()}, model_dir/'checkpoints'/'last.ckpt')
    x = 0.2*np.random.default_rng(3).standard_normal((8000, 2))
    src, dst = str(tmp_path/'in.wav'), str(tmp_path/'out.flac')
    with wave.open(src, 'wb') as w:                    # (the native FLAC encoder writes mono files only)
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(np.rint(x*32768), -32768, 32767).astype('<i2').tobytes())
    out = subprocess.run([sys.executable, 'scripts/stream_enhance.py', '-i', str(model_dir), src, dst],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'real-time factor' in out.stdout
    with open(dst, 'rb') as f:
        y, fs = audio_read(f, dst)
    assert fs == 16000 and y.shape == (8000,)
