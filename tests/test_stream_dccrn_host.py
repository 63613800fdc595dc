"""Streaming inference of DCCRN: what is checked without a GPU (state layout, argument errors, C ABI, the lag,
and the look-ahead claim on the CPU oracle)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from brever_amd import hip
from brever_amd.models import DCCRN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CFG = dict(channels=[4, 8, 8, 16, 16, 16], lstm_channels=24, lstm_layers=2)


def up(x, a):
    return (x + a - 1)//a*a


def layout_bytes(n=512, hop=128, channels=(16, 32, 64, 128, 128, 128), kf=5, kt=2, sf=2, pf=2, H=128, layers=2):
    """Bytes of one stream slot: [int64 hops, int64 reserved][input history n - hop][overlap-add
    tail n - hop][LSTM (h, c) of layers x 4 chains x H][rings: spectrum D frames x 2 n/2; encoder level e
    (L + 1 - e) G frames x 2 C_e F_e; recurrent output G x 2 C_L F_L; decoder k < L G x 2 C_(L-k) F_(L-k)]."""
    L, G = len(channels), kt - 1
    D = L*G
    C = [1] + list(channels)
    F = [n//2]
    for _ in channels:
        F.append((F[-1] + 2*pf - kf)//sf + 1)
    floats = 2*(n - hop) + layers*4*2*H + max(D, G)*2*F[0]
    floats += sum((L + 1 - e)*G*2*C[e]*F[e] for e in range(1, L + 1))
    floats += G*2*C[L]*F[L]
    floats += sum(G*2*C[L - k]*F[L - k] for k in range(1, L))
    return up(16 + 4*floats, 256)


def geometry(model):
    from brever_amd.streaming import DCCRNStreamer
    return DCCRNStreamer._geometry(model)


@pytest.mark.parametrize('kw, layout', [
    (dict(), dict()),
    (GOLDEN_CFG, dict(channels=GOLDEN_CFG['channels'], H=24)),
    (dict(GOLDEN_CFG, stft_frame_length=256, stft_hop_length=64, lstm_layers=1),
     dict(n=256, hop=64, channels=GOLDEN_CFG['channels'], H=24, layers=1)),
    (dict(GOLDEN_CFG, kernel_size=(5, 3)), dict(channels=GOLDEN_CFG['channels'], H=24, kt=3)),
])
def test_state_bytes_follow_the_layout(kw, layout):
    cfg = geometry(DCCRN(**kw))
    assert hip.lib().brv_dccrn_stream_state_bytes(ctypes.byref(cfg)) == layout_bytes(**layout)


def test_default_state_is_about_0_42_mb():
    nbytes = hip.lib().brv_dccrn_stream_state_bytes(ctypes.byref(geometry(DCCRN())))
    assert nbytes == up(16 + 4*104192, 256)          # 416 768 bytes + header


def test_workspace_grows_with_the_columns():
    lib = hip.lib()
    cfg = ctypes.byref(geometry(DCCRN()))
    one = lib.brv_dccrn_stream_workspace_bytes(cfg, 1, 1, 0)
    assert 0 < one < lib.brv_dccrn_stream_workspace_bytes(cfg, 16, 1, 0)
    assert lib.brv_dccrn_stream_workspace_bytes(cfg, 16, 1, 1) == lib.brv_dccrn_stream_workspace_bytes(cfg, 1, 16, 1)
    assert lib.brv_dccrn_stream_workspace_bytes(cfg, 4, 8, 0) > lib.brv_dccrn_stream_workspace_bytes(cfg, 4, 4, 0)
    assert lib.brv_dccrn_stream_workspace_bytes(cfg, 0, 1, 0) < 0


def _bad_models():
    yield DCCRN(**dict(GOLDEN_CFG, stride=(2, 2)))                       # time stride 2
    yield DCCRN(**dict(GOLDEN_CFG, padding=(2, 1)))                      # time padding
    yield DCCRN(**dict(GOLDEN_CFG, output_padding=(1, 1)))               # time output padding
    yield DCCRN(**dict(GOLDEN_CFG, stft_frame_length=512, stft_hop_length=192))   # 512 % 384 != 0
    m = DCCRN(**GOLDEN_CFG)
    m.stft.n_fft = 1024                                                  # n_fft != frame_length
    yield m
    m = DCCRN(**GOLDEN_CFG)
    m.mask_net.encoder[2].norm = torch.nn.BatchNorm2d(16, track_running_stats=False)
    yield m
    yield DCCRN(**dict(GOLDEN_CFG, channels=[4, 8, 8, 16, 16, 2048]))   # channels beyond 1024
    yield DCCRN(**dict(GOLDEN_CFG, lstm_channels=1024))                 # LSTM beyond 512
    yield DCCRN(stft_frame_length=8192, stft_hop_length=2048, **GOLDEN_CFG)   # n_fft beyond 4096
    yield DCCRN(**dict(GOLDEN_CFG, channels=[4]*9))                      # 9 levels


def test_unsupported_configurations_are_refused():
    from brever_amd.models import ConvTasNet
    from brever_amd.streaming import DCCRNStreamer
    for m in _bad_models():
        with pytest.raises(ValueError):
            DCCRNStreamer(m)
    with pytest.raises(ValueError):
        DCCRNStreamer(ConvTasNet(causal=True))
    with pytest.raises(ValueError):
        DCCRNStreamer(DCCRN(**GOLDEN_CFG), max_streams=0)
    lib = hip.lib()
    cfg = geometry(DCCRN(**dict(GOLDEN_CFG, stride=(2, 2))))
    assert lib.brv_dccrn_stream_state_bytes(ctypes.byref(cfg)) < 0
    assert lib.brv_dccrn_stream_step(ctypes.byref(cfg), *[None]*6, 1, None, 1, None, 0, None, 0, None, None) < 0
    assert lib.brv_dccrn_stream_tail(ctypes.byref(cfg), *[None]*6, 1, None, 0, None, 0, None, 0, None, None) < 0


def test_cpu_model_fails_like_the_rest_of_the_package():
    from brever_amd.streaming import DCCRNStreamer, enhance_streaming
    with pytest.raises(RuntimeError, match='ROCm device'):
        DCCRNStreamer(DCCRN(**GOLDEN_CFG))
    with pytest.raises(RuntimeError, match='ROCm device'):
        enhance_streaming(DCCRN(**GOLDEN_CFG), torch.zeros(2, 1000), chunk_samples=128)


@pytest.mark.parametrize('kw', [dict(), GOLDEN_CFG, dict(GOLDEN_CFG, kernel_size=(5, 3))])
def test_lag_is_latency_minus_hop(kw):
    from brever_amd.streaming import DCCRNStreamer
    m = DCCRN(**kw)
    assert DCCRNStreamer.lag_for(m) == m.latency - m.stft.hop_length
    if kw == {}:
        assert DCCRNStreamer.lag_for(m) == 1152
    if torch.cuda.is_available():
        assert DCCRNStreamer(m.cuda(), max_streams=1).lag == m.latency - m.stft.hop_length


def test_stream_symbols_are_declared_and_bound():
    import re
    header = open(os.path.join(ROOT, 'include', 'brever_hip.h')).read()
    names = {'brv_dccrn_stream_state_bytes', 'brv_dccrn_stream_workspace_bytes', 'brv_dccrn_stream_reset',
             'brv_dccrn_stream_step', 'brv_dccrn_stream_tail'}
    assert names <= set(re.findall(r'\b(brv_[a-z0-9_]+)\s*\(', header))
    assert names <= set(hip.SIGNATURES)
    for name in names:
        assert getattr(hip.lib(), name) is not None
    assert 'dccrn_stream.hip' in open(os.path.join(ROOT, 'brever_amd', 'csrc', 'Makefile')).read()


def test_look_ahead_is_the_lag():
    """On the CPU oracle (narrow widths, eval mode, non-trivial running statistics): output hop m depends on
    input hop m + 9 and on nothing from hop m + 10 onwards -- lag = 9 hops is the least possible."""
    from oracle.dccrn import OracleDCCRN
    torch.manual_seed(3)
    net = OracleDCCRN(**json.loads(json.dumps(GOLDEN_CFG))).double()
    for mod in net.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.2, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
    net.eval()
    hop, L = 128, 3000
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, L, generator=g, dtype=torch.float64)
    with torch.no_grad():
        base = net(x)
        for h in (10, 14):
            x2 = x.clone()
            x2[:, h*hop:] += torch.randn(1, L - h*hop, generator=g, dtype=torch.float64)
            diff = (net(x2) - base).abs()[0]
            per_hop = np.array([float(diff[k*hop:(k + 1)*hop].max()) for k in range(L//hop)])
            changed = np.nonzero(per_hop > 1e-12)[0]
            assert changed[0] == h - 9, (h, changed[:3])
