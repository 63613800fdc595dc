"""Streaming inference of the causal Conv-TasNet: what is checked without a GPU (argument errors,
state layout, C ABI)."""
import ctypes

import pytest
import torch

from brever_amd import hip
from brever_amd.models import ConvTasNet

GOLDEN_CFG = dict(filters=48, filter_length=16, bottleneck_channels=24, hidden_channels=40,
                  skip_channels=16, kernel_size=3, layers=3, repeats=2, causal=True)


def up(x, a):
    return (x + a - 1)//a*a


def layout_bytes(N=512, L=32, B=128, H=512, Sc=128, P=3, X=8, R=3, S=1, **_):
    """Bytes of one stream slot: [hop count][fp64 (sum, sum of squares) per cumulative norm][last hop of
    input][overlap-add tail per source][per block: ring of (P - 1) 2^(i mod X) frames x H channels]."""
    hop = L//2
    norms = 1 + 2*X*R
    ring_frames = sum((P - 1)*2**(i % X) for i in range(X*R))
    nbytes = 16 + 16*norms + up(4*hop, 16) + up(4*S*hop, 16) + 4*H*ring_frames
    return up(nbytes, 256)


@pytest.mark.parametrize('kw, layout', [
    (dict(causal=True), dict()),
    (GOLDEN_CFG, dict(N=48, L=16, B=24, H=40, Sc=16, P=3, X=3, R=2)),
    (dict(GOLDEN_CFG, kernel_size=2, output_sources=2), dict(N=48, L=16, B=24, H=40, Sc=16, P=2, X=3, R=2, S=2)),
    (dict(GOLDEN_CFG, kernel_size=1), dict(N=48, L=16, B=24, H=40, Sc=16, P=1, X=3, R=2)),
])
def test_state_bytes_follow_the_layout(kw, layout):
    net = ConvTasNet(**kw)
    assert hip.lib().brv_ctn_stream_state_bytes(ctypes.byref(net.cfg)) == layout_bytes(**layout)


def test_default_state_is_the_ring_of_1530_frames():
    net = ConvTasNet(causal=True)
    nbytes = hip.lib().brv_ctn_stream_state_bytes(ctypes.byref(net.cfg))
    assert 1530*512*4 <= nbytes < 1530*512*4 + 4096          # ~3.1 MB per stream


def test_non_causal_and_unsupported_configs_are_refused():
    from brever_amd.streaming import ConvTasNetStreamer, enhance_streaming
    lib = hip.lib()
    net = ConvTasNet(**dict(GOLDEN_CFG, causal=False))
    assert lib.brv_ctn_stream_state_bytes(ctypes.byref(net.cfg)) < 0
    assert lib.brv_ctn_stream_workspace_bytes(ctypes.byref(net.cfg), 1, 1, 0) < 0
    assert lib.brv_ctn_stream_step(ctypes.byref(net.cfg), None, None, None, 1, None, 1, None, 0, None, 0,
                                   None, None) < 0
    with pytest.raises(ValueError):
        ConvTasNetStreamer(net)
    with pytest.raises(ValueError):
        enhance_streaming(net, torch.zeros(1, 2, 160), chunk_samples=16)
    with pytest.raises(ValueError):
        ConvTasNetStreamer(ConvTasNet(**dict(GOLDEN_CFG, filter_length=15)))
    causal = ConvTasNet(**GOLDEN_CFG)
    with pytest.raises(ValueError):
        ConvTasNetStreamer(causal, max_streams=0)


def test_cpu_model_fails_like_the_rest_of_the_package():
    from brever_amd.streaming import ConvTasNetStreamer
    with pytest.raises(RuntimeError, match='ROCm device'):
        ConvTasNetStreamer(ConvTasNet(**GOLDEN_CFG))


def test_workspace_grows_with_the_columns():
    lib = hip.lib()
    cfg = ctypes.byref(ConvTasNet(causal=True).cfg)
    one = lib.brv_ctn_stream_workspace_bytes(cfg, 1, 1, 0)
    assert 0 < one < lib.brv_ctn_stream_workspace_bytes(cfg, 16, 1, 0)
    assert lib.brv_ctn_stream_workspace_bytes(cfg, 16, 1, 1) == lib.brv_ctn_stream_workspace_bytes(cfg, 1, 16, 1)
    assert lib.brv_ctn_stream_workspace_bytes(cfg, 0, 1, 0) < 0


def test_stream_symbols_are_declared_and_bound():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'brever_hip.h')).read()
    names = {'brv_ctn_stream_state_bytes', 'brv_ctn_stream_workspace_bytes', 'brv_ctn_stream_reset',
             'brv_ctn_stream_step', 'brv_ctn_stream_tail'}
    assert names <= set(re.findall(r'\b(brv_[a-z0-9_]+)\s*\(', header))
    assert names <= set(hip.SIGNATURES)
    for name in names:
        assert getattr(hip.lib(), name) is not None
