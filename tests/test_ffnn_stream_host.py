"""Streaming inference of FFNN: what is checked without a GPU (the C ABI of libbrever_ffnn_stream.so -- header,
exports, refusals -- the state layout, the lag and the models ``FFNNStreamer`` does not take)."""
import ctypes

import pytest

from brever_amd import hip, mixture
from brever_amd.models import FFNN, ConvTasNet

EXPORTS = {'brv_ffs_version', 'brv_ffs_last_error', 'brv_ffs_state_bytes', 'brv_ffs_workspace_bytes',
           'brv_ffs_reset', 'brv_ffs_step_frames', 'brv_ffs_step_net', 'brv_ffs_step_emit'}
QUERIES = {'brv_ffs_state_bytes', 'brv_ffs_workspace_bytes'}


def up(x, a):
    return (x + a - 1)//a*a


def layout_bytes(n=512, hop=256, channels=2, mel=64, features=1, stacks=5, cumulative=False):
    """Bytes of one stream slot: [int64 hops received, int64 feature frames made][cumulative
    normaliser only: fp64 sums, then fp64 sums of squares, one per stacked input row][input carry: channels x
    (n - hop)][feature ring: stacks x features mel][overlap-add tail: n - hop], fp32, rounded up to 256."""
    nf = features*mel
    rows = (stacks + 1)*nf
    floats = channels*(n - hop) + stacks*nf + (n - hop)
    return up(16 + (16*rows if cumulative else 0) + 4*floats, 256)


def geometry(model, channels=2):
    from brever_amd.streaming import FFNNStreamer
    return FFNNStreamer._geometry(model, channels)


def test_header_parses_and_every_export_resolves():
    from brever_amd import ffnn_stream as ffs
    with open(ffs.HEADER_PATH) as f:
        table = hip.parse_header(f.read())
    assert set(table) == EXPORTS == set(ffs.SIGNATURES)
    lib = ffs.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        if name in QUERIES:
            assert restype is ctypes.c_int64, name
        elif name not in ('brv_ffs_version', 'brv_ffs_last_error'):
            # the conventions of the main library: int status, a stream as the last argument
            assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr, name
    assert lib.brv_ffs_version() >= 100
    # a library of its own: nothing of it is declared in the other two headers
    assert not any(n.startswith('brv_ffs_') for n in hip.SIGNATURES)
    assert not any(n.startswith('brv_ffs_') for n in mixture.SIGNATURES)
    assert ctypes.sizeof(ffs.FfsConfig) == 160 + 8*(2*(ffs.MAX_HIDDEN + 1) + 4)


REST = {'brv_ffs_step_frames': 7, 'brv_ffs_step_net': 6, 'brv_ffs_step_emit': 7}     # position of `rest`


def _args(name, cfg, fill, numbers=None):
    """Arguments for ``name``: ``cfg`` first, ``fill`` for every other pointer but the stream, and numbers a call
    would ACCEPT (1 everywhere, ``rest`` = -1: a step) unless ``numbers`` says otherwise by position."""
    from brever_amd import ffnn_stream as ffs
    _, argtypes = ffs.SIGNATURES[name]
    last = len(argtypes) - 1 if name not in QUERIES else None
    values = {REST[name]: -1} if name in REST else {}
    values.update(numbers or {})
    return [(cfg if i == 0 else None if i == last else fill) if t is hip._c_ptr else values.get(i, 1)
            for i, t in enumerate(argtypes)]


@pytest.mark.parametrize('name', sorted(EXPORTS - {'brv_ffs_version', 'brv_ffs_last_error'}))
def test_every_export_refuses_null_and_zero_arguments(name):
    from brever_amd import ffnn_stream as ffs
    lib = ffs.lib()
    _, argtypes = ffs.SIGNATURES[name]
    cfg = geometry(FFNN())
    buf = ctypes.create_string_buffer(64)            # never read: each call below is refused on the host
    # a known message from another call first, so that each refusal shows it wrote its own
    assert lib.brv_ffs_workspace_bytes(ctypes.byref(cfg), 0, 0) == -1
    sentinel = lib.brv_ffs_last_error()
    assert sentinel and b'requires' in sentinel
    assert getattr(lib, name)(*_args(name, None, None)) == -1
    null_msg = lib.brv_ffs_last_error()
    assert null_msg and b'null' in null_msg
    for i, t in enumerate(argtypes):
        if t is hip._c_ptr:
            continue
        # the refused value: 0, or for `rest` (where 0 is a tail with nothing left) a whole hop
        bad = cfg.hop if i == REST.get(name) else 0
        assert getattr(lib, name)(*_args(name, ctypes.byref(cfg), buf, {i: bad})) == -1, (name, i)
        msg = lib.brv_ffs_last_error()
        assert msg and msg != null_msg and b'requires' in msg, (name, i, msg)
    if name not in QUERIES:
        with pytest.raises(RuntimeError, match=name):
            ffs.call(name, *_args(name, None, None))


@pytest.mark.parametrize('kw, layout', [
    (dict(), dict()),
    (dict(normalization='cumulative'), dict(cumulative=True)),
    (dict(stft_frame_length=256, stft_hop_length=64, mel_filters=24, stacks=2),
     dict(n=256, hop=64, mel=24, stacks=2)),
    (dict(features={'logfbe', 'cubicpdf'}, stacks=3, normalization='cumulative'),
     dict(features=2, stacks=3, cumulative=True)),
])
def test_state_bytes_follow_the_layout(kw, layout):
    from brever_amd import ffnn_stream as ffs
    cfg = geometry(FFNN(**kw))
    assert ffs.lib().brv_ffs_state_bytes(ctypes.byref(cfg)) == layout_bytes(**layout)
    mono = geometry(FFNN(**kw), channels=1)
    assert ffs.lib().brv_ffs_state_bytes(ctypes.byref(mono)) == layout_bytes(channels=1, **layout)


def test_default_state_is_4608_bytes():
    from brever_amd import ffnn_stream as ffs
    # 16 + 4 (2 x 256 carry + 5 x 64 ring + 256 tail) = 4368, rounded up to 256
    assert ffs.lib().brv_ffs_state_bytes(ctypes.byref(geometry(FFNN()))) == 4608 == layout_bytes()


def test_workspace_grows_with_the_columns():
    from brever_amd import ffnn_stream as ffs
    lib = ffs.lib()
    cfg = ctypes.byref(geometry(FFNN()))
    one = lib.brv_ffs_workspace_bytes(cfg, 1, 1)
    assert 0 < one < lib.brv_ffs_workspace_bytes(cfg, 16, 1)
    assert lib.brv_ffs_workspace_bytes(cfg, 4, 8) > lib.brv_ffs_workspace_bytes(cfg, 4, 4)
    # two activation buffers of (columns, widest layer rounded up to 32) and one feature frame per column
    assert lib.brv_ffs_workspace_bytes(cfg, 16, 1) >= 16*4*(2*1024 + 64)


def test_lag_is_frame_length_minus_hop():
    from brever_amd.streaming import FFNNStreamer
    assert FFNNStreamer.lag_for(FFNN()) == 256
    assert FFNNStreamer.lag_for(FFNN(stft_frame_length=256, stft_hop_length=64)) == 192
    assert FFNNStreamer.lag_for(FFNN(features={'fbe', 'logfbe', 'cubicfbe', 'pdf', 'logpdf', 'cubicpdf'},
                                     normalization='cumulative', decimation=2)) == 256


@pytest.mark.parametrize('make, cause', [
    (lambda: ConvTasNet(causal=True), 'needs an FFNN, got ConvTasNet'),
    (lambda: FFNN(features={'mfcc'}), "DCT feature 'mfcc'"),
    (lambda: FFNN(features={'ic'}), "binaural cue feature 'ic'"),
    (lambda: FFNN(stft_frame_length=512, stft_hop_length=200), 'multiple of 2 hop'),
    (lambda: FFNN(hidden_layers=[8]*9), 'at most 8 hidden layers'),
], ids=['convtasnet', 'mfcc', 'ic', 'hop200', '9layers'])
def test_models_the_streamer_does_not_take(make, cause):
    from brever_amd.streaming import FFNNStreamer
    model = make()
    with pytest.raises(ValueError, match=cause):
        FFNNStreamer.lag_for(model)
    with pytest.raises(ValueError, match=cause):
        FFNNStreamer(model)


def test_the_library_refuses_what_it_cannot_run():
    from brever_amd import ffnn_stream as ffs
    lib = ffs.lib()
    buf = ctypes.create_string_buffer(64)

    def refused(cfg, word):
        assert lib.brv_ffs_state_bytes(ctypes.byref(cfg)) == -2
        assert word in lib.brv_ffs_last_error(), lib.brv_ffs_last_error()
        assert lib.brv_ffs_reset(ctypes.byref(cfg), buf, 1, buf, 1, None) == -2
        assert lib.brv_ffs_step_net(*_args('brv_ffs_step_net', ctypes.byref(cfg), buf, {6: -1})) == -2
        assert word in lib.brv_ffs_last_error(), lib.brv_ffs_last_error()

    refused(geometry(FFNN(stft_frame_length=512, stft_hop_length=200)), b'2 hop')
    refused(geometry(FFNN(hidden_layers=[8]*9)), b'8 hidden layers')
    cfg = geometry(FFNN())
    cfg.n_fft = 1024                                                     # n_fft != frame_length
    refused(cfg, b'STFT')
    cfg = geometry(FFNN())
    cfg.compression = 0.5
    refused(cfg, b'STFT')
    refused(geometry(FFNN(stft_frame_length=8192, stft_hop_length=2048)), b'4096')
    refused(geometry(FFNN(), channels=9), b'channels')
    # a step of more streams than slots, a tail of the wrong frame count
    cfg = geometry(FFNN())
    assert lib.brv_ffs_reset(ctypes.byref(cfg), buf, 1, buf, 2, None) == -1
    assert b'n <= slots' in lib.brv_ffs_last_error()
    assert lib.brv_ffs_step_frames(ctypes.byref(cfg), buf, 1, buf, 1, buf, 3, 5, buf, None) == -1
    assert b'tail' in lib.brv_ffs_last_error()


def test_cpu_model_fails_like_the_rest_of_the_package():
    import torch

    from brever_amd.streaming import FFNNStreamer, enhance_streaming
    with pytest.raises(RuntimeError, match='ROCm device'):
        FFNNStreamer(FFNN(hidden_layers=[16]))
    with pytest.raises(RuntimeError, match='ROCm device'):
        enhance_streaming(FFNN(hidden_layers=[16]), torch.zeros(2, 1000), chunk_samples=256)
