"""The host side of the GPU FLAC decoder (include/brever_flac.h, brever_amd/flac_gpu.py): the frame index against
the test encoder's own frame boundaries, its rejections, the binding, the stand-alone check of the decode core under
the sanitizers, and the opt-in switch of the dataset. No test here needs a device."""
import ctypes
import os
import shutil
import struct
import subprocess
import tarfile

import numpy as np
import pytest
import torch

from brever_amd import flac_gpu, hip
from helpers import _crc, flac_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_host.py::test_flac_decoder_known_stream
KNOWN = bytes.fromhex('664c614380000022100010000000' '0f00000f0ac442f000000001'
                      '3e84b41807dc6903075' '86a3dad1a2e0f' 'fff869180000bf' '0358fd03128b' 'aa9a')


def _signal(n, channels, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(-300, 300, (n, channels)).cumsum(axis=0).clip(-30000, 30000)


def _boundaries(pcm, blocksize, **kw):
    """The stream of ``pcm`` and where each of its frames starts: frame k starts where the stream of the first k
    blocks ends (the encoder writes frames one after another, and a prefix's frames are the same bytes)."""
    data = flac_encode(pcm, blocksize=blocksize, **kw)
    n_frames = -(-len(pcm)//blocksize)
    starts = [len(flac_encode(pcm[:k*blocksize], blocksize=blocksize, **kw)) if k else 42 for k in range(n_frames)]
    return data, starts


@pytest.mark.parametrize('channels, stereo', [(1, 'independent'), (2, 'independent'), (2, 'mid_side')])
@pytest.mark.parametrize('blocksize, n', [(16, 2100), (192, 192*3 + 5), (4096, 4096*2 + 77)])
def test_index_finds_the_encoders_frames(channels, stereo, blocksize, n):
    """Mono and stereo, block sizes 16 (132 frames: the coded frame number takes two bytes from 128 on), 192 and
    4096, each with a short last block."""
    pcm = _signal(n, channels, seed=blocksize)
    data, starts = _boundaries(pcm, blocksize, stereo=stereo, kind='fixed', order=1, porder=1)
    info, frames = flac_gpu.index(data)
    assert info == dict(sample_rate=16000, channels=channels, bits_per_sample=16, total_samples=n,
                        min_block=n % blocksize, max_block=blocksize, first_frame=42, variable=0)
    assert frames[:, 0].tolist() == starts
    assert frames[:, 1].tolist() == [b - a for a, b in zip(starts, starts[1:] + [len(data)])]
    assert frames[:, 2].tolist() == list(range(0, n, blocksize))
    assert frames[:, 3].tolist() == [min(blocksize, n - s) for s in range(0, n, blocksize)]
    assert set(frames[:, 4].tolist()) == {10 if stereo == 'mid_side' else channels - 1}
    assert set(frames[:, 5].tolist()) == {16}
    assert frames[:, 6].tolist() == [8 if k < 128 else 9 for k in range(len(starts))]
    assert frames[:, 7].tolist() == list(range(len(starts)))
    if blocksize == 16:
        assert len(starts) == 132


def test_index_capacity_convention():
    data = flac_encode(_signal(2100, 1), blocksize=16, kind='fixed', order=0)
    buf = np.zeros((4, 8), dtype=np.int64)
    n = flac_gpu.lib().brv_flacdec_index(data, len(data), None, buf.ctypes.data_as(ctypes.c_void_p), 4)
    assert n == 132 and buf[3, 2] == 48                       # the number needed; what fits is filled
    assert flac_gpu.lib().brv_flacdec_index(data, len(data), None, None, 0) == 132


def test_a_planted_sync_pattern_does_not_split_a_frame():
    pcm = _signal(600, 1)
    pcm[40:120, 0] = -8                                       # 0xfff8: sync code + reserved bits, again and again
    pcm[130, 0], pcm[131, 0] = -8, 0x6918                     # ... and once followed by a plausible header
    data = flac_encode(pcm, blocksize=256, kind='verbatim')
    assert data.count(b'\xff\xf8') > 40
    info, frames = flac_gpu.index(data)
    assert frames[:, 3].tolist() == [256, 256, 88] and frames[:, 1].tolist() == [8 + 1 + 512 + 2]*2 + [8 + 1 + 176 + 2]


def test_index_of_the_known_stream():
    info, frames = flac_gpu.index(KNOWN)
    assert (info['sample_rate'], info['channels'], info['bits_per_sample'], info['total_samples']) == (44100, 2, 16, 1)
    assert frames.tolist() == [[42, 15, 0, 1, 1, 16, 7, 0]]


def test_index_counts_samples_when_the_header_says_zero():
    n = 1000
    data = bytearray(flac_encode(_signal(n, 2), blocksize=192))
    data[21] &= 0xf0
    data[22:26] = bytes(4)
    info, frames = flac_gpu.index(bytes(data))
    assert info['total_samples'] == n and len(frames) == 6 and frames[-1, 3] == n - 5*192


def test_index_skips_long_metadata():
    data = flac_encode(_signal(500, 1), blocksize=192)
    pad = 70000
    long = data[:4] + bytes([0x00]) + data[5:42] + bytes([0x81]) + pad.to_bytes(3, 'big') + bytes(pad) + data[42:]
    info, frames = flac_gpu.index(long)
    assert info['first_frame'] == 42 + 4 + pad > 1 << 16
    assert (frames[:, 0] - (4 + pad)).tolist() == flac_gpu.index(data)[1][:, 0].tolist()


def _code(data):
    with pytest.raises(flac_gpu.FlacIndexError) as e:
        flac_gpu.index(bytes(data), 'x.flac')
    assert 'x.flac' in str(e.value) and len(str(e.value)) > 20
    return e.value.code, str(e.value)


def test_index_rejections_have_their_own_codes_and_messages():
    seen = {}
    bad = bytearray(KNOWN); bad[-3] ^= 1                      # the flipped payload bit of the known stream
    seen['crc'] = _code(bad)
    assert seen['crc'][0] == flac_gpu.BAD_CRC16 == -61
    pcm = _signal(1000, 2)
    data = flac_encode(pcm, blocksize=192, stereo='left_side')
    frames = flac_gpu.index(data)[1]
    for k in (0, 3):                                          # a flipped header bit, first frame and a later one
        for bit in (2*8 + 1, 3*8 + 5, 4*8 + 7):                 # block size code, channel code, frame number
            bad = bytearray(data); bad[int(frames[k, 0]) + bit//8] ^= 0x80 >> (bit % 8)
            seen['header'] = _code(bad)
            assert seen['header'][0] == flac_gpu.BAD_HEADER == -60, (k, bit)
    bad = bytearray(data); bad[int(frames[2, 0]) + 20] ^= 4   # a flipped payload bit inside
    assert _code(bad)[0] == flac_gpu.BAD_CRC16                # ... of a middle frame: the same code, never 'truncated'
    removed = data[:int(frames[2, 0])] + data[int(frames[3, 0]):]
    seen['number'] = _code(removed)
    assert seen['number'][0] == flac_gpu.BAD_NUMBER == -62
    for cut in (1, 2, 3, 40, int(frames[-1, 1])):               # a truncated tail, the whole last frame among them
        seen['cut'] = _code(data[:-cut])
        assert seen['cut'][0] == flac_gpu.TRUNCATED == -63, cut
    seen['junk'] = _code(b'not a flac stream' + bytes(64))
    assert seen['junk'][0] == flac_gpu.NOT_FLAC == -10
    wide = bytearray(data); wide[8 + 12] |= 1; wide[8 + 13] |= 0xf0      # STREAMINFO: 32 bits per sample
    seen['wide'] = _code(wide)
    assert seen['wide'][0] == flac_gpu.NOT_TAKEN == -2 and '32 bits' in seen['wide'][1]
    assert len({v[0] for v in seen.values()}) == len(seen) == 6
    assert len({v[1].split('(status')[0].split(': ', 2)[-1] for v in seen.values()}) == 6      # and its own words


def _utf8(v):
    if v < 0x80:
        return bytes([v])
    extra = next(e for e in range(1, 7) if v < 1 << (5*e + 6))
    return bytes([((0xff00 >> (extra + 1)) & 0xff) | (v >> (6*extra))] +
                 [0x80 | ((v >> (6*e)) & 0x3f) for e in range(extra - 1, -1, -1)])


def _as_variable(data, frames):
    """The same stream in the variable-block-size blocking strategy: every header says so and carries the first
    sample's number instead of the frame's; both CRCs are written anew."""
    out = bytearray(data[:int(frames[0, 0])])
    for off, length, first, _, _, _, hdr, number in frames.tolist():
        f = data[off:off + length]
        head = bytes([f[0], f[1] | 1, f[2], f[3]]) + _utf8(first) + f[4 + len(_utf8(number)):hdr - 1]
        head += bytes([_crc(head, 0x07, 8)])
        body = head + f[hdr:-2]
        out += body + _crc(body, 0x8005, 16).to_bytes(2, 'big')
    return bytes(out)


def test_index_takes_the_variable_blocking_strategy():
    pcm = _signal(16*140 + 3, 1)
    data = flac_encode(pcm, blocksize=16, kind='fixed', order=2, porder=0)
    fixed = flac_gpu.index(data)[1]
    var = _as_variable(data, fixed)
    info, frames = flac_gpu.index(var)
    assert info['variable'] == 1 and info['total_samples'] == len(pcm)
    assert frames[:, 2:6].tolist() == fixed[:, 2:6].tolist()
    assert frames[:, 7].tolist() == fixed[:, 2].tolist()            # the coded number is the first sample
    assert frames[[1, 8, -1], 6].tolist() == [8, 9, 10]                # samples 16, 128, 2240: 1, 2, 3 bytes
    # a removed frame breaks the sample numbering too
    gone = var[:int(frames[5, 0])] + var[int(frames[6, 0]):]
    assert _code(gone)[0] == flac_gpu.BAD_NUMBER
    # the host decoder reads the same stream: the rewrite is a valid one
    import io
    from brever_amd.data import audio_read
    x, _ = audio_read(io.BytesIO(var), 'v.flac')
    assert np.array_equal(np.round(np.asarray(x, dtype=np.float64)*32768).astype(np.int64), pcm[:, 0])


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_flacdec_version', 'brv_flacdec_last_error', 'brv_flacdec_index', 'brv_flacdec_scratch_elems',
           'brv_flacdec_decode'}


def test_header_parses_and_every_export_resolves():
    with open(flac_gpu.HEADER_PATH) as f:
        table = hip.parse_header(f.read())
    assert set(table) == EXPORTS == set(flac_gpu.SIGNATURES)
    lib = flac_gpu.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.brv_flacdec_version() >= 100
    restype, argtypes = table['brv_flacdec_decode']
    assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr          # the stream, explicit
    assert (flac_gpu.INFO_WORDS, flac_gpu.FRAME_WORDS, flac_gpu.JOB_WORDS) == (8, 8, 12)
    with open(flac_gpu.HEADER_PATH) as f:
        constants = hip.parse_constants(f.read())
    assert constants == flac_gpu._LIB.constants and len(constants) == 13
    for name, value in (('INFO_WORDS', 8), ('FRAME_WORDS', 8), ('JOB_WORDS', 12), ('NOT_TAKEN', -2),
                        ('NOT_FLAC', -10), ('BAD_HEADER', -60), ('BAD_CRC16', -61),
                        ('BAD_NUMBER', -62), ('TRUNCATED', -63)):
        assert constants['BRV_FLACDEC_' + name] == getattr(flac_gpu, name) == value, name
    assert {name[len('BRV_FLACDEC_JOB_'):]: value for name, value in constants.items()
            if name.startswith('BRV_FLACDEC_JOB_') and name != 'BRV_FLACDEC_JOB_WORDS'} == \
        dict(BAD_FIELDS=1, RESERVED=2, OVERRUN=3, LENGTH=4)
    assert list(flac_gpu.JOB_MESSAGES) == [1, 2, 3, 4]


def test_every_entry_point_sets_its_message():
    lib = flac_gpu.lib()
    buf = ctypes.create_string_buffer(256)           # never read: each call below is refused on the host

    def refused(name, word, *args):
        arm = (1, 0, 1) if word == b'n_jobs' else (0, 1, 1)                # re-arm a known older message
        assert lib.brv_flacdec_scratch_elems(*arm) == -1
        sentinel = lib.brv_flacdec_last_error()
        assert (b'channels' if word == b'n_jobs' else b'n_jobs') in sentinel
        assert getattr(lib, name)(*args) == -1, name
        msg = lib.brv_flacdec_last_error()
        assert msg and msg != sentinel and word in msg, (name, msg)

    refused('brv_flacdec_index', b'null', None, 0, None, None, 0)
    refused('brv_flacdec_index', b'requires', buf, -1, None, None, 0)
    refused('brv_flacdec_index', b'null', buf, 64, None, None, 3)
    refused('brv_flacdec_scratch_elems', b'channels', 1, 9, 16)
    refused('brv_flacdec_scratch_elems', b'max_block', 1, 2, 65536)
    assert lib.brv_flacdec_scratch_elems(65, 2, 100) == 128*2*100
    good = [buf, 64, buf, 1, 1, 16, buf, 64*16, buf, 16, buf, None]
    refused('brv_flacdec_decode', b'null', *[None if a is buf else a for a in good])
    for pos, value, word in ((1, 63, b'bytes_size'), (3, 0, b'n_jobs'), (4, 0, b'channels'), (5, 0, b'max_block'),
                             (7, 64*16 - 1, b'scratch_elems'), (9, 0, b'out_elems')):
        args = list(good)
        args[pos] = value
        refused('brv_flacdec_decode', word, *args)
    with pytest.raises(RuntimeError, match='brv_flacdec_decode'):
        flac_gpu.call('brv_flacdec_decode', *[None if a is buf else a for a in good])
    with pytest.raises(RuntimeError, match='ROCm device'):
        flac_gpu.FlacBatchDecoder('cpu')


# -- the decode core on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def core_check(tmp_path_factory):
    """tools/flac_core_check.cpp built with the address and undefined-behaviour sanitizers (a stand-alone program:
    nothing is preloaded and nothing is loaded into python)."""
    exe = str(tmp_path_factory.mktemp('flac_core')/'flac_core_check')
    src = os.path.join(ROOT, 'tools', 'flac_core_check.cpp')
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    compilers = [c for c in (clang if os.path.exists(clang) else None, shutil.which('clang++'), shutil.which('g++'))
                 if c]
    assert compilers, 'no C++ compiler'
    flags = ['-std=c++17', '-O1', '-g']
    for sanitize in (['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], []):
        for cxx in compilers:
            r = subprocess.run([cxx] + flags + sanitize + [src, '-o', exe], capture_output=True, text=True)
            if r.returncode == 0:
                return exe, bool(sanitize)
    pytest.fail('tools/flac_core_check.cpp does not compile:\n' + r.stderr)


def test_core_check_program_under_the_sanitizers(core_check):
    exe, sanitized = core_check
    assert sanitized, 'no sanitizer runtime links here'
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'cases ok' in r.stdout and int(r.stdout.split()[1]) > 50000


@pytest.mark.parametrize('kw', [
    dict(kind='fixed', order=2, stereo='mid_side', porder=3), dict(kind='fixed', order=4, escape=True),
    dict(kind='fixed', order=3, stereo='side_right', five_bit=True, escape=True),
    dict(kind='lpc', order=32, stereo='mid_side', bps=24, blocksize=256), dict(kind='lpc', order=1, bps=12),
    dict(kind='verbatim', bps=20, stereo='left_side'),
])
def test_core_decodes_what_the_test_encoder_writes(core_check, tmp_path, kw):
    """The index's frame table and the core, the kernel's own code, on the CPU: the PCM that went in."""
    bps = kw.get('bps', 16)
    n = 1500
    t = np.arange(n)
    amp = 2**(bps - 3)
    left = amp*np.sin(2*np.pi*220*t/16000) + np.random.default_rng(1).normal(0, amp/200, n)
    pcm = np.stack([left, 0.8*left + amp/8*np.sin(2*np.pi*950*t/16000)], axis=1).round().astype(np.int64)
    pcm[100:400] = 0
    pcm[1024:1400] = (pcm[1024:1400] >> 3) << 3
    data = flac_encode(pcm, **{**dict(blocksize=512, bps=bps), **kw})
    frames = flac_gpu.index(data)[1]
    (tmp_path/'s.flac').write_bytes(data)
    frames.tofile(str(tmp_path/'frames.bin'))
    r = subprocess.run([core_check[0], 'decode', str(tmp_path/'s.flac'), str(tmp_path/'frames.bin'),
                        str(tmp_path/'out.bin')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(str(tmp_path/'out.bin'), dtype=np.int32).reshape(n, 2)
    assert np.array_equal(got, pcm)


# -- the dataset's switch ----------------------------------------------------------------------------------------
def _wav_bytes(x, fs=16000):
    pcm = np.asarray(x, dtype='<i2')
    return (b'RIFF' + struct.pack('<I', 36 + pcm.nbytes) + b'WAVEfmt ' +
            struct.pack('<IHHIIHH', 16, 1, pcm.shape[1], fs, fs*2*pcm.shape[1], 2*pcm.shape[1], 16) +
            b'data' + struct.pack('<I', pcm.nbytes) + pcm.tobytes())


def test_enable_gpu_decode_refuses_wav_and_dynamic_mixing(tmp_path):
    from brever_amd import data
    for ext, root in (('wav', tmp_path/'w'), ('flac', tmp_path/'f')):
        os.makedirs(root/'audio')
        for src in ('mixture', 'foreground'):
            pcm = _signal(700, 2)
            (root/'audio'/f'00000_{src}.{ext}').write_bytes(_wav_bytes(pcm) if ext == 'wav' else flac_encode(pcm))
        with tarfile.open(root/'audio.tar', 'w') as tar:
            tar.add(root/'audio', arcname='audio')
    wav = data.BreverDataset(str(tmp_path/'w'))
    with pytest.raises(ValueError, match='FLAC members'):
        data.enable_gpu_decode(wav)
    assert isinstance(wav[0], torch.Tensor)
    data.set_mixture_maker(data.SyntheticMixtureMaker)
    try:
        dyn = data.BreverDataset(str(tmp_path), dynamic_mixing=True, dynamic_mixtures_per_epoch=3)
        with pytest.raises(ValueError, match='dynamic mixing'):
            data.enable_gpu_decode(dyn)
    finally:
        data.set_mixture_maker(None)
    with pytest.raises(ValueError, match='BreverDataset'):
        data.enable_gpu_decode(data.SyntheticMixtureDataset(2, 100))
    # FLAC members: the switch is an attribute, set through a Subset too; items turn into compressed ones
    dset = data.BreverDataset(str(tmp_path/'f'), segment_length=0.02, segment_strategy='pass')
    assert dset._gpu_decode is False and isinstance(dset[0], torch.Tensor)
    assert data.enable_gpu_decode(torch.utils.data.Subset(dset, [0, 1])) is dset and dset._gpu_decode is True
    item = dset[1]
    assert isinstance(item, data.CompressedItem) and item.window == (320, 640)
    assert [len(m) for m in item.members] == [len((tmp_path/'f'/'audio'/f'00000_{s}.flac').read_bytes())
                                              for s in ('mixture', 'foreground')]
    assert item.tables[0][0]['total_samples'] == 700 and item.tables[0][1].shape == (1, 8)
    batch = data.BreverDataLoader._collate_fn([dset[0], dset[2]])
    assert isinstance(batch, data.CompressedBatch) and len(batch) == 2
    with pytest.raises(RuntimeError, match='ROCm device'):
        list(data.DevicePrefetcher(data.BreverDataLoader(dset, batch_size=2), 'cpu'))


def test_collate_of_tensor_items_is_unchanged():
    from brever_amd.data import BreverDataLoader
    a = torch.tensor([[1., 2., 3.], [4., 5., 6.]])
    b = torch.tensor([[7.], [8.]])
    batch, lengths = BreverDataLoader._collate_fn([a, b])
    assert batch.tolist() == [[[1., 2., 3.], [4., 5., 6.]], [[7., 0., 0.], [8., 0., 0.]]]
    assert lengths.tolist() == [3, 1] and lengths.dtype == torch.int64
    batch, lengths = BreverDataLoader._collate_fn([(a, b[0]), (b, a[1])])
    assert [x.tolist() for x in batch] == [[[[1., 2., 3.], [4., 5., 6.]], [[7., 0., 0.], [8., 0., 0.]]],
                                           [[7., 0., 0.], [4., 5., 6.]]]
    assert lengths.tolist() == [[3, 1], [1, 3]]
