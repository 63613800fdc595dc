"""The host side of the GPU FLAC encoder (include/brever_flacenc.h, brever_amd/flac_enc.py): the binding and its
refusals, the size queries, the stand-alone check of the encode core under the sanitizers, the NumPy restatement of
the decision rule against hand-computed frames and against the core run on the CPU, and the command line of
scripts/create_dataset.py. No test here needs a device."""
import ctypes
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import flacenc_ref
from brever_amd import flac_enc, flac_gpu, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {'brv_flacenc_version', 'brv_flacenc_last_error', 'brv_flacenc_frame_capacity',
           'brv_flacenc_scratch_elems', 'brv_flacenc_out_capacity', 'brv_flacenc_encode'}


# -- the C ABI ---------------------------------------------------------------------------------------------------
def test_header_parses_and_every_export_resolves():
    with open(flac_enc.HEADER_PATH) as f:
        text = f.read()
    table = hip.parse_header(text)
    assert set(table) == EXPORTS == set(flac_enc.SIGNATURES)
    lib = flac_enc.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.brv_flacenc_version() >= 100
    restype, argtypes = table['brv_flacenc_encode']
    assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr          # the stream, explicit
    constants = hip.parse_constants(text)
    assert constants == flac_enc._LIB.constants == {'BRV_FLACENC_' + name: value for name, value in (
        ('ROW_NONFINITE', 1), ('ROW_RANGE', 2), ('ROW_LENGTH', 4), ('ROW_INTERNAL', 8), ('MAX_LPC_ORDER', 32),
        ('MAX_ROWS', 65535))}
    assert (flac_enc.MAX_ROWS, flac_enc.MAX_LPC_ORDER) == \
        (constants['BRV_FLACENC_MAX_ROWS'], constants['BRV_FLACENC_MAX_LPC_ORDER'])
    assert set(flac_enc.ROW_MESSAGES) == {1, 2, 4, 8}
    assert (flac_enc.MAX_ROWS, flac_enc.MAX_LPC_ORDER) == (65535, 32)


def test_every_entry_point_sets_its_message():
    lib = flac_enc.lib()
    buf = ctypes.create_string_buffer(4096 + 256)    # never read or written: each call below is refused on the host
    aligned = ctypes.c_void_p((ctypes.addressof(buf) + 255)//256*256)

    def refused(name, word, *args):
        arm = (3, 16, 4096) if word != b'channels' else (1, 12, 4096)      # re-arm a known older message
        assert lib.brv_flacenc_frame_capacity(*arm) == -1
        sentinel = lib.brv_flacenc_last_error()
        assert (b'channels' if word != b'channels' else b'bits_per_sample') in sentinel
        assert getattr(lib, name)(*args) == -1, name
        msg = lib.brv_flacenc_last_error()
        assert msg and msg != sentinel and word in msg, (name, msg)

    refused('brv_flacenc_frame_capacity', b'bits_per_sample', 2, 20, 4096)
    refused('brv_flacenc_frame_capacity', b'block_size', 2, 16, 15)
    refused('brv_flacenc_frame_capacity', b'block_size', 2, 16, 65536)
    for name in ('brv_flacenc_scratch_elems', 'brv_flacenc_out_capacity'):
        refused(name, b'rows', 0, 2, 100, 16, 4096)
        refused(name, b'rows', 65536, 2, 100, 16, 4096)
        refused(name, b'channels', 1, 3, 100, 16, 4096)
        refused(name, b'max_len', 1, 2, 0, 16, 4096)
        refused(name, b'max_len', 1, 2, (1 << 30) + 1, 16, 4096)
        refused(name, b'frames', 65535, 1, 1 << 20, 16, 16)
        refused(name, b'per row', 1, 2, 1 << 30, 24, 65535)
    scratch = lib.brv_flacenc_scratch_elems(2, 2, 100, 16, 16)
    out = lib.brv_flacenc_out_capacity(2, 2, 100, 16, 16)
    good = [aligned, 0, aligned, 2, 2, 100, 16000, 16, 16, 8, aligned, scratch, aligned, out, aligned, None]
    for pos in (0, 2, 10, 12, 14):
        args = list(good)
        args[pos] = None
        refused('brv_flacenc_encode', b'null', *args)
    for pos, value, word in ((3, 0, b'rows'), (4, 0, b'channels'), (5, 0, b'max_len'), (6, 0, b'sample_rate'),
                             (6, 655351, b'sample_rate'), (7, 8, b'bits_per_sample'), (8, 8, b'block_size'),
                             (9, -1, b'lpc_order'), (9, 33, b'lpc_order'), (11, scratch - 1, b'scratch_elems'),
                             (13, out - 1, b'out_capacity'),
                             (10, ctypes.c_void_p(aligned.value + 4), b'aligned')):
        args = list(good)
        args[pos] = value
        refused('brv_flacenc_encode', word, *args)
    with pytest.raises(RuntimeError, match='brv_flacenc_encode'):
        flac_enc.call('brv_flacenc_encode', *[None if a is aligned else a for a in good])
    with pytest.raises(ValueError, match='block_size'):
        flac_enc.query('brv_flacenc_frame_capacity', 2, 16, 3)
    with pytest.raises(RuntimeError, match='ROCm device'):
        flac_enc.FlacBatchEncoder('cpu')


def test_capacities_are_monotone_and_hold_the_worst_case():
    lib = flac_enc.lib()
    for channels in (1, 2):
        for bps in (16, 24):
            last = 0
            for block in (16, 17, 192, 255, 256, 4096, 4097, 65535):
                cap = lib.brv_flacenc_frame_capacity(channels, bps, block)
                # the worst frame: the longest header (a 6-byte number, a 16-bit block size), VERBATIM subframes with a
                # side channel one bit wider, padding, CRC-16 -- and the word the bit writer looks ahead
                worst = 4 + 6 + 2 + 1 + (8*channels + block*(bps*channels + (channels == 2)) + 7)//8 + 2
                assert cap >= worst + 8 and cap % 256 == 0 and cap >= last, (channels, bps, block)
                last = cap
    base = (3, 2, 1000, 16, 256)
    for name in ('brv_flacenc_scratch_elems', 'brv_flacenc_out_capacity'):
        fn = getattr(lib, name)
        n = fn(*base)
        assert n > 0
        for pos, more in ((0, 4), (1, 2), (2, 1001), (2, 1025), (3, 24)):
            args = list(base)
            args[pos] = more
            if pos == 1:
                args[1], n1 = 1, fn(3, 1, 1000, 16, 256)
                assert n1 <= n
            else:
                assert fn(*args) >= n, (name, pos)
    # every frame's image and the streams' bytes fit what the queries say
    frames = -(-1000//256)
    cap = lib.brv_flacenc_frame_capacity(2, 16, 256)
    assert lib.brv_flacenc_scratch_elems(*base)*4 >= 3*frames*cap
    assert lib.brv_flacenc_out_capacity(*base) >= 3*(42 + frames*cap)


# -- the encode core on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def enc_check(tmp_path_factory):
    """tools/flac_enc_check.cpp built with the address and undefined-behaviour sanitizers (a stand-alone program:
    nothing is preloaded and nothing is loaded into python)."""
    exe = str(tmp_path_factory.mktemp('flac_enc')/'flac_enc_check')
    src = os.path.join(ROOT, 'tools', 'flac_enc_check.cpp')
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    compilers = [c for c in (clang if os.path.exists(clang) else None, shutil.which('clang++'), shutil.which('g++'))
                 if c]
    assert compilers, 'no C++ compiler'
    flags = ['-std=c++17', '-O1', '-g', '-ffp-contract=off']
    for sanitize in (['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], []):
        for cxx in compilers:
            r = subprocess.run([cxx] + flags + sanitize + [src, '-o', exe], capture_output=True, text=True)
            if r.returncode == 0:
                return exe, bool(sanitize)
    pytest.fail('tools/flac_enc_check.cpp does not compile:\n' + r.stderr)


def test_enc_check_program_passes_its_corpus(enc_check):
    exe, _ = enc_check
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert 'ok' in words and int(words[1]) > 4000 and int(words[4]) > 3000


def _core_stream(enc_check, tmp_path, pcm, bps, block, lpc=0, rate=16000):
    """The stream the encode core writes for ``pcm`` (channels, n), run on the CPU."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int32)
    pcm.tofile(str(tmp_path/'pcm.bin'))
    r = subprocess.run([enc_check[0], 'encode', str(tmp_path/'pcm.bin'), str(pcm.shape[0]), str(bps), str(block),
                        str(lpc), str(rate), str(tmp_path/'out.flac')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return (tmp_path/'out.flac').read_bytes()


def _host_decode(data, bps):
    from brever_amd.data import audio_read
    x, rate = audio_read(io.BytesIO(data), 'x.flac')
    x = np.asarray(x, dtype=np.float64)
    x = x[None, :] if x.ndim == 1 else x.T
    return np.round(x*2.0**(bps - 1)).astype(np.int64), rate


@pytest.mark.parametrize('bps', [16, 24])
@pytest.mark.parametrize('block', [16, 64])
def test_the_core_reaches_the_brute_force_minimum(enc_check, tmp_path, bps, block):
    """The decision rule on the CPU: every frame the core writes without LPC is exactly as long as the shortest one
    of the search space, decodes to the samples that went in, and every kind and assignment wins somewhere."""
    blocks = flacenc_ref.decision_blocks(bps, block, seed=bps + block)
    seen_kinds, seen_assignments = set(), set()
    for stereo in (True, False):
        pcm = np.concatenate(blocks, axis=1)
        pcm = pcm if stereo else pcm[:1]
        data = _core_stream(enc_check, tmp_path, pcm, bps, block)
        info, frames = flac_gpu.index(data)
        want = flacenc_ref.stream_frame_bytes(pcm, bps, block)
        assert info['total_samples'] == pcm.shape[1] and len(frames) == len(want)
        assert frames[:, 1].tolist() == [w[0] for w in want]
        assert frames[:, 4].tolist() == [w[1] for w in want]      # the helper's order of ties is the encoder's
        got, rate = _host_decode(data, bps)
        assert rate == 16000 and np.array_equal(got, pcm)
        for _, assignment, kinds in want:
            seen_assignments.add(assignment)
            seen_kinds.update(kinds)
    assert seen_assignments == {0, 1, 8, 9, 10}
    assert {'constant', 'verbatim'} <= seen_kinds and len({k for k in seen_kinds if k.startswith('fixed')}) >= 3


def test_core_with_lpc_is_never_longer_and_wins_on_tones(enc_check, tmp_path):
    t = np.arange(4096)
    tone = 0.4*np.sin(2*np.pi*5000*t/16000) + 0.3*np.sin(2*np.pi*6500*t/16000 + 1)
    for bps in (16, 24):
        pcm = flacenc_ref.quantise(tone, bps)[None]
        plain = _core_stream(enc_check, tmp_path, pcm, bps, 4096, lpc=0)
        lpc = _core_stream(enc_check, tmp_path, pcm, bps, 4096, lpc=8)
        assert len(lpc) < len(plain)
        assert np.array_equal(_host_decode(lpc, bps)[0], pcm)
        assert flac_gpu.index(lpc)[1][0, 1] == len(lpc) - 42


# -- the NumPy restatement against frames worked out by hand -----------------------------------------------------
def test_reference_helper_on_hand_computed_frames():
    # 16 equal samples, mono, 16 bits: header 4 bytes + number 1 + explicit 8-bit block size 1 + CRC-8 1 = 56 bits;
    # CONSTANT subframe 8 + 16 bits; 80 bits = 10 bytes, and the CRC-16
    assert flacenc_ref.frame_choice(np.full((1, 16), 5), 16) == (12, 0, ['constant'])
    # a ramp of 192 samples (block size code 1: no extra byte, header 48 bits): FIXED 2 has zero residuals --
    # 8 + 2 x 16 warm-up + 2 + 4 + one 4-bit parameter 0 + 190 one-bit codes = 240 bits; FIXED 3 spends 16 more on the
    # third warm-up sample and saves one code. 288 bits = 36 bytes, and the CRC-16
    assert flacenc_ref.frame_choice((3*np.arange(192) + 7)[None], 16) == (38, 0, ['fixed2'])
    # 16 samples alternating between the range ends: FIXED 0 needs 17 bits a sample at parameter 15 (272 + 5 + 6
    # bits) or 18 at parameter 14, every higher order doubles the residual; VERBATIM is 8 + 256 bits.
    # 56 + 264 = 320 bits = 40 bytes, and the CRC-16
    ends = np.where(np.arange(16) % 2 == 0, 32767, -32768)[None]
    assert flacenc_ref.frame_choice(ends, 16) == (42, 0, ['verbatim'])
    # the same in both channels: the side channel is CONSTANT zero (8 + 17 bits), left is VERBATIM: left/side wins
    # over independent (2 x 264) and ties with mid/side, which comes later. 56 + 264 + 25 = 345 bits -> 44 bytes + 2
    assert flacenc_ref.frame_choice(np.concatenate([ends, ends]), 16) == (46, 8, ['verbatim', 'constant'])
    # frame numbers: 1 byte below 128, 2 below 2048, 3 below 65536
    assert [flacenc_ref.number_bytes(v) for v in (0, 127, 128, 2047, 2048, 65535, 65536)] == [1, 1, 2, 2, 3, 3, 4]
    assert flacenc_ref.min_frame_bytes(np.full((1, 16), 5), 16, number=2099) == 14
    # full-scale white noise codes longer with every FIXED order than verbatim
    noise = np.random.default_rng(0).integers(-32768, 32768, 4096)[None]
    assert flacenc_ref.frame_choice(noise, 16)[2] == ['verbatim']
    assert flacenc_ref.quantise([1.0, -1.0, 0.5/32768, 1.5/32768, 2.5/32768, -0.5/32768], 16).tolist() == \
        [32767, -32768, 0, 2, 2, 0]


# -- the command line ----------------------------------------------------------------------------------------------
def test_create_dataset_help_and_refusal_of_an_existing_dataset(tmp_path):
    script = os.path.join(ROOT, 'scripts', 'create_dataset.py')
    r = subprocess.run([sys.executable, script, '-h'], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for option in ('--pool', '--output', '--size', '--sources', '--seed', '--epoch', '--bits', '--no_tar', '-f',
                   '--noise_count', '--snr', '--diffuse'):
        assert option in r.stdout, option
    (tmp_path/'mixture_info.json').write_text('[]')
    pool = tmp_path/'pools.npz'
    np.savez(pool, speech_0=np.zeros(100, dtype=np.float32), brir_0_0=np.zeros((4, 2), dtype=np.float32))
    r = subprocess.run([sys.executable, script, '--pool', str(pool), '--output', str(tmp_path), '--size', '2'],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and 'already exists' in r.stderr
    assert (tmp_path/'mixture_info.json').read_text() == '[]' and not (tmp_path/'audio.tar').exists()
