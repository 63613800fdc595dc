"""The Fourier resampler on the host: the NumPy restatement (tests/resample_ref.py) against the reference's recorded
output and scipy, the output-length rule, the yardsticks and the tie margin the GPU tests rely on, the C ABI of
libbrever_resample.so (header, exports, refusals), the chirp cache's bookkeeping, and the host logic of
scripts/vbdemand_to_brever.py with the resampler replaced by the restatement. No GPU."""
import ctypes
import io as pyio
import os
import tarfile

import numpy as np
import pytest

import resample_ref as R
import vbdemand_fixture as V
from brever_amd import hip, io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [(48000, 16000), (44100, 16000), (16000, 48000), (8000, 16000)]


# -- the restatement ---------------------------------------------------------------------------------------------
def test_restatement_equals_the_recorded_reference():
    z = R.golden()
    assert {c[0] for c in R.GOLDEN_CASES} == {1, 2, 3, 7, 8, 16, 441, 442, 4800, 4801, 4802}
    assert {c[1:3] for c in R.GOLDEN_CASES} == set(RATES) and any(c[3] == 2 for c in R.GOLDEN_CASES)
    for case in R.GOLDEN_CASES:
        x, ref = z['x_' + R.case_key(case)], z['y_' + R.case_key(case)]
        assert np.array_equal(x, R.case_input(case)) and np.array_equal(np.round(x*32768), x*32768)
        got = R.resample(x, case[1], case[2])
        assert got.shape == ref.shape == (R.out_length(*case[:3]),) + x.shape[1:]
        assert np.linalg.norm(got - ref) <= 1e-13*np.linalg.norm(ref), case


def test_restatement_equals_scipy_on_every_gpu_length():
    signal = pytest.importorskip('scipy.signal')
    for case in R.CASES:
        x = R.case_input(case)
        ref = signal.resample(x, R.out_length(*case[:3]), axis=0)
        got = R.resample(x, case[1], case[2])
        assert np.linalg.norm(got - ref) <= 1e-13*np.linalg.norm(ref), case


def test_restatement_along_another_axis():
    x = R.case_input((442, 44100, 16000, 2))
    assert np.array_equal(R.resample(x.T, 44100, 16000, axis=1), R.resample(x, 44100, 16000).T)


def test_output_length_is_the_exact_rational_ceiling():
    n = np.arange(1, 600001, dtype=np.int64)
    for old, new in RATES:
        got = io.out_length(n, old, new)
        assert got.dtype == np.int64 and np.array_equal(got, (n*new + old - 1)//old), (old, new)
        for k in (1, 2, 3, 441, 4801, 599999):
            assert io.out_length(k, old, new) == R.out_length(k, old, new) == int(got[k - 1])


# -- what the GPU tests rely on ----------------------------------------------------------------------------------
def test_yardsticks_of_the_kernels_algorithm_in_numpy():
    """rel-L2 error of the complex128 Bluestein restatement (same L, same decomposition) per case, printed; the
    recorded values (tests/golden/resample.npz) are what the GPU value test multiplies by 8."""
    z = R.golden()
    for case in R.CASES:
        recorded = float(z['yard_' + R.case_key(case)])
        if case[0] > 200000:                     # the largest class takes seconds in NumPy: its record is used as is
            print(case, f'recorded {recorded:.3e}')
            assert 0 < recorded < 1e-14
            continue
        got = R.yardstick(case)
        print(case, f'measured {got:.3e} recorded {recorded:.3e}')
        assert got < 1e-14
        assert got == recorded or 0.5*recorded <= got <= 2*recorded, case      # (another libm: a few ulps)
    assert R.fft_length(1048579, 349527) == 1 << 21 and R._plan(1 << 21) == ([1, 8], 12)
    assert R._plan(1 << 20) == ([8], 12) and R._plan(4096) == ([], 12) and R._plan(16) == ([], 4)


def test_no_sample_of_the_pcm_cases_is_near_a_tie():
    closest = 1.0
    for case in R.PCM_CASES:
        v = 32768.0*R.reference(case)
        d = np.abs(v - np.floor(v) - 0.5).min()
        closest = min(closest, d)
        assert d > 2.0**-24, (case, d)
    print(f'closest sample to a tie: {closest:.3e} of an int16 step')
    assert sum(R.reference(c).size for c in R.PCM_CASES) > 2e5


def test_library_length_rule_is_the_restatements():
    for n, m in [(1, 1), (2, 1), (7, 21), (4801, 1601), (70001, 25398), (1048579, 349527), (1 << 22, 1 << 22)]:
        assert io.fft_length(n, m) == R.fft_length(n, m)
    assert io.plan(4802, 48000, 16000) == (1601, 8192)
    assert io.max_length() >= 1 << 22
    with pytest.raises(ValueError, match=str(io.max_length())):
        io.plan(io.max_length() + 1, 48000, 16000)
    with pytest.raises(ValueError, match=str(io.max_length())):
        io.plan(io.max_length(), 16000, 48000)                           # the output is too long
    with pytest.raises(ValueError, match='empty'):
        io.plan(0, 48000, 16000)


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_rs_version', 'brv_rs_last_error', 'brv_rs_max_length', 'brv_rs_fft_length', 'brv_rs_chirp_spectra',
           'brv_rs_analysis', 'brv_rs_synthesis'}
KERNEL_CALLS = sorted(EXPORTS - {'brv_rs_version', 'brv_rs_last_error', 'brv_rs_max_length', 'brv_rs_fft_length'})


def test_header_parses_and_every_export_resolves():
    with open(io.HEADER_PATH) as f:
        table = hip.parse_header(f.read())
    assert set(table) == EXPORTS == set(io.SIGNATURES)
    lib = io.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        if name in KERNEL_CALLS:
            assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr, name
    assert lib.brv_rs_version() >= 100
    from brever_amd import mixture
    assert not any(n.startswith('brv_rs_') for n in list(hip.SIGNATURES) + list(mixture.SIGNATURES))
    assert not hasattr(hip.lib(), 'brv_rs_version')
    # the limit is the header's macro
    assert io._LIB.constants == {'BRV_RS_MAX_COLUMNS': 32768} and io.MAX_COLUMNS == 32768


def _args(name, fill, fft_len=4096):
    """Arguments a call would accept: every pointer ``fill``, every number 1, fft_len a power of two, no stream."""
    _, argtypes = io.SIGNATURES[name]
    names = _arg_names(name)
    return [None if i == len(argtypes) - 1 else fill if t is hip._c_ptr else fft_len if names[i] == 'fft_len' else 1
            for i, t in enumerate(argtypes)]


def _arg_names(name):
    import re
    with open(io.HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    args = re.search(name + r'\s*\(([^)]*)\)', text).group(1)
    return [a.split()[-1].lstrip('*') for a in args.split(',')]


@pytest.mark.parametrize('name', KERNEL_CALLS)
def test_every_export_refuses_null_negative_and_too_long(name):
    lib = io.lib()
    _, argtypes = io.SIGNATURES[name]
    names = _arg_names(name)
    buf = ctypes.create_string_buffer(64)            # never read: each call below is refused on the host
    assert lib.brv_rs_fft_length(0, 1) == -1
    sentinel = lib.brv_rs_last_error()
    assert sentinel
    assert getattr(lib, name)(*_args(name, None)) == -1
    null_msg = lib.brv_rs_last_error()
    assert null_msg and b'null' in null_msg and null_msg != sentinel          # a refusal overwrites the older message
    for i, t in enumerate(argtypes[:-1]):
        if t is hip._c_ptr:
            continue
        args = _args(name, buf)
        args[i] = -1
        assert getattr(lib, name)(*args) == -1, (name, names[i])
        msg = lib.brv_rs_last_error()
        assert msg and msg != null_msg and b'requires' in msg, (name, names[i], msg)
    for bad, status in ((4097, -1), (8, -1), (1 << 24, -2)):                     # not a power of two, short, too long
        assert getattr(lib, name)(*_args(name, buf, fft_len=bad)) == status, (name, bad)
        assert lib.brv_rs_last_error() not in (null_msg, b'')
    assert b'4194304' in lib.brv_rs_last_error()                                 # the limit, named
    with pytest.raises(RuntimeError, match=name):
        io.call(name, *_args(name, None))


def test_length_queries_refuse_with_a_message():
    lib = io.lib()
    top = lib.brv_rs_max_length()
    assert lib.brv_rs_fft_length(top, top) == 1 << 23
    for n, m in ((0, 1), (1, 0), (-5, 3)):
        assert lib.brv_rs_fft_length(n, m) == -1 and b'requires' in lib.brv_rs_last_error()
    for n, m in ((top + 1, 1), (1, top + 1)):
        assert lib.brv_rs_fft_length(n, m) == -1 and str(top).encode() in lib.brv_rs_last_error()


# -- the chirp cache's bookkeeping (meta tensors: nothing is allocated) ------------------------------------------------
def test_chirp_cache_hits_misses_and_evictions():
    cache = io.ChirpCache(max_bytes=4*3*16*1024)                 # slabs of a quarter of it: three slots of L = 1024
    assert cache.slots(1024) == 3 and cache.slots(1 << 20) == 1
    slab, slots, fill = cache.acquire([(0, 700), (0, 701), (0, 700)], 1024, 'meta')
    assert slab.shape == (3, 1024, 2) and len(slots) == 2 and len(fill) == 2
    assert (cache.hits, cache.misses, cache.evictions) == (0, 2, 0)
    assert sorted(f[1:] for f in fill) == [(700, 0), (701, 0)] and {f[0] for f in fill} == set(slots.values())
    _, again, fill = cache.acquire([(0, 701)], 1024, 'meta')
    assert again[(0, 701)] == slots[(0, 701)] and not fill and (cache.hits, cache.misses) == (1, 2)
    _, more, fill = cache.acquire([(1, 234), (1, 235)], 1024, 'meta')          # one free slot, one eviction: (0, 700)
    assert (cache.hits, cache.misses, cache.evictions) == (1, 4, 1)
    assert set(more.values()) | {slots[(0, 701)]} == {0, 1, 2}
    _, _, fill = cache.acquire([(0, 700)], 1024, 'meta')                       # it is gone: filled again
    assert len(fill) == 1 and cache.misses == 5
    with pytest.raises(ValueError, match='holds 3'):
        cache.acquire([(0, k) for k in range(4)], 1024, 'meta')
    cache.acquire([(0, 5)], 2048, 'meta')
    cache.acquire([(0, 5)], 4096, 'meta')                                      # 48 + 32 + 64 KiB: all held
    assert cache.bytes <= cache.max_bytes
    cache.acquire([(0, 5)], 8192, 'meta')                                      # + 128 KiB: the oldest slabs go
    assert cache.bytes <= cache.max_bytes and (str('meta'), 1024) not in cache._slabs


# -- scripts/vbdemand_to_brever.py ------------------------------------------------------------------------------------
@pytest.fixture()
def vb(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'scripts'))
    import vbdemand_to_brever as module
    monkeypatch.setattr(module, '_resample', lambda xs, rates: [R.resample(x, fs, 16000) for x, fs in zip(xs, rates)])
    return module


def _members(path):
    with tarfile.open(path) as tar:
        return tar.getnames()


def _decoded(path, name):
    from brever_amd.data import audio_read
    with tarfile.open(path) as tar:
        x, fs = audio_read(pyio.BytesIO(tar.extractfile(name).read()), name)
    assert fs == 16000
    return np.round(x.astype(np.float64)*32768).astype(np.int16)


def _check_archives(out, sig):
    for split, items in V.expected(sig).items():
        path = os.path.join(out, split, 'vbdemand', 'audio.tar')
        want = [f'audio/{i:05d}_mixture.flac' for i in range(len(items))] + \
               [f'audio/{i:05d}_foreground.flac' for i in range(len(items))]
        assert _members(path) == want, split
        for i, (name, noisy, clean) in enumerate(items):
            for source, pcm in (('mixture', noisy), ('foreground', clean)):
                ref = R.pcm16(R.resample(pcm/32768.0, 48000, 16000))
                assert np.array_equal(_decoded(path, f'audio/{i:05d}_{source}.flac'), ref), (split, name, source)


def test_script_members_order_and_speaker_split(vb, tmp_path):
    sig = V.build(tmp_path/'vb.zip')
    out = str(tmp_path/'datasets')
    vb.main(['--vbdemand_path', str(tmp_path/'vb.zip'), '--datasets_dir', out, '--batch', '4'])
    _check_archives(out, sig)
    assert [n for n, _, _ in V.expected(sig)['val']] == ['p226_001', 'p287_001', 'p226_002']
    # other validation speakers, the inner zips in a directory: the split follows
    V.build(tmp_path/'dir', as_directory=True)
    vb.main(['--vbdemand_path', str(tmp_path/'dir'), '--datasets_dir', str(tmp_path/'other'), '--val_speakers', 'p300'])
    assert len(_members(tmp_path/'other'/'val'/'vbdemand'/'audio.tar')) == 6
    assert len(_members(tmp_path/'other'/'train'/'vbdemand'/'audio.tar')) == 6


def test_script_appends_skips_and_rewrites(vb, tmp_path, monkeypatch, capsys):
    sig = V.build(tmp_path/'vb.zip')
    out = str(tmp_path/'datasets')
    argv = ['--vbdemand_path', str(tmp_path/'vb.zip'), '--datasets_dir', out]
    vb.main(argv)
    train = os.path.join(out, 'train', 'vbdemand', 'audio.tar')
    first = _members(train)
    calls = []
    real = vb._resample
    monkeypatch.setattr(vb, '_resample', lambda xs, rates: calls.append(len(xs)) or real(xs, rates))
    vb.main(argv)                                            # everything present: nothing is resampled or added
    assert not calls and _members(train) == first
    # a partial archive: only what is missing is added, behind what is there
    with tarfile.open(train) as tar:
        keep = [(m, tar.extractfile(m).read()) for m in tar.getmembers() if '00001' not in m.name]
    with tarfile.open(train, 'w') as tar:
        for m, blob in keep:
            tar.addfile(m, pyio.BytesIO(blob))
    vb.main(argv)
    assert calls == [1, 1] and sorted(_members(train)) == sorted(first) and _members(train)[:4] == [m.name for m, _ in keep]
    calls.clear()
    vb.main(argv + ['-f'])                                   # afresh
    assert sum(calls) == 16 and _members(train) == first
    _check_archives(out, sig)
    with open(train, 'wb') as f:                             # unreadable: recreated, with the reference's message
        f.write(b'this is not a tar archive' * 50)
    capsys.readouterr()
    vb.main(argv)
    assert 'output archive is corrupted, recreating...' in capsys.readouterr().out and _members(train) == first


def test_script_refuses_unpaired_and_multichannel_members(vb, tmp_path):
    V.build(tmp_path/'vb.zip', rename_clean=(2, 'p300_009'))
    with pytest.raises(ValueError, match='p300_009'):
        vb.main(['--vbdemand_path', str(tmp_path/'vb.zip'), '--datasets_dir', str(tmp_path/'d')])
    import zipfile
    stereo = V.wav_bytes(np.zeros((9601, 2), dtype=np.int16), channels=2)
    os.makedirs(tmp_path/'st')
    for kind in ('noisy', 'clean'):
        for suffix in ('trainset_28spk', 'testset'):
            with zipfile.ZipFile(tmp_path/'st'/f'{kind}_{suffix}_wav.zip', 'w') as z:
                z.writestr('p300_001.wav', stereo)
    with pytest.raises(ValueError, match=r'p300_001\.wav.*2 channels'):
        vb.main(['--vbdemand_path', str(tmp_path/'st'), '--datasets_dir', str(tmp_path/'d2')])


def test_script_without_a_path_names_the_archive_and_opens_no_socket(vb, monkeypatch):
    import socket

    def no_socket(*a, **k):
        raise AssertionError('the script opened a socket')
    monkeypatch.setattr(socket, 'socket', no_socket)
    monkeypatch.setattr(socket, 'create_connection', no_socket)
    with pytest.raises(SystemExit) as e:
        vb.main([])
    assert 'DS_10283_2791.zip' in str(e.value) and 'vbdemand_path' in str(e.value)
    with pytest.raises(SystemExit):
        vb.main(['--help'])


def test_flac_bytes_is_what_write_flac_writes(tmp_path):
    from brever_amd.data import flac_bytes, write_flac
    x = R.case_input((4801, 48000, 16000, 1))
    write_flac(tmp_path/'a.flac', x, 16000)
    with open(tmp_path/'a.flac', 'rb') as f:
        assert f.read() == flac_bytes(x, 16000)
