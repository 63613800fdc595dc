"""Octave-band walls and the spherical-head ear on the host: the filter bank and the head's low-pass of
brever_amd/rir.py, the fp64 restatement of tests/rir_bands_ref.py against closed forms, the band tables that
libbrever_rir.so builds on the host, summed image by image in NumPy, against that restatement, the refusals of the new
entry points, and `random_rooms` with bands. No GPU."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import rir_bands_ref as B
from brever_amd import rir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAD, C0 = 0.0875, 343.0
BETA6 = (0.8, 0.7, 0.6, 0.75, 0.5, 0.65)


def _beta(K, tilt=0.93):
    """Six different walls, different in every band."""
    return np.array([[b*tilt**k*(1.0 - 0.02*((k + w) % 3)) for w, b in enumerate(BETA6)] for k in range(K)])


# -- the filter bank ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fs', [16000, 48000])
@pytest.mark.parametrize('K', [1, 3, 6, 8])
def test_the_band_filters_sum_to_the_impulse(fs, K):
    if 125*2**(K - 1) >= fs/2:
        with pytest.raises(ValueError, match='below fs/2'):
            rir.band_filter_bank(fs, K)
        return
    g = rir.band_filter_bank(fs, K)
    N = {16000: 256, 48000: 1024}[fs]
    assert g.shape == (K, N) and rir.default_band_taps(fs) == N
    impulse = np.zeros(N)
    impulse[N//2] = 1.0
    err, against = np.abs(g.sum(axis=0) - impulse).max(), np.abs(g - B.bank(fs, K)).max()
    print(f'fs {fs} K {K}: |sum g_k - impulse| {err:.2e}, |g - restatement| {against:.2e}')
    assert err <= 1e-15 and against <= 1e-15
    if K == 1:
        assert np.array_equal(g[0], impulse)
    else:
        assert all(np.abs(g[k]).max() > 1e-3 for k in range(K))


def test_a_last_band_at_or_above_half_the_sample_rate_is_refused():
    with pytest.raises(ValueError, match='below fs/2'):
        rir.band_filter_bank(16000, 7)                   # 8 kHz = fs/2
    assert rir.band_filter_bank(16000.5, 7).shape == (7, 512)
    with pytest.raises(ValueError, match='bands'):
        rir.band_filter_bank(48000, 9)


@pytest.mark.parametrize('fs,taps', [(16000, 56), (48000, 170)])
def test_the_head_lowpass(fs, taps):
    lp = rir.head_lowpass(fs, RAD, C0)
    kk = fs*RAD/C0
    assert len(lp) == taps == math.ceil(40*math.log(2)/-math.log(abs((1 - kk)/(1 + kk))))
    longer = B.lowpass(fs, RAD, C0, taps=4*taps)         # the recurrence itself, run on
    cut = np.abs(longer[taps:]).max()
    print(f'fs {fs}: {taps} taps, largest coefficient cut off {cut:.2e} = 2^{math.log2(cut):.1f}, '
          f'DC gain - 1 {lp.sum() - 1:.2e}')
    assert np.abs(lp - longer[:taps]).max() <= 1e-16 and cut < 2.0**-40 and abs(lp.sum() - 1.0) <= 1e-12


def test_the_channel_filters_of_both_modes():
    f, pad = rir.band_filters(16000, 6, 'pattern')
    assert f.shape == (6, 256) and pad == 128 and not f.flags.writeable
    assert rir.band_filters(16000, 6, 'pattern', head_radius=0.1)[0] is f          # cached: no head, no radius
    s, pad = rir.band_filters(16000, 6, 'sphere', RAD)
    assert s.shape == (12, 320) and pad == 128 and s.shape[1] % rir.FILTER_MULTIPLE == 0
    ref = B.channel_filters(16000, 6, True, RAD)
    for c in range(12):
        assert np.abs(s[c, :len(ref[c])] - ref[c]).max() <= 1e-15 and not s[c, len(ref[c]):].any()
    assert rir.band_filters(16000, 6, 'sphere', 0.09)[0] is not s


# -- the restatement against closed forms ---------------------------------------------------------------------------
def _one_image(angle, ear, d=1.25, fs=16000, taps=200):
    """Anechoic, one band, sphere mode: ``(channel rows, delay in samples)`` of ear 0 (left) or 1 (right)."""
    head = (2.0, 1.5, 1.2)
    source, _, sides = B.head_geometry(head, 0.0, angle, d, RAD)
    count = []
    x = B.channels((4.0, 3.0, 2.5), np.zeros((1, 6)), source, head, sides[ear], 0.75, taps, fs, True, RAD, window=64,
                   N=2, count=count)
    assert count == [1]
    return x


def test_a_source_on_the_ear_axis_and_one_opposite():
    fs, d = 16000, 1.25
    spread = 1.0/(4*math.pi*d)
    t = np.arange(201)
    for angle, ear, excess, gains in ((90.0, 0, -RAD, (2.0, -1.0)), (-90.0, 0, RAD*math.pi/2, None),
                                      (-90.0, 1, -RAD, (2.0, -1.0)), (90.0, 1, RAD*math.pi/2, None)):
        x = _one_image(angle, ear, d, fs)
        tau = (d + excess)*fs/C0
        u = t - tau
        pulse = np.where(np.abs(u) < 32, np.sinc(u)*(1 + np.cos(2*np.pi*u/64))/2, 0.0)
        if gains is None:                                # theta = pi: alpha = 1.05 + 0.95 cos(216 degrees)
            alpha = 1.05 + 0.95*math.cos(math.radians(216.0))
            gains = (alpha, 1.0 - alpha)
        err = max(np.abs(x[k] - gains[k]*spread*pulse).max() for k in range(2))
        print(f'angle {angle} ear {ear}: delay {tau:.4f} samples, gains {gains}, |x - closed form| {err:.2e}')
        assert err < 1e-15 and np.abs(x[0]).max() > 1e-2


def test_left_and_right_swap_under_mirroring():
    dims, head, beta = (4.0, 3.0, 2.5), (1.5, 1.5, 1.3), _beta(3)
    beta[:, 2] = beta[:, 3]                              # the walls that the median plane y = Ly/2 separates
    a = B.brir(dims, beta, head, 0.0, 35.0, 1.2, 300, 16000, True, window=48)
    b = B.brir(dims, beta, head, 0.0, -35.0, 1.2, 300, 16000, True, window=48)
    print(f'mirroring: peak {np.abs(a).max():.3e}, |left(+35) - right(-35)| {np.abs(a[:, 0] - b[:, 1]).max():.2e}')
    assert np.abs(a).max() > 1e-2 and np.abs(a[:, 0] - a[:, 1]).max() > 1e-3
    assert np.abs(a[:, 0] - b[:, 1]).max() < 1e-12 and np.abs(a[:, 1] - b[:, 0]).max() < 1e-12


def test_equal_bands_give_the_single_band_response():
    import rir_ref as R
    args = ((3.2, 2.6, 2.4), (0.9, 1.7, 1.1), (2.4, 0.8, 1.6), (0.6, 0.8, 0.0))
    one = R.rir(args[0], BETA6, args[1], args[2], args[3], 0.75, 200, 16000, window=48)
    six = B.rir(args[0], [BETA6]*6, args[1], args[2], args[3], 0.75, 200, 16000, window=48)
    print(f'equal bands: peak {np.abs(one).max():.3e}, difference {np.abs(one - six).max():.2e}')
    assert np.abs(one - six).max() < 1e-15


# -- the host tables against the restatement ----------------------------------------------------------------------
def _batch(K=3, mode='pattern', beta=None, **over):
    g = dict(L=(3.2, 2.6, 2.4), s=(0.9, 1.7, 1.1), r=(2.4, 0.8, 1.6), o=(0.6, 0.8, 0.0), a=0.75)
    h = dict(taps=200, out_offset=0, out_stride=1)
    opts = dict(fs=16000.0, c=343.0, W=48.0, K=float(K), mode=float(rir.EAR_MODELS.get(mode, mode)), rad=RAD,
                pad=128.0)
    for d in (g, h, opts):
        d.update({k: v for k, v in over.items() if k in d})
    beta = _beta(int(K) if 1 <= K <= 8 else 1) if beta is None else np.asarray(beta, dtype=np.float64)
    geom = np.zeros((1, rir.BANDS_GEOM_DOUBLES))
    geom[0, :13] = np.concatenate([np.ravel(v) for v in g.values()])
    geom[0, 13:13 + beta.size] = beta.ravel()
    return geom, np.array([list(h.values())], dtype=np.int64), np.array(list(opts.values())), beta


def _sum_tables(rows, ix, opts, max_order):
    """The channel rows of one job from its tables: every (x, y, z) triple, one at a time."""
    fs, c, W, K, mode, rad, pad = opts
    K, sphere = int(K), int(mode) == rir.SPHERE
    hdr, nx, ny, nz, taps = (int(v) for v in ix[:5])
    o, a = rows[hdr, :3], rows[hdr, 3]
    tx, ty, tz = rows[hdr + 1:hdr + 1 + nx], rows[hdr + 1 + nx:hdr + 1 + nx + ny], \
        rows[hdr + 1 + nx + ny:hdr + 1 + nx + ny + nz]
    T = taps + int(pad)
    x, t = np.zeros((2*K if sphere else K, T)), np.arange(T)
    for rx in tx:
        for ry in ty:
            for rz in tz:
                if max_order >= 0 and rx[1] + ry[1] + rz[1] > max_order:
                    continue
                d = math.sqrt(rx[2] + ry[2] + rz[2])
                cosang = (rx[0]*o[0] + ry[0]*o[1] + rz[0]*o[2])/d
                A = rx[3:]*ry[3:]*rz[3:]
                if sphere:
                    alpha, delta = B.head_terms(cosang, rad)
                    tau, amps = (d + delta)*fs/c, np.concatenate([A*alpha, A*(1 - alpha)])/(4*math.pi*d)
                else:
                    tau, amps = d*fs/c, A*(a + (1 - a)*cosang)/(4*math.pi*d)
                u = t - tau
                m = np.abs(u) < W/2
                x[:, m] += amps[:, None]*(np.sinc(u[m])*(1 + np.cos(2*math.pi*u[m]/W))/2)[None, :]
    return x


def _tables(geom, shape, opts, max_order=-1):
    n = rir.bands_query('brv_rir_bands_table_rows', geom.ctypes.data, shape.ctypes.data, len(geom), opts.ctypes.data,
                        max_order)
    rows = np.full((n, 3 + int(opts[3])), np.nan)
    index = np.full((len(geom), rir.INDEX_WORDS), -7, dtype=np.int64)
    rir.bands_call('brv_rir_bands_build_tables', geom.ctypes.data, shape.ctypes.data, len(geom), opts.ctypes.data,
                   max_order, rows.ctypes.data, index.ctypes.data, n)
    return rows, index


@pytest.mark.parametrize('mode,max_order', [('pattern', -1), ('sphere', -1), ('sphere', 2)])
def test_the_band_tables_hold_the_images_of_the_restatement(mode, max_order):
    geom, shape, opts, beta = _batch(3, mode, taps=200, pad=32.0)
    rows, index = _tables(geom, shape, opts, max_order)
    assert np.isfinite(rows).all() and index[0].tolist()[:1] == [0] and index[0, 4:].tolist() == [200, 0, 1, 0]
    assert rows[0].tolist() == [0.6, 0.8, 0.0, 0.75, 0.0, 0.0]
    at = 1
    for k in range(3):
        table = rows[at:at + index[0, 1 + k]]
        at += index[0, 1 + k]
        assert np.all(np.diff(table[:, 2]) >= 0) and np.array_equal(table[:, 2], table[:, 0]**2)
        assert np.all(table[:, 3:] > 0) and np.all(table[:, 3:] <= 1) and np.all(table[:, 1] == np.round(table[:, 1]))
    assert at == len(rows)
    g = geom[0]
    ref = B.channels(g[0:3], beta, g[3:6], g[6:9], g[9:12], g[12], 200, 16000, mode == 'sphere', RAD, window=48,
                     max_order=max_order, N=64)
    got = _sum_tables(rows, index[0], opts, max_order)
    print(f'{mode} max_order {max_order}: {len(rows) - 1} rows, peak {np.abs(ref).max():.3e}, tables - restatement '
          f'{np.abs(got - ref).max():.2e}')
    assert got.shape == ref.shape and np.abs(ref).max() > 1e-2 and np.abs(got - ref).max() < 1e-13


def test_a_wall_dead_in_one_band_keeps_its_rows_and_dead_in_all_drops_them():
    live = _tables(*_batch(3)[:3])[1]
    one = _beta(3)
    one[1, 1] = 0.0
    rows, index = _tables(*_batch(3, beta=one)[:3])
    assert index[0, 1:4].tolist() == live[0, 1:4].tolist()
    x_rows = rows[1:1 + index[0, 1]]
    assert (x_rows[:, 4] == 0).any() and np.all(x_rows[:, [3, 5]] > 0)
    every = _beta(3)
    every[:, 1] = 0.0
    dropped = _tables(*_batch(3, beta=every)[:3])[1]
    assert dropped[0, 1] < live[0, 1] and dropped[0, 2:4].tolist() == live[0, 2:4].tolist()
    # the scratch offsets of a batch: C (taps + pad) doubles per job
    geom, shape, opts, _ = _batch(3, 'sphere')
    geom, shape = np.tile(geom, (3, 1)), np.tile(shape, (3, 1))
    shape[:, 0] = (200, 50, 77)
    assert _tables(geom, shape, opts)[1][:, 7].tolist() == [0, 6*328, 6*(328 + 178)]


# -- the C ABI ---------------------------------------------------------------------------------------------------
NEW = {'brv_rir_bands_table_rows', 'brv_rir_bands_build_tables', 'brv_rir_bands_channels', 'brv_rir_bands_combine'}


def test_the_band_header_parses_and_every_export_resolves():
    assert os.path.samefile(rir._BANDS.header_path, os.path.join(ROOT, 'include', 'rir', 'brever_rir_bands.h'))
    assert rir._BANDS.path == rir.LIB_PATH
    assert set(rir._BANDS.signatures) == NEW | {'brv_rir_last_error'} and rir._BANDS.structs == {}
    lib = rir._BANDS.lib()
    for name, (restype, argtypes) in rir._BANDS.signatures.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert rir._BANDS.constants == {
        'BRV_RIR_BANDS_MAX_BANDS': 8, 'BRV_RIR_BANDS_GEOM_DOUBLES': 61, 'BRV_RIR_BANDS_OPT_DOUBLES': 7,
        'BRV_RIR_BANDS_PATTERN': 0, 'BRV_RIR_BANDS_SPHERE': 1, 'BRV_RIR_BANDS_MAX_FILTER': 2048,
        'BRV_RIR_BANDS_COMBINE_TILE': 1024}
    with open(rir.HEADER_PATH) as f:
        assert 'brv_rir_bands' not in f.read()           # the first header is as it was


def _refused(fn, args, word):
    status = fn(*args)
    msg = rir._BANDS.lib().brv_rir_last_error()
    assert status == -1 and msg and word.encode() in msg, (status, msg, word)


def test_the_new_refusals_carry_a_message():
    lib = rir._BANDS.lib()
    buf = ctypes.create_string_buffer(4096)              # stands for the outputs: every call below is refused first
    ptr = lambda a: a.ctypes.data                                                       # noqa: E731

    def both(word, K=3, mode='pattern', beta=None, **over):
        geom, shape, opts, _ = _batch(K, mode, beta, **over)
        _refused(lib.brv_rir_bands_table_rows, (ptr(geom), ptr(shape), 1, ptr(opts), -1), word)
        _refused(lib.brv_rir_bands_build_tables, (ptr(geom), ptr(shape), 1, ptr(opts), -1, buf, buf, 100), word)

    geom, shape, opts, _ = _batch()
    assert lib.brv_rir_bands_table_rows(ptr(geom), ptr(shape), 1, ptr(opts), -1) > 3
    both('1 <= K <= 8', K=0)
    both('1 <= K <= 8', K=9)
    both('1 <= K <= 8', K=2.5)
    both('below fs/2', K=7)                              # 8 kHz at fs 16 kHz
    bad = _beta(3)
    bad[2, 4] = 1.01
    both('beta in [0, 1]', beta=bad)
    bad[2, 4] = -0.01
    both('beta in [0, 1]', beta=bad)
    bad[2, 4] = float('nan')
    both('beta in [0, 1]', beta=bad)
    both('ear model', mode=2)
    both('ear model', mode=-1)
    both('inside the sphere', mode='sphere', s=(2.4 + 0.05, 0.8 + 0.05, 1.6))
    both('head radius', mode='sphere', rad=0.0)
    both('head reaches a wall', mode='sphere', r=(3.2 - 0.05, 0.8, 1.6))
    both('pad', pad=1025.0)
    both('source', s=(0.0, 1.7, 1.1))
    both('taps', taps=0)
    # a source inside the sphere's radius is no refusal in pattern mode
    g2, s2, o2, _ = _batch(s=(2.45, 0.85, 1.6))
    assert lib.brv_rir_bands_table_rows(ptr(g2), ptr(s2), 1, ptr(o2), -1) > 3
    # the launches: refused on the host before anything is launched
    chan = dict(tables=buf, index=buf, n_jobs=1, n_rows=10, max_taps=200, opts=ptr(opts), max_order=-1, scratch=buf,
                scratch_len=3*328, stream=None)
    for name, value, word in (('tables', None, 'null'), ('scratch', None, 'null'), ('n_jobs', 0, 'n_jobs'),
                              ('n_rows', 0, 'n_rows'), ('max_taps', 0, 'max_taps'), ('max_order', -2, 'max_order'),
                              ('scratch_len', 3*328 - 1, 'scratch is too small')):
        _refused(lib.brv_rir_bands_channels, list(dict(chan, **{name: value}).values()), word)
    comb = dict(scratch=buf, scratch_len=3*328, index=buf, n_jobs=1, max_taps=200, opts=ptr(opts), filters=buf,
                n_filter=256, out=buf, out_len=200, stream=None)
    for name, value, word in (('filters', None, 'null'), ('out', None, 'null'), ('n_jobs', 0, 'n_jobs'),
                              ('n_filter', 250, 'n_filter'), ('n_filter', 2064, 'n_filter'), ('out_len', 0, 'out_len'),
                              ('scratch_len', 3*328 - 1, 'scratch is too small')):
        _refused(lib.brv_rir_bands_combine, list(dict(comb, **{name: value}).values()), word)
    for k, value, word in ((3, 9.0, '1 <= K <= 8'), (4, 3.0, 'ear model'), (0, 0.0, 'fs')):
        wrong = opts.copy()
        wrong[k] = value
        _refused(lib.brv_rir_bands_channels, list(dict(chan, opts=ptr(wrong)).values()), word)
        _refused(lib.brv_rir_bands_combine, list(dict(comb, opts=ptr(wrong)).values()), word)
    with pytest.raises(RuntimeError, match='brv_rir_bands_table_rows failed with status -1: job 0: the source is '
                                           'inside the sphere'):
        g3, s3, o3, _ = _batch(3, 'sphere', s=(2.45, 0.85, 1.6))
        rir.build_band_tables(g3, s3, o3)


# -- the Python layer ----------------------------------------------------------------------------------------------
FIELDS = ('dims', 'beta', 'head', 'yaw', 'distance', 'angles', 'taps', 'ear_pattern', 'head_radius', 'rt60')


def test_random_rooms_keep_every_field_they_had():
    with open(os.path.join(ROOT, 'tests', 'golden', 'rir_random_rooms_seed3.json')) as f:
        golden = json.load(f)                            # the rooms of (5, seed 3) before the bands existed

    def same(a, b):
        return a == (tuple(b) if isinstance(b, list) else b)

    rooms = rir.random_rooms(golden['n'], golden['seed'])
    for room, was in zip(rooms, golden['rooms']):
        assert all(same(getattr(room, k), was[k]) for k in FIELDS) and room.ear_model == 'pattern'
        assert room.bands() == 0 and 'ear_model' not in repr(room)
    banded = rir.random_rooms(golden['n'], golden['seed'], bands=6, ear_model='sphere')
    tilts = np.random.default_rng([golden['seed'], 1]).uniform(0.0, 0.25, size=golden['n'])
    for room, was, u in zip(banded, golden['rooms'], tilts):
        assert all(same(getattr(room, k), was[k]) for k in FIELDS if k != 'beta')
        assert np.shape(room.beta) == (6, 6) and room.bands() == 6 and room.ear_model == 'sphere'
        floor = 1.01*rir.min_rt60(room.dims)
        for k in range(6):
            t60 = max(was['rt60']*2.0**(-u*(k - 2)), floor)
            assert room.rt60_bands[k] == t60 and set(room.beta[k]) == {rir.beta_from_rt60(room.dims, t60)}
        assert room.rt60_bands[2] == was['rt60'] and room.beta[2] == tuple(was['beta'])
        assert room.beta[0][0] >= room.beta[5][0]
    flat = rir.random_rooms(3, 1, bands=4, band_tilt=(0.0, 0.0))
    assert all(len({row for row in room.beta}) == 1 for room in flat)


def test_beta_from_rt60_takes_a_sequence_and_rooms_take_bands():
    dims = (5.0, 4.0, 3.0)
    assert rir.beta_from_rt60(dims, [0.3, 0.5]) == (rir.beta_from_rt60(dims, 0.3), rir.beta_from_rt60(dims, 0.5))
    with pytest.raises(ValueError, match='out of reach'):
        rir.beta_from_rt60(dims, [0.5, 0.01])
    room = rir.ShoeboxRoom((4, 3, 2.5), _beta(3), (2, 1.5, 1.2), 0.0, 1.0, (0,), 100, ear_model='sphere')
    assert room.bands() == 3 and np.allclose(room.beta, _beta(3), rtol=0, atol=0) and "ear_model='sphere'" in repr(room)
    with pytest.raises(ValueError, match='ear_model'):
        rir.ShoeboxRoom((4, 3, 2.5), (0.5,)*6, (2, 1.5, 1.2), 0.0, 1.0, (0,), 100, ear_model='kemar')
    with pytest.raises(ValueError, match=r'\(K, 6\)'):
        rir.ShoeboxRoom((4, 3, 2.5), np.zeros((9, 6)), (2, 1.5, 1.2), 0.0, 1.0, (0,), 100)
    with pytest.raises(RuntimeError, match='ROCm device'):
        rir.simulate_brirs([room], device='cpu')
    with pytest.raises(RuntimeError, match='ROCm device'):
        rir.simulate_rirs((4, 3, 2.5), _beta(3), [(1, 1, 1)], [(2, 2, 1)], [(1.0, 0.0, 0.0)], [1.0], 100, 16000,
                          device='cpu')
    assert rir.chunk_jobs([100, 100, 100, 100], 2, 28, 8*2*128*2) == [(0, 2), (2, 4)]
    assert rir.chunk_jobs([100, 100, 100], 2, 28, 1) == [(0, 1), (1, 2), (2, 3)]
    assert rir.chunk_jobs([100, 100, 100], 2, 28, 1 << 30) == [(0, 3)]
