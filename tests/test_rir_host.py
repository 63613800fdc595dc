"""The shoebox image-source simulator on the host: the fp64 restatement of tests/rir_ref.py against closed forms,
reciprocity and symmetry; the candidate tables that libbrever_rir.so builds on the host, summed image by image in
NumPy, against that restatement; the host helpers of brever_amd/rir.py; the C ABI (header, exports, refusals).
No GPU."""
import ctypes
import glob
import importlib
import math
import os

import numpy as np
import pytest

import rir_ref as R
from brever_amd import hip, rir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, OMNI = (1.0, 0.0, 0.0), 1.0


# -- the restatement ---------------------------------------------------------------------------------------------
def test_anechoic_room_has_one_image_at_an_exact_delay():
    count = []
    h = R.rir((4.0, 3.0, 2.5), (0.0,)*6, (1.0, 1.5, 1.2), (2.25, 1.5, 1.2), X, OMNI, 128, 16384, window=64,
              c=320.0, count=count)
    assert count == [1]
    assert h[64] == 1.0/(4*math.pi*1.25)
    rest = np.delete(h, 64)
    print(f'anechoic: h[64] {h[64]:.17g}, the other taps at most {np.abs(rest).max():.2e}')
    assert np.abs(rest).max() < 1e-15


def test_reciprocity_with_omni_receivers():
    dims, beta = (3.2, 2.6, 2.4), (0.8, 0.7, 0.6, 0.75, 0.5, 0.65)
    a, b = (0.9, 1.7, 1.1), (2.4, 0.8, 1.6)
    hab = R.rir(dims, beta, a, b, X, OMNI, 400, 16000, window=48)
    hba = R.rir(dims, beta, b, a, X, OMNI, 400, 16000, window=48)
    print(f'reciprocity: peak {np.abs(hab).max():.3e}, difference {np.abs(hab - hba).max():.2e}')
    assert np.abs(hab).max() > 1e-2 and np.abs(hab - hba).max() < 1e-12


def test_a_frontal_source_in_a_symmetric_room_gives_equal_ears():
    # the median plane of the head is y = Ly/2, and the two walls it separates reflect alike
    h = R.brir((4.0, 3.0, 2.5), (0.7, 0.6, 0.65, 0.65, 0.5, 0.8), (1.5, 1.5, 1.3), 0.0, 0.0, 1.2, 400, 16000, window=48)
    print(f'symmetry: peak {np.abs(h).max():.3e}, left - right {np.abs(h[:, 0] - h[:, 1]).max():.2e}')
    assert np.abs(h).max() > 1e-2 and np.abs(h[:, 0] - h[:, 1]).max() < 1e-12
    # and a source on the left is louder in the left ear
    left = R.brir((4.0, 3.0, 2.5), (0.0,)*6, (1.5, 1.5, 1.3), 0.3, 60.0, 1.0, 200, 16000)
    assert np.abs(left[:, 0]).max() > np.abs(left[:, 1]).max()


# -- the host helpers --------------------------------------------------------------------------------------------
def test_beta_from_rt60_round_trip_and_refusal():
    dims = (5.0, 4.0, 3.0)
    V, S = 60.0, 2*(20.0 + 15.0 + 12.0)
    for rt60 in (0.2, 0.5, 1.2):
        beta = rir.beta_from_rt60(dims, rt60)
        assert 0.0 < beta < 1.0 and abs(0.161*V/(S*(1.0 - beta**2)) - rt60) < 1e-12
    assert rir.min_rt60(dims) == pytest.approx(0.161*V/S, rel=1e-15)
    for bad in (0.161*V/S, 0.05, 0.0, -1.0):
        with pytest.raises(ValueError, match='out of reach'):
            rir.beta_from_rt60(dims, bad)


def test_random_rooms_are_a_function_of_the_arguments_and_keep_the_margin():
    rooms = rir.random_rooms(200, seed=3)
    again = rir.random_rooms(200, seed=3)
    assert [repr(a) for a in rooms] == [repr(b) for b in again]
    assert repr(rir.random_rooms(1, seed=4)[0]) != repr(rooms[0])
    assert [repr(a) for a in rir.random_rooms(5, seed=3)] == [repr(a) for a in rooms[:5]]
    margin = 0.3
    for room in rooms:
        L = np.array(room.dims)
        assert np.all(L >= (3, 3, 2.4)) and np.all(L <= (10, 8, 4))
        assert room.angles == tuple(float(a) for a in range(-90, 91, 10)) and len(room.angles) == 19
        assert room.taps == math.ceil(room.rt60*16000) and 0.2 <= room.rt60 <= 0.8
        assert all(0.0 < b < 1.0 for b in room.beta) and len(set(room.beta)) == 1
        assert room.beta[0] == rir.beta_from_rt60(room.dims, room.rt60)
        assert 0.0 < room.distance <= 3.0 and 1.0 <= room.head[2] <= min(1.8, L[2] - margin)
        points = [np.array(room.head), *room.ears()] + [room.source(a) for a in room.angles]
        for p in points:
            assert np.all(p >= margin - 1e-12) and np.all(p <= L - margin + 1e-12), (room, p)
        left, right = room.ears()
        assert abs(np.linalg.norm(left - right) - 2*room.head_radius) < 1e-12
        for a in room.angles:
            assert abs(np.linalg.norm(room.source(a) - np.array(room.head)) - room.distance) < 1e-12
    assert rir.random_rooms(3, seed=0, taps=800, angles=(-30, 0, 30))[2].taps == 800
    # the geometry is that of the restatement
    room = rooms[7]
    source, ears, sides = R.head_geometry(room.head, room.yaw, 40.0, room.distance)
    assert np.allclose(source, room.source(40.0), atol=1e-15) and np.allclose(ears[0], room.ears()[0], atol=1e-15)
    assert np.allclose(ears[1], room.ears()[1], atol=1e-15) and np.allclose(sides[0], room.side(), atol=1e-15)


def test_save_pool_writes_what_the_maker_loads(tmp_path):
    from brever_amd.mixture import PoolMixtureMaker
    rng = np.random.default_rng(0)
    brirs = [[rng.standard_normal((20, 2)).astype(np.float32) for _ in range(3)],
             [rng.standard_normal((30, 2)).astype(np.float32)]]
    speech, noises = [rng.standard_normal(100), rng.standard_normal(50)], [rng.standard_normal(70)]
    path = str(tmp_path/'pool.npz')
    rir.save_pool(path, brirs, speech, noises)
    s, n, b = PoolMixtureMaker._load(path)
    assert [len(room) for room in b] == [3, 1] and all(
        np.array_equal(b[r][a], brirs[r][a]) for r in range(2) for a in range(len(brirs[r])))
    assert [x.tolist() for x in s] == [np.float32(x).tolist() for x in speech] and len(n) == 1


# -- the host tables against the restatement ----------------------------------------------------------------------
def _batch(jobs=1, **over):
    """A valid batch of ``jobs`` equal jobs as the arrays of the C ABI, with single values replaced."""
    g = dict(L=(3.2, 2.6, 2.4), beta=(0.8, 0.7, 0.6, 0.75, 0.5, 0.65), s=(0.9, 1.7, 1.1), r=(2.4, 0.8, 1.6),
             o=(0.6, 0.8, 0.0), a=0.75)
    h = dict(taps=200, out_offset=0, out_stride=1)
    opts = dict(fs=16000.0, c=343.0, W=48.0)
    for d in (g, h, opts):
        d.update({k: v for k, v in over.items() if k in d})
    geom = np.tile(np.concatenate([np.ravel(v) for v in g.values()]).astype(np.float64), (jobs, 1))
    shape = np.tile(np.array(list(h.values()), dtype=np.int64), (jobs, 1))
    shape[:, 1] += np.arange(jobs)*h['taps']*h['out_stride']
    return geom, shape, np.array(list(opts.values()), dtype=np.float64)


def _tables(geom, shape, opts, max_order=-1):
    n = rir.query('brv_rir_table_rows', geom.ctypes.data, shape.ctypes.data, len(geom), opts.ctypes.data, max_order)
    rows, index = np.full((n, rir.ROW_DOUBLES), np.nan), np.full((len(geom), rir.INDEX_WORDS), -7, dtype=np.int64)
    rir.call('brv_rir_build_tables', geom.ctypes.data, shape.ctypes.data, len(geom), opts.ctypes.data, max_order,
             rows.ctypes.data, index.ctypes.data, n)
    return rows, index


def _sum_tables(rows, ix, opts, max_order):
    """The response of one job from its tables: every (x, y, z) triple, one at a time."""
    fs, c, W = opts
    hdr, nx, ny, nz, taps = (int(v) for v in ix[:5])
    o, a = rows[hdr, :3], rows[hdr, 3]
    tx, ty, tz = rows[hdr + 1:hdr + 1 + nx], rows[hdr + 1 + nx:hdr + 1 + nx + ny], \
        rows[hdr + 1 + nx + ny:hdr + 1 + nx + ny + nz]
    h, t = np.zeros(taps), np.arange(taps)
    for x in tx:
        for y in ty:
            for z in tz:
                if max_order >= 0 and x[2] + y[2] + z[2] > max_order:
                    continue
                d = math.sqrt(x[3] + y[3] + z[3])
                u = t - d*fs/c
                m = np.abs(u) < W/2
                g = a + (1 - a)*(x[0]*o[0] + y[0]*o[1] + z[0]*o[2])/d
                h[m] += x[1]*y[1]*z[1]*g/(4*math.pi*d)*np.sinc(u[m])*(1 + np.cos(2*math.pi*u[m]/W))/2
    return h


@pytest.mark.parametrize('max_order,beta', [(-1, None), (2, None), (-1, (0.8, 0.0, 0.6, 0.75, 0.0, 0.65))])
def test_the_tables_hold_the_images_of_the_restatement(max_order, beta):
    over = {} if beta is None else dict(beta=beta)
    geom, shape, opts = _batch(2, **over)
    geom[1, 12:15] = (1.0, 1.9, 0.7)                                  # another receiver for the second job
    rows, index = _tables(geom, shape, opts, max_order)
    assert np.isfinite(rows).all() and index[0, 0] == 0 and index[1, 0] == 1 + index[0, 1:4].sum()
    assert index[:, 4].tolist() == [200, 200] and index[:, 5].tolist() == [0, 200] and index[:, 6:].tolist() == [[1, 0]]*2
    for j in range(2):
        hdr, counts = index[j, 0], index[j, 1:4]
        assert rows[hdr].tolist() == [0.6, 0.8, 0.0, 0.75] and np.all(counts >= 1) and np.all(counts <= rir.MAX_AXIS_ROWS)
        at = hdr + 1
        for k in range(3):
            table = rows[at:at + counts[k]]
            at += counts[k]
            assert np.all(np.diff(table[:, 3]) >= 0) and np.array_equal(table[:, 3], table[:, 0]**2)
            assert np.all(table[:, 1] > 0) and np.all(table[:, 1] <= 1) and np.all(table[:, 2] == np.round(table[:, 2]))
            if max_order >= 0:
                assert table[:, 2].max() <= max_order
        g = geom[j]
        ref = R.rir(g[0:3], g[3:9], g[9:12], g[12:15], g[15:18], g[18], 200, 16000, window=48, max_order=max_order)
        got = _sum_tables(rows, index[j], opts, max_order)
        print(f'job {j} max_order {max_order}: peak {np.abs(ref).max():.3e}, tables - restatement '
              f'{np.abs(got - ref).max():.2e}')
        assert np.abs(ref).max() > 1e-2 and np.abs(got - ref).max() < 1e-13


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_rir_version', 'brv_rir_last_error', 'brv_rir_table_rows', 'brv_rir_build_tables', 'brv_rir_simulate'}


def test_header_parses_and_every_export_resolves():
    assert os.path.samefile(rir.HEADER_PATH, os.path.join(ROOT, 'include', 'rir', 'brever_rir.h'))
    assert rir.LIB_PATH == os.path.join(ROOT, 'brever_amd', 'csrc', 'libbrever_rir.so')
    with open(rir.HEADER_PATH) as f:
        text = f.read()
    table = hip.parse_header(text)
    assert set(table) == EXPORTS == set(rir.SIGNATURES) and hip.parse_structs(text, {}) == {}
    lib = rir.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert table['brv_rir_table_rows'][0] is ctypes.c_int64
    for name in ('brv_rir_build_tables', 'brv_rir_simulate'):
        assert table[name][0] is ctypes.c_int, name
    assert table['brv_rir_simulate'][1][-1] is hip._c_ptr and lib.brv_rir_version() >= 100
    # the limits are the header's macros, and the module's constants are those
    assert rir._LIB.constants == {
        'BRV_RIR_GEOM_DOUBLES': 19, 'BRV_RIR_SHAPE_WORDS': 3, 'BRV_RIR_OPT_DOUBLES': 3, 'BRV_RIR_ROW_DOUBLES': 4,
        'BRV_RIR_INDEX_WORDS': 8, 'BRV_RIR_TILE': 128, 'BRV_RIR_MAX_AXIS_ROWS': 1024, 'BRV_RIR_MAX_TAPS': 1 << 20,
        'BRV_RIR_MAX_JOBS': 1 << 20}
    assert (rir.GEOM_DOUBLES, rir.SHAPE_WORDS, rir.OPT_DOUBLES, rir.ROW_DOUBLES, rir.INDEX_WORDS, rir.TILE,
            rir.MAX_AXIS_ROWS, rir.MAX_TAPS, rir.MAX_JOBS) == tuple(rir._LIB.constants.values())
    # a library of its own: nothing of it is declared in, or exported by, another
    entry = importlib.import_module('__graft_entry__')
    assert ('rir', 'lib', 'brv_rir_version') in entry.LIBRARIES
    for module, loader, version in entry.LIBRARIES:
        if module != 'rir':
            other = getattr(importlib.import_module('brever_amd.' + module), loader)()
            assert not any(hasattr(other, name) for name in EXPORTS), module
    headers = glob.glob(os.path.join(ROOT, 'include', '*.h'))
    assert headers
    for header in headers:
        with open(header) as f:
            assert 'brv_rir_' not in f.read(), header


def _refused(fn, args, word):
    status = fn(*args)
    msg = rir.lib().brv_rir_last_error()
    assert status == -1 and msg and word.encode() in msg, (status, msg, word)


def test_refusals_carry_a_message():
    lib = rir.lib()
    buf = ctypes.create_string_buffer(4096)           # stands for the outputs: every call below is refused first
    ptr = lambda a: a.ctypes.data                                                       # noqa: E731

    def both(word, max_order=-1, jobs=1, **over):
        geom, shape, opts = _batch(jobs, **over)
        _refused(lib.brv_rir_table_rows, (ptr(geom), ptr(shape), jobs, ptr(opts), max_order), word)
        _refused(lib.brv_rir_build_tables, (ptr(geom), ptr(shape), jobs, ptr(opts), max_order, buf, buf, 100), word)

    geom, shape, opts = _batch()
    good = (ptr(geom), ptr(shape), 1, ptr(opts), -1)
    n = lib.brv_rir_table_rows(*good)
    assert n > 3
    # nulls and zero counts
    for i, name in enumerate(('geom', 'shape', None, 'opts')):
        if name:
            bad = list(good)
            bad[i] = None
            _refused(lib.brv_rir_table_rows, bad, 'null')
            _refused(lib.brv_rir_build_tables, bad + [buf, buf, n], 'null')
            assert name.encode() in lib.brv_rir_last_error()
    for i in (5, 6):
        args = list(good) + [buf, buf, n]
        args[i] = None
        _refused(lib.brv_rir_build_tables, args, 'null')
    for jobs in (0, -1, rir.MAX_JOBS + 1):
        _refused(lib.brv_rir_table_rows, (ptr(geom), ptr(shape), jobs, ptr(opts), -1), 'n_jobs')
    for wrong in (0, n - 1, n + 1):
        _refused(lib.brv_rir_build_tables, list(good) + [buf, buf, wrong], 'n_rows')
    # the values of the model
    both('source', s=(0.0, 1.7, 1.1))
    both('source', s=(0.9, 2.6, 1.1))
    both('source', s=(0.9, 1.7, -0.1))
    both('source', s=(float('nan'), 1.7, 1.1))
    both('receiver', r=(3.2, 0.8, 1.6))
    both('receiver', r=(2.4, 0.8, 2.5))
    both('direct path', r=(0.9, 1.7, 1.1 + 5e-4))
    both('beta', beta=(0.8, 0.7, 0.6, 0.75, 0.5, 1.01))
    both('beta', beta=(-0.01, 0.7, 0.6, 0.75, 0.5, 0.65))
    both('beta', beta=(0.8, float('nan'), 0.6, 0.75, 0.5, 0.65))
    both('taps', taps=0)
    both('taps', taps=-5)
    both('taps', taps=rir.MAX_TAPS + 1)
    both('W', W=1.99)
    both('W', W=float('nan'))
    both('fs', fs=0.0)
    both('fs', c=-343.0)
    both('fs', c=float('inf'))
    both('dimensions', L=(3.2, 0.0, 2.4))
    both('orientation', o=(0.6, 0.6, 0.0))
    both('pattern', a=1.5)
    both('out_offset', out_offset=-1)
    both('out_stride', out_stride=0)
    both('max_order', max_order=-2)
    # the second job of a batch is checked like the first, and named
    geom2, shape2, _ = _batch(2)
    geom2[1, 9] = 5.0
    _refused(lib.brv_rir_table_rows, (ptr(geom2), ptr(shape2), 2, ptr(opts), -1), 'job 1: the source')
    # table sizes over the header's limit: 1 s at 48 kHz in a 1 m cube is 686 candidates per axis and fits,
    # 2 s does not
    small = dict(L=(1.0, 1.0, 1.0), s=(0.3, 0.4, 0.5), r=(0.6, 0.5, 0.4), fs=48000.0)
    g3, s3, o3 = _batch(taps=48000, **small)
    assert lib.brv_rir_table_rows(ptr(g3), ptr(s3), 1, ptr(o3), -1) > 3*600
    both('BRV_RIR_MAX_AXIS_ROWS', taps=96000, **small)
    # the launch: refused before anything is launched
    sim = dict(tables=buf, index=buf, n_jobs=1, n_rows=n, max_taps=200, opts=ptr(opts), max_order=-1, out=buf,
               out_len=200, stream=None)
    for name, value, word in (('tables', None, 'null'), ('index', None, 'null'), ('opts', None, 'null'),
                              ('out', None, 'null'), ('n_jobs', 0, 'n_jobs'), ('n_jobs', rir.MAX_JOBS + 1, 'n_jobs'),
                              ('n_rows', 0, 'n_rows'), ('max_taps', 0, 'max_taps'),
                              ('max_taps', rir.MAX_TAPS + 1, 'max_taps'), ('out_len', 0, 'out_len'),
                              ('max_order', -2, 'max_order')):
        _refused(lib.brv_rir_simulate, list(dict(sim, **{name: value}).values()), word)
    for k, value, word in ((0, 0.0, 'fs'), (1, float('nan'), 'fs'), (2, 1.5, 'W')):
        bad = opts.copy()
        bad[k] = value
        _refused(lib.brv_rir_simulate, list(dict(sim, opts=ptr(bad)).values()), word)
    with pytest.raises(RuntimeError, match='brv_rir_table_rows failed with status -1: job 0: requires beta'):
        rir.query('brv_rir_table_rows', *_ptrs(_batch(beta=(2.0,)*6)), -1)


def _ptrs(batch):
    geom, shape, opts = batch
    _ptrs.keep = batch                                # the arrays outlive the call
    return geom.ctypes.data, shape.ctypes.data, len(geom), opts.ctypes.data


def test_python_refuses_a_cpu_device_and_ragged_arguments():
    room = rir.ShoeboxRoom((4, 3, 2.5), (0.5,)*6, (2, 1.5, 1.2), 0.0, 1.0, (0,), 100)
    with pytest.raises(RuntimeError, match='ROCm device'):
        rir.simulate_brirs([room], device='cpu')
    with pytest.raises(RuntimeError, match='ROCm device'):
        rir.simulate_rirs((4, 3, 2.5), (0.5,)*6, [(1, 1, 1)], [(2, 2, 1)], [X], [1.0], 100, 16000, device='cpu')
    with pytest.raises(ValueError, match='per receiver'):
        rir.simulate_rirs((4, 3, 2.5), (0.5,)*6, [(1, 1, 1)], [(2, 2, 1)], [X, X], [1.0], 100, 16000)
    with pytest.raises(ValueError, match='3 values'):
        rir.ShoeboxRoom((4, 3), (0.5,)*6, (2, 1.5, 1.2), 0.0, 1.0, (0,), 100)
    assert rir.simulate_brirs([]) == []
