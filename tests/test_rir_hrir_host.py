"""The measured ear without a GPU (brever_amd/rir.py, include/rir/brever_rir_hrir.h): the ``HrirSet``
and its files, SOFA through ``h5lite``, the argument checks of the rooms, the host table entry points, and the
restatement tests/rir_hrir_ref.py against tests/rir_bands_ref.py."""
import json
import math
import os
import re

import numpy as np
import pytest

import rir_bands_ref as B
import rir_hrir_ref as H
from brever_amd import h5lite, rir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA6 = (0.8, 0.7, 0.6, 0.75, 0.5, 0.65)


def _set(taps=24, seed=1, fs=16000):
    az, el = H.fixture_grid()
    return rir.HrirSet.from_angles(az, el, H.fixture_hrirs(len(az), taps, seed), fs)


# -- the set -----------------------------------------------------------------------------------------------------
def test_from_angles_is_x_front_y_left_z_up():
    s = rir.HrirSet.from_angles([0, 90, 180, 270, 0, 0, 30], [0, 0, 0, 0, 90, -90, 45], np.ones((7, 2, 3)), 44100)
    want = [(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
            (math.cos(math.pi/4)*math.cos(math.pi/6), math.cos(math.pi/4)*math.sin(math.pi/6), math.sin(math.pi/4))]
    assert np.abs(s.directions - np.array(want)).max() < 1e-15
    assert len(s) == 7 and s.taps == 3 and s.fs == 44100.0 and 'D=7' in repr(s)
    assert np.abs(H.unit([0, 90, 30], [0, 0, 45]) - s.directions[[0, 1, 6]]).max() < 1e-15
    az, el = H.fixture_grid()
    assert len(az) == 38 and len(np.unique(np.round(H.unit(az, el), 12), axis=0)) == 38


def test_a_set_validates_normalises_and_is_read_only():
    h = np.ones((2, 2, 4))
    s = rir.HrirSet([(2.0, 0, 0), (0, 0, -0.5)], h, 16000)
    assert s.directions.tolist() == [[1.0, 0, 0], [0, 0, -1.0]] and s.hrirs.dtype == np.float64
    h[0, 0, 0] = 5.0
    assert s.hrirs[0, 0, 0] == 1.0                                     # a copy
    with pytest.raises(ValueError):
        s.hrirs[0, 0, 0] = 2.0
    with pytest.raises(ValueError):
        s.directions[0, 0] = 2.0
    with pytest.raises(AttributeError, match='read-only'):
        s.fs = 8000
    for bad, match in (((np.ones((2, 2)), h, 16000), r'\(D, 3\)'),
                       (([(1, 0, 0)], h, 16000), r'\(D, 2, T_h\)'),
                       (([(1, 0, 0), (0, 1, 0)], np.ones((2, 3, 4)), 16000), r'\(D, 2, T_h\)'),
                       ((np.zeros((0, 3)), np.ones((0, 2, 4)), 16000), 'D <= 2048'),
                       ((np.ones((2049, 3)), np.ones((2049, 2, 1)), 16000), 'D <= 2048'),
                       (([(1, 0, 0), (0, 1, 0)], np.ones((2, 2, 513)), 16000), 'T_h <= 512'),
                       (([(1, 0, 0), (0, 1, 0)], np.ones((2, 2, 0)), 16000), 'T_h <= 512'),
                       (([(1, 0, 0), (0, math.nan, 0)], h, 16000), 'finite'),
                       (([(1, 0, 0), (0, 1, 0)], h*math.inf, 16000), 'finite'),
                       (([(1, 0, 0), (0, 0, 0)], h, 16000), 'direction 1 has zero length'),
                       (([(1, 0, 0), (0, 1, 0)], h, 0), 'fs'),
                       (([(1, 0, 0), (0, 1, 0)], h, math.nan), 'fs')):
        with pytest.raises(ValueError, match=match):
            rir.HrirSet(*bad)
    with pytest.raises(ValueError, match='one azimuth and one elevation'):
        rir.HrirSet.from_angles([0, 1], [0], h, 16000)
    assert s.resample(16000) is s                                      # (no device is touched)


def test_npz_round_trip(tmp_path):
    s = _set()
    s.save(str(tmp_path/'set.npz'))
    t = rir.load_hrirs(str(tmp_path/'set.npz'))
    assert np.array_equal(t.directions, s.directions) and np.array_equal(t.hrirs, s.hrirs) and t.fs == s.fs
    np.savez(str(tmp_path/'other.npz'), directions=s.directions, fs=16000.0)
    with pytest.raises(ValueError, match="'hrirs'"):
        rir.load_hrirs(str(tmp_path/'other.npz'))


# -- SOFA --------------------------------------------------------------------------------------------------------
def _write_sofa(path, position, kind, ir, fs=44100.0, convention='SimpleFreeFieldHRIR', data_type='FIR',
                variable=False):
    with h5lite.File(str(path), 'w') as f:
        f.write_array('Data.IR', ir)
        f.write_array('Data.SamplingRate', [fs])
        f.write_array('SourcePosition', position)
        f.write_attr('/', 'Conventions', 'SOFA', variable)
        f.write_attr('/', 'SOFAConventions', convention, variable)
        f.write_attr('/', 'DataType', data_type, variable)
        f.write_attr('SourcePosition', 'Type', kind, variable)
        f.write_attr('SourcePosition', 'Units', 'degree, degree, metre' if kind == 'spherical' else 'metre', variable)


needs_hdf5 = pytest.mark.skipif(not h5lite.available(), reason='libhdf5 / libhdf5_hl cannot be loaded here')


@needs_hdf5
def test_sofa_round_trip_spherical_and_cartesian(tmp_path):
    az, el = H.fixture_grid()
    ir = H.fixture_hrirs(38, 40, 2)
    want = rir.HrirSet.from_angles(az, el, ir, 44100)
    _write_sofa(tmp_path/'s.sofa', np.stack([az, el, np.full(38, 1.2)], axis=1), 'spherical', ir)
    _write_sofa(tmp_path/'c.sofa', 1.2*H.unit(az, el), 'cartesian', ir, variable=True)
    with h5lite.File(str(tmp_path/'s.sofa'), 'r') as f:
        assert f.read_attr('/', 'SOFAConventions') == 'SimpleFreeFieldHRIR' and f.read_attr('/', 'nothing') is None
        assert f.read_attr('SourcePosition', 'Type') == 'spherical' and f.read_attr('Nothing', 'Type') is None
        assert f.read_array('Data.IR').shape == (38, 2, 40)
    for name in ('s.sofa', 'c.sofa'):
        got = rir.load_hrirs(str(tmp_path/name))                       # by its suffix
        assert isinstance(got, rir.HrirSet) and got.fs == 44100.0 and np.array_equal(got.hrirs, ir)
        assert np.abs(got.directions - want.directions).max() < 1e-15, name
    assert np.array_equal(rir.load_sofa(str(tmp_path/'s.sofa')).directions, want.directions)


@needs_hdf5
def test_sofa_files_that_are_refused_name_the_field(tmp_path):
    az, el = H.fixture_grid()
    pos, ir = np.stack([az, el, np.ones(38)], axis=1), H.fixture_hrirs(38, 8, 2)
    _write_sofa(tmp_path/'a.sofa', pos, 'spherical', ir, convention='SimpleFreeFieldSOS')
    with pytest.raises(ValueError, match="SOFAConventions is 'SimpleFreeFieldSOS'"):
        rir.load_sofa(str(tmp_path/'a.sofa'))
    _write_sofa(tmp_path/'b.sofa', pos, 'spherical', ir, data_type='TF')
    with pytest.raises(ValueError, match="DataType is 'TF'"):
        rir.load_sofa(str(tmp_path/'b.sofa'))
    _write_sofa(tmp_path/'c.sofa', pos, 'spherical', np.ones((38, 1, 8)))
    with pytest.raises(ValueError, match=r'Data\.IR .*R = 2'):
        rir.load_sofa(str(tmp_path/'c.sofa'))
    _write_sofa(tmp_path/'d.sofa', pos, 'polar', ir)
    with pytest.raises(ValueError, match="SourcePosition Type is 'polar'"):
        rir.load_sofa(str(tmp_path/'d.sofa'))
    _write_sofa(tmp_path/'e.sofa', pos[:5], 'spherical', ir)
    with pytest.raises(ValueError, match='SourcePosition is'):
        rir.load_sofa(str(tmp_path/'e.sofa'))
    with h5lite.File(str(tmp_path/'f.sofa'), 'w') as f:
        f.write_array('Data.IR', ir)
    with pytest.raises(ValueError, match='SOFAConventions is None'):
        rir.load_sofa(str(tmp_path/'f.sofa'))


def test_load_sofa_without_the_hdf5_library(monkeypatch, tmp_path):
    monkeypatch.setattr(h5lite, 'available', lambda: False)
    with pytest.raises(RuntimeError, match='HDF5'):
        rir.load_sofa(str(tmp_path/'x.sofa'))


# -- rooms -------------------------------------------------------------------------------------------------------
def test_room_arguments():
    s = _set()
    args = ((4, 3, 2.5), BETA6, (2, 1.5, 1.2), 0.3, 1.0, (0,), 100)
    room = rir.ShoeboxRoom(*args, ear_model='hrir', hrirs=s)
    assert room.ear_model == 'hrir' and room.hrirs is s and room.bands() == 0
    assert "ear_model='hrir'" in repr(room) and 'HrirSet(D=38' in repr(room)
    assert np.allclose(room.front(), (math.cos(0.3), math.sin(0.3), 0.0), rtol=0, atol=0)
    assert abs(room.front() @ room.side()) < 1e-17
    with pytest.raises(ValueError, match='requires hrirs'):
        rir.ShoeboxRoom(*args, ear_model='hrir')
    with pytest.raises(ValueError, match='requires hrirs'):
        rir.ShoeboxRoom(*args, ear_model='hrir', hrirs=s.hrirs)
    for model in ('pattern', 'sphere'):
        with pytest.raises(ValueError, match="hrirs goes with ear_model='hrir'"):
            rir.ShoeboxRoom(*args, ear_model=model, hrirs=s)
        plain = rir.ShoeboxRoom(*args, ear_model=model)
        assert plain.hrirs is None and 'hrirs' not in repr(plain)
    with pytest.raises(ValueError, match='ear_model'):
        rir.ShoeboxRoom(*args, ear_model='kemar', hrirs=s)
    with pytest.raises(ValueError, match='simulate_brirs'):
        rir.simulate_rirs((4, 3, 2.5), BETA6, [(1, 1, 1)], [(2, 2, 1)], [(1.0, 0.0, 0.0)], [1.0], 100, 16000,
                          ear_model='hrir')
    with pytest.raises(RuntimeError, match='ROCm device'):
        rir.simulate_brirs([room], device='cpu')
    with pytest.raises(ValueError, match="hrirs goes with"):
        rir.random_rooms(1, 0, hrirs=s)
    with pytest.raises(ValueError, match='requires hrirs'):
        rir.random_rooms(1, 0, ear_model='hrir')


def test_random_rooms_draw_the_same_rooms_with_a_measured_ear():
    with open(os.path.join(ROOT, 'tests', 'golden', 'rir_random_rooms_seed3.json')) as f:
        golden = json.load(f)
    s = _set()
    fields = [k for k in golden['rooms'][0] if k != 'rt60'] if isinstance(golden.get('rooms'), list) else None
    plain = rir.random_rooms(golden['n'], golden['seed'])
    measured = rir.random_rooms(golden['n'], golden['seed'], ear_model='hrir', hrirs=s)
    banded = rir.random_rooms(golden['n'], golden['seed'], bands=6, ear_model='hrir', hrirs=s)
    same = rir.random_rooms(golden['n'], golden['seed'], bands=6)
    assert len(plain) == len(measured) == golden['n']
    for a, b, c, d in zip(plain, measured, banded, same):
        for k in ('dims', 'beta', 'head', 'yaw', 'distance', 'angles', 'taps', 'ear_pattern', 'head_radius', 'rt60'):
            assert getattr(a, k) == getattr(b, k), k
            if k != 'beta':
                assert getattr(a, k) == getattr(c, k), k
        assert c.beta == d.beta and c.rt60_bands == d.rt60_bands
        assert a.ear_model == 'pattern' and a.hrirs is None and b.hrirs is s and c.hrirs is s
    if fields:                                  # the golden of the existing keyword set, at the new keyword's default
        for room, was in zip(plain, golden['rooms']):
            for k in fields:
                got = getattr(room, k)
                assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(was[k], dtype=np.float64)), k


# -- the host table entry points ------------------------------------------------------------------------------------
def _batch(K=3, jobs=1, D=38, Th=24, **over):
    g = dict(L=(3.2, 2.6, 2.4), s=(0.9, 1.7, 1.1), r=(2.4, 0.8, 1.6), f=(0.6, 0.8, 0.0), l=(-0.8, 0.6, 0.0))
    h = dict(taps=200, out_offset=0, out_stride=2, ear_offset=1)
    opts = dict(fs=16000.0, c=343.0, W=48.0, K=float(K), pad=128.0, D=float(D), Th=float(Th))
    for d in (g, h, opts):
        d.update({k: v for k, v in over.items() if k in d})
    kk = int(K) if 1 <= K <= 8 else 1
    beta = np.array([[b*0.93**k for b in BETA6] for k in range(kk)]) if 'beta' not in over else \
        np.asarray(over['beta'], dtype=np.float64)
    geom = np.zeros((jobs, rir.HRIR_GEOM_DOUBLES))
    geom[:, :15] = np.concatenate([np.ravel(v) for v in g.values()])
    geom[:, 15:15 + beta.size] = beta.ravel()
    shape = np.array([list(h.values())]*jobs, dtype=np.int64)
    dirs = np.ascontiguousarray(over.get('dirs', H.unit(*H.fixture_grid())[:max(int(D), 1) if D == D else 1]))
    return geom, shape, np.array(list(opts.values())), dirs


def _rows(geom, shape, opts, dirs, max_order=-1):
    return rir.hrir_query('brv_rir_hrir_table_rows', geom.ctypes.data, shape.ctypes.data, len(geom), opts.ctypes.data,
                          dirs.ctypes.data, max_order)


def test_the_host_steps_refuse_each_bad_argument_with_a_message():
    assert _rows(*_batch()) > 3
    bent = H.unit(*H.fixture_grid())
    nan, zero, long_ = bent.copy(), bent.copy(), bent.copy()
    nan[5, 1], zero[7], long_[0] = math.nan, 0.0, (2.0, 0.0, 0.0)
    cases = [(dict(D=0), 'D <= 2048'), (dict(D=2049, dirs=np.tile(bent, (54, 1))), 'D <= 2048'),
             (dict(D=1.5), 'D <= 2048'), (dict(Th=0), 'T_h <= 512'), (dict(Th=513), 'T_h <= 512'),
             (dict(dirs=nan), 'direction 5 is not a finite unit vector'),
             (dict(dirs=zero), 'direction 7 is not a finite unit vector'),
             (dict(dirs=long_), 'direction 0 is not a finite unit vector'),
             (dict(s=(2.4, 0.8, 1.6)), "the source is at the head's centre"),
             (dict(f=(1.0, 0.0, 0.0)), 'at right angles'), (dict(f=(0.6, 0.7, 0.0)), 'unit front and left'),
             (dict(f=(0.0, 0.0, 1.0), l=(0.0, 1.0, 0.0)), 'upright head'),
             (dict(ear_offset=0), 'ear_offset'), (dict(out_stride=0), 'out_stride'),
             (dict(out_offset=-1), 'out_offset'),
             (dict(taps=0), 'taps'), (dict(K=0), 'K <= 8'), (dict(K=9), 'K <= 8'), (dict(K=8), 'below fs/2'),
             (dict(pad=1025.0), 'pad'), (dict(fs=0.0), 'fs > 0'), (dict(W=1.0), 'W'),
             (dict(L=(3.2, -2.6, 2.4)), 'room dimensions'), (dict(s=(0.9, 2.7, 1.1)), 'source is outside'),
             (dict(r=(3.3, 0.8, 1.6)), 'head is outside'), (dict(beta=[[1.1]*6]*3), 'beta in')]
    for over, match in cases:
        with pytest.raises(RuntimeError, match=re.escape(match)):
            _rows(*_batch(**over))
    geom, shape, opts, dirs = _batch()
    with pytest.raises(RuntimeError, match='max_order'):
        _rows(geom, shape, opts, dirs, -2)
    n = _rows(geom, shape, opts, dirs)
    rows, index, ear = np.zeros((n, 6)), np.zeros((1, 8), dtype=np.int64), np.zeros((2, 8), dtype=np.int64)
    with pytest.raises(RuntimeError, match='n_rows is not what'):
        rir.hrir_call('brv_rir_hrir_build_tables', geom.ctypes.data, shape.ctypes.data, 1, opts.ctypes.data,
                      dirs.ctypes.data, -1, rows.ctypes.data, index.ctypes.data, ear.ctypes.data, n - 1)
    with pytest.raises(RuntimeError, match='null pointer'):
        rir.hrir_call('brv_rir_hrir_build_tables', geom.ctypes.data, shape.ctypes.data, 1, opts.ctypes.data,
                      dirs.ctypes.data, -1, rows.ctypes.data, index.ctypes.data, None, n)
    with pytest.raises(RuntimeError, match='direction 7'):
        rir.build_hrir_tables(geom, shape, opts, zero)
    with pytest.raises(ValueError, match='another number of directions'):
        rir.build_hrir_tables(geom, shape, opts, bent[:5])


def test_the_index_of_a_three_job_batch_is_what_the_header_says():
    K, D, pad = 3, 38, 128
    geom, shape, opts, dirs = _batch(K, jobs=3)
    shape[:, 0] = (200, 131, 257)
    shape[:, 1] = (0, 400, 1000)
    shape[:, 2] = (2, 1, 3)
    shape[:, 3] = (1, 131, 2)
    rows, index, ear = rir.build_hrir_tables(geom, shape, opts, dirs)
    T = shape[:, 0] + pad
    assert rows.shape[1] == 3 + K
    assert index[:, 0].tolist() == [0] + np.cumsum(1 + index[:, 1:4].sum(axis=1))[:2].tolist()
    assert len(rows) == int((1 + index[:, 1:4].sum(axis=1)).sum())
    assert index[:, 4].tolist() == [200, 131, 257] and index[:, 6].tolist() == [0, 0, 0]
    assert index[:, 5].tolist() == [0, K*D*T[0], K*D*(T[0] + T[1])]               # the direction scratch
    assert index[:, 7].tolist() == [0, 2*K*T[0], 2*K*(T[0] + T[1])]                # the fold scratch
    for j in range(3):
        assert rows[index[j, 0]].tolist() == [0.6, 0.8, -0.8, 0.6, 0.0, 0.0]       # f and l
        for e in range(2):
            assert ear[2*j + e].tolist() == [0, 0, 0, 0, shape[j, 0], shape[j, 1] + e*shape[j, 3], shape[j, 2],
                                             index[j, 7] + e*K*T[j]], (j, e)
    # the axis tables are those of the band entry points in pattern mode for the same geometry
    bgeom = np.zeros((1, rir.BANDS_GEOM_DOUBLES))
    bgeom[0, :9], bgeom[0, 9:12], bgeom[0, 12], bgeom[0, 13:13 + 6*K] = geom[0, :9], (1.0, 0.0, 0.0), 1.0, \
        geom[0, 15:15 + 6*K]
    brows, bindex = rir.build_band_tables(bgeom, shape[:1, :3], rir.band_opts(16000, K, window=48, pad=pad))
    assert np.array_equal(bindex[0, 1:4], index[0, 1:4]) and np.array_equal(brows[1:], rows[1:index[1, 0]])


# -- the restatement -----------------------------------------------------------------------------------------------
def test_an_all_impulse_set_is_an_omni_receiver_at_the_heads_centre():
    az, el = H.fixture_grid()
    impulses = np.zeros((38, 2, 5))
    impulses[:, :, 0] = 1.0
    dims, head, yaw, angle, distance = (3.2, 2.6, 2.4), (1.4, 1.2, 1.3), 0.3, 25.0, 1.0
    for beta, taps in ((BETA6, 700), ([[b*0.93**k for b in BETA6] for k in range(3)], 257)):
        used = set()
        got, margins = H.brir(dims, beta, head, yaw, angle, distance, taps, 16000, H.unit(az, el), impulses,
                              window=48, used=used)
        source = np.array(head) + distance*np.array([math.cos(yaw + math.radians(angle)),
                                                     math.sin(yaw + math.radians(angle)), 0.0])
        ref = B.rir(dims, np.reshape(beta, (-1, 6)), source, head, (1.0, 0.0, 0.0), 1.0, taps, 16000, window=48)
        err = np.abs(got - ref[:, None]).max()/np.abs(ref).max()
        print(f'taps {taps}: {len(margins)} images, {len(used)} directions in use, least margin {margins.min():.2e}, '
              f'impulse set - omni receiver {err:.2e} of the peak')
        assert got.shape == (taps, 2) and np.abs(ref).max() > 1e-2 and err <= 1e-13
        assert margins.min() >= 1e-9 and len(used) >= 31
