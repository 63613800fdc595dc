"""The measured ear on the GPU (brever_amd/rir.py; csrc/rir/rir_hrir.cuh on the walk of rir_shell.cuh, the FIR tile of
rir_fir.cuh and the host side of rir_host.h) against the fp64 restatement of tests/rir_hrir_ref.py,
against closed forms and the merged kernels, bitwise repeatability, and the plumbing up to the dataset script.

Parity is the bound of tests/test_gpu_rir.py, ``rir_ref.bound``: ``|h - float32(h_ref)| <= 2^-23 max|h_ref|`` per tap.
It carries over because every sum -- direction rows, fold and band filters -- is fp64 and the only fp32 rounding is the
store. Every parity test first asserts that the restatement's least margin between the best and the second-best
direction of an image is at least 1e-9: a condition on the inputs, so that fp64 rounding cannot change an argmax."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_ref
import rir_bands_ref as B
import rir_hrir_ref as H
import rir_ref as R
from brever_amd import rir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
FS = 16000
BETA6 = (0.8, 0.7, 0.6, 0.75, 0.5, 0.65)
MARGIN = 1e-9
_REF, _SETS = {}, {}


def _beta(K, tilt=0.93):
    """Six different walls, different in every band (the construction of tests/test_gpu_rir_bands.py)."""
    return np.array([[b*tilt**k*(1.0 - 0.02*((k + w) % 3)) for w, b in enumerate(BETA6)] for k in range(K)])


def _grid_set(taps, seed=1):
    """The 38-direction fixture set, one object per argument set (``simulate_brirs`` groups by identity)."""
    if (taps, seed) not in _SETS:
        az, el = H.fixture_grid()
        _SETS[taps, seed] = rir.HrirSet.from_angles(az, el, H.fixture_hrirs(38, taps, seed), FS)
    return _SETS[taps, seed]


ROOMS = {'a257': dict(dims=(3.2, 2.6, 2.4), head=(1.4, 1.2, 1.3), yaw=0.3, angles=(25.0,), distance=1.0, taps=257),
         'a700': dict(dims=(3.2, 2.6, 2.4), head=(1.4, 1.2, 1.3), yaw=0.3, angles=(25.0,), distance=1.0, taps=700),
         'a1100': dict(dims=(3.2, 2.6, 2.4), head=(1.4, 1.2, 1.3), yaw=0.3, angles=(25.0,), distance=1.0, taps=1100),
         'c400': dict(dims=(4.1, 3.3, 2.7), head=(1.9, 1.45, 1.25), yaw=1.1, angles=(-70.0,), distance=1.2, taps=400)}


def _room(name, beta, hrirs, **over):
    kw = dict(ROOMS[name], beta=beta, ear_model='hrir', hrirs=hrirs)
    kw.update(over)
    return rir.ShoeboxRoom(**kw)


def _ref(room, angle=None, fs=FS, **kw):
    """``(response, margins, directions in use)`` of the restatement for one angle of a room, computed once per
    argument set and left unchanged."""
    angle = room.angles[0] if angle is None else angle
    key = (room.dims, room.beta, room.head, room.yaw, angle, room.distance, room.taps, room.hrirs.directions.tobytes(),
           room.hrirs.hrirs.tobytes(), fs, tuple(sorted(kw.items())))
    if key not in _REF:
        used = set()
        h, margins = H.brir(room.dims, room.beta, room.head, room.yaw, angle, room.distance, room.taps, fs,
                            room.hrirs.directions, room.hrirs.hrirs, used=used, **kw)
        h.setflags(write=False)
        _REF[key] = (h, margins, len(used))
    return _REF[key]


def _hold(name, got, ref):
    """The parity bound on one response, figures printed before the assertion."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max())
    print(f'{name}: peak {np.abs(ref).max():.4e}, |h - f32(ref)| {err:.3e}, bound {R.bound(ref):.3e}')
    assert np.abs(ref).max() > 0 and err <= R.bound(ref), name


def _hold_ears(name, got, ref):
    for e, ear in enumerate(('left', 'right')):
        _hold(f'{name} {ear}', np.ascontiguousarray(got[:, e]), ref[:, e])


def _parity(name, room, **kw):
    ref, margins, used = _ref(room, **kw)
    print(f'{name}: {len(margins)} images, {used} of {len(room.hrirs)} directions in use, least margin '
          f'{margins.min():.2e}')
    assert margins.min() >= MARGIN, name
    got = rir.simulate_brirs([room], fs=FS, device=DEV, **kw)[0][0]
    _hold_ears(name, got, ref)
    return got


# -- parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,bands,taps_h', [('a257', 0, 24), ('a700', 3, 40), ('c400', 3, 24), ('c400', 0, 40)])
def test_parity_with_the_restatement(name, bands, taps_h):
    """257 + 128 and 700 + 128 taps of a direction row are not whole tiles, the 700-tap room fills the list of a far
    tile more than once, and neither 24 nor 40 HRIR taps are a multiple of the fold's 16."""
    _parity(f'{name} K = {bands} T_h = {taps_h}', _room(name, _beta(bands) if bands else BETA6, _grid_set(taps_h)))


@pytest.mark.parametrize('K', range(1, 9))
def test_every_tile_kernel_the_dispatch_can_return(K):
    """All eight instantiations of ``rir_hrir_tile_kernel``, which share the walk, the list entry and the tap weight of
    the band kernels (csrc/rir/rir_shell.cuh), on the room of the same test of tests/test_gpu_rir_bands.py. The last
    band's centre has to lie below fs/2, so K = 7 and 8 run at 48 kHz, with a set of that rate. The last tile of a
    direction row is not a whole tile and lists more than 256 images, counted from the job's own tables: a list of 512
    entries (K <= 6) is sorted and flushed in the middle of the tile, a list of 256 many times."""
    fs, taps = (FS, 600) if K <= 6 else (48000, 2900)
    az, el = H.fixture_grid()
    hrirs = _grid_set(24) if fs == FS else rir.HrirSet.from_angles(az, el, H.fixture_hrirs(38, 24, 1), fs)
    room = rir.ShoeboxRoom((3.2, 2.6, 2.4), _beta(K), (1.4, 1.2, 1.3), math.radians(20.0), 1.0, (40.0,), taps,
                           ear_model='hrir', hrirs=hrirs)
    _, pad = rir.band_filters(fs, K)
    rows, index, _ = rir.build_hrir_tables(rir._hrir_geom_row(room.dims, room.beta, room.source(40.0), room.head,
                                                              room.front(), room.side()), [[taps, 0, 2, 1]],
                                           rir.hrir_opts(fs, K, hrirs, 33, pad=pad), hrirs.directions)
    images = R.last_tile_images(rows, index, 0, taps + pad, fs, 33)
    print(f'K = {K}: rows of {taps + pad} taps, {(taps + pad - 1)%rir.TILE + 1} in the last tile, which lists {images} '
          f'images')
    assert (taps + pad)%rir.TILE != 0 and images > 256
    ref, margins, used = _ref(room, fs=fs, window=33)
    print(f'K = {K}: {len(margins)} images, {used} of {len(hrirs)} directions in use, least margin {margins.min():.2e}')
    assert margins.min() >= MARGIN
    _hold_ears(f'K = {K}', rir.simulate_brirs([room], fs=fs, window=33, device=DEV)[0][0], ref)


@pytest.mark.parametrize('angle,azimuth', [(90.0, 90), (-90.0, 270), (0.0, 0)])
def test_free_field_is_the_hrir_of_the_direction_found_by_hand(angle, azimuth):
    """No wall reflects: each ear is the HRIR pair of (azimuth, elevation 0) scaled by 1 / (4 pi d) and delayed by the
    windowed sinc. Pins left and right, the sign of the azimuth and the yaw without the restatement's direction code."""
    hrirs, d, taps = _grid_set(24), 1.2, 200
    j = 12 + azimuth//30                                    # the ring at elevation 0 follows the 12 of elevation -45
    az, el = H.fixture_grid()
    assert (az[j], el[j]) == (azimuth, 0.0)
    room = rir.ShoeboxRoom((6.0, 5.0, 3.0), (0.0,)*6, (3.0, 2.5, 1.5), 0.3, d, (angle,), taps, ear_model='hrir',
                           hrirs=hrirs)
    got = rir.simulate_brirs([room], fs=FS, device=DEV)[0][0]
    N, W = B.default_n(FS), B.default_window(FS)
    t = np.arange(taps + N//2)
    u = t - d*FS/343.0
    x = np.where(np.abs(u) < W/2, np.sinc(u)*(1 + np.cos(2*math.pi*u/W))/2, 0.0)/(4*math.pi*d)
    for e, ear in enumerate(('left', 'right')):
        y = np.convolve(x, hrirs.hrirs[j, e])[:len(t)]
        _hold(f'free field, angle {angle}, {ear}', np.ascontiguousarray(got[:, e]),
              B.combine([y], B.bank(FS, 1), taps, N))
    assert np.abs(got[:, 0] - got[:, 1]).max() > 1e-3


@pytest.mark.parametrize('bands', [1, 3])
def test_an_all_impulse_set_is_the_merged_kernels_with_an_omni_receiver(bands):
    """Ties the new kernels to ``simulate_rirs`` without the restatement: both round one fp64 sum to fp32."""
    impulses = np.zeros((38, 2, 16))
    impulses[:, :, 0] = 1.0
    az, el = H.fixture_grid()
    beta = _beta(bands)
    room = _room('a700', beta, rir.HrirSet.from_angles(az, el, impulses, FS))
    got = rir.simulate_brirs([room], fs=FS, device=DEV)[0][0]
    omni = rir.simulate_rirs(room.dims, beta, [room.source(25.0)], [room.head], [(1.0, 0.0, 0.0)], [1.0], room.taps, FS,
                             device=DEV)[0, 0].cpu().numpy()
    for e in range(2):
        diff = float(np.abs(got[:, e].astype(np.float64) - omni).max())
        print(f'K = {bands} ear {e}: peak {np.abs(omni).max():.4e}, impulse set - omni {diff:.3e}, bound '
              f'{R.bound(omni):.3e}')
        assert np.abs(omni).max() > 1e-2 and diff <= R.bound(omni)


def test_parity_with_more_pairs_than_the_workgroup_has_lanes():
    """1 100 taps with a window of 48: 17 x 21 = 357 (x, y) pairs, so the list is carried across two rounds of pairs,
    and about 4 000 images, so that the far tiles flush it several times."""
    room = _room('a1100', BETA6, _grid_set(24))
    opts = rir.hrir_opts(FS, 1, room.hrirs, 48)
    _, index, _ = rir.build_hrir_tables(rir._hrir_geom_row(room.dims, room.beta, room.source(25.0), room.head,
                                                           room.front(), room.side()), [[1100, 0, 2, 1]], opts,
                                        room.hrirs.directions)
    assert index[0, 1]*index[0, 2] > 256
    _parity('1 100 taps', room, window=48)
    assert len(_ref(room, window=48)[1]) > 4000             # in 10 tiles: the last ones hold more than a list of 512


# -- the tie rule, and sets of other sizes ---------------------------------------------------------------------------
def test_ties_go_to_the_lowest_index_and_the_order_of_a_set_does_not_matter():
    hrirs = _grid_set(24)
    room = _room('a700', BETA6, hrirs)
    alone = _parity('the set alone', room)
    doubled = rir.HrirSet(np.concatenate([hrirs.directions, hrirs.directions]),
                          np.concatenate([hrirs.hrirs, H.fixture_hrirs(38, 24, 9)]), FS)
    twice = rir.simulate_brirs([_room('a700', BETA6, doubled)], fs=FS, device=DEV)[0][0]
    assert twice.tobytes() == alone.tobytes()              # every image ties exactly between j and j + 38
    turned = rir.HrirSet(hrirs.directions[::-1], hrirs.hrirs[::-1], FS)
    got = rir.simulate_brirs([_room('a700', BETA6, turned)], fs=FS, device=DEV)[0][0]
    _hold_ears('the set reversed', got, _ref(room)[0])


def test_one_direction_one_dropped_and_seven_hundred():
    hrirs = _grid_set(24)
    one = rir.HrirSet(hrirs.directions[5:6], hrirs.hrirs[5:6], FS)
    ref, margins, used = _ref(_room('a257', BETA6, one))
    assert used == 1 and np.isinf(margins).all()
    _hold_ears('D = 1', rir.simulate_brirs([_room('a257', BETA6, one)], fs=FS, device=DEV)[0][0], ref)
    keep = [j for j in range(38) if j != 15]
    _parity('D = 37', _room('a257', _beta(3), rir.HrirSet(hrirs.directions[keep], hrirs.hrirs[keep], FS)))
    many = rir.HrirSet(H.fibonacci_sphere(700, 4), H.fixture_hrirs(700, 16, 4), FS)
    _parity('D = 700', _room('c400', BETA6, many, taps=300))


# -- bitwise -----------------------------------------------------------------------------------------------------
def _batch_rooms():
    return [_room('a257', _beta(3), _grid_set(24), angles=(25.0, -110.0)),
            _room('c400', _beta(3), _grid_set(24), taps=131, angles=(-70.0,)),
            _room('a257', _beta(3), _grid_set(24), yaw=2.0, taps=200, angles=(5.0, 60.0))]


def test_repeatable_alone_as_in_a_batch_and_whatever_the_chunks():
    rooms = _batch_rooms()
    first = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    again = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    assert [[h.shape for h in room] for room in first] == [[(257, 2)]*2, [(131, 2)], [(200, 2)]*2]
    for a_room, b_room in zip(first, again):
        for a, b in zip(a_room, b_room):
            assert np.abs(a).max() > 1e-3 and a.tobytes() == b.tobytes()
    for i, room in enumerate(rooms):
        for k, angle in enumerate(room.angles):
            alone = _room('a257', room.beta, room.hrirs, dims=room.dims, head=room.head, yaw=room.yaw,
                          distance=room.distance, taps=room.taps, angles=(angle,))
            got = rir.simulate_brirs([alone], fs=FS, window=48, device=DEV)[0][0]
            assert got.tobytes() == first[i][k].tobytes(), (i, k)
    _hold_ears('batch room 0 angle 1', first[0][1], _ref(rooms[0], -110.0, window=48)[0])
    # a job of K = 3, D = 38 and 257 taps takes 3 (38 + 2)(257 + 128) doubles of the two scratches: room for one only
    job = 8*3*40*(257 + 128)
    assert len(rir.chunk_jobs([257, 257, 131, 200, 200], 3*40, 128, job)) == 5
    chunked = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV, scratch_bytes=job)
    for a_room, b_room in zip(first, chunked):
        for a, b in zip(a_room, b_room):
            assert a.tobytes() == b.tobytes()


def test_one_call_with_two_sets_a_pattern_room_and_a_sphere_room():
    rooms = [_room('a257', _beta(3), _grid_set(24)),
             rir.ShoeboxRoom((5.1, 4.3, 2.9), _beta(3, 0.97), (2.0, 2.2, 1.5), 2.0, 1.5, (-60.0, 35.0), 200),
             _room('c400', _beta(3), _grid_set(40), taps=150),
             rir.ShoeboxRoom((3.2, 2.6, 2.4), BETA6, (1.4, 1.2, 1.3), 0.3, 1.0, (25.0,), 257, ear_model='sphere'),
             _room('c400', BETA6, _grid_set(24), taps=150)]
    together = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    for i, room in enumerate(rooms):
        own = rir.simulate_brirs([room], fs=FS, window=48, device=DEV)[0]
        assert len(own) == len(together[i]) == len(room.angles)
        for a, b in zip(own, together[i]):
            assert np.abs(a).max() > 1e-3 and a.tobytes() == b.tobytes(), i
    assert together[2][0].tobytes() != together[4][0].tobytes()


# -- a wrong index is not followed ---------------------------------------------------------------------------------
def test_a_job_that_points_outside_the_tables_or_a_scratch_is_skipped():
    hrirs, K, D, taps = _grid_set(24), 3, 38, 200
    room = _room('c400', _beta(K), hrirs, taps=taps, angles=(-70.0, 20.0))
    geom = [rir._hrir_geom_row(room.dims, room.beta, room.source(a), room.head, room.front(), room.side())
            for a in room.angles]
    shape = np.array([[taps, 0, 2, 1], [taps, 2*taps, 2, 1]])
    filters, pad = rir.band_filters(FS, K)
    opts, copts = rir.hrir_opts(FS, K, hrirs, 48, pad=pad), rir.band_opts(FS, K, window=48, pad=pad)
    rows, index, ear = rir.build_hrir_tables(geom, shape, opts, hrirs.directions)
    T = taps + pad
    dir_job, fold_job = K*D*T, 2*K*T
    tables, filters_d = torch.from_numpy(rows).to(DEV), torch.tensor(filters, device=DEV)
    dirs_d = torch.tensor(hrirs.directions, device=DEV)
    responses = torch.from_numpy(rir.padded_hrirs(hrirs)).to(DEV)

    def run(ix, ex=ear, dir_len=2*dir_job, fold_len=2*fold_job):
        dirs = torch.full((2*dir_job,), 7.0, dtype=torch.float64, device=DEV)
        fold = torch.full((2*fold_job,), 7.0, dtype=torch.float64, device=DEV)
        out = torch.full((4*taps,), 7.0, dtype=torch.float32, device=DEV)
        rir.launch_hrir(tables, torch.from_numpy(ix).to(DEV), torch.from_numpy(ex).to(DEV), opts, copts, -1, taps,
                        dirs_d, responses, dirs[:dir_len], fold[:fold_len], filters_d, out)
        torch.cuda.synchronize()
        return out.cpu().numpy(), dirs.cpu().numpy(), fold.cpu().numpy()

    good, dirs_good, fold_good = run(index)
    assert not (good == 7.0).any() and not (fold_good == 7.0).any() and np.abs(dirs_good[dir_job:]).max() > 1e-3

    def first_job_is_as_it_was(out, dirs, fold, why):
        assert np.array_equal(out[:2*taps], good[:2*taps]), why
        assert np.array_equal(dirs[:dir_job], dirs_good[:dir_job]), why
        assert np.array_equal(fold[:fold_job], fold_good[:fold_job]), why

    # the tables: the tile kernel writes nothing of the job, whose rows stay cleared
    for word, value in ((0, len(rows)), (0, -1), (1, rir.MAX_AXIS_ROWS + 1), (3, len(rows))):
        bad = index.copy()
        bad[1, word] = value
        out, dirs, fold = run(bad)
        first_job_is_as_it_was(out, dirs, fold, (word, value))
        assert not dirs[dir_job:].any() and not fold[fold_job:].any(), (word, value)
    # taps and the direction scratch: neither the tile kernel nor the fold follows the job
    for word, value in ((4, 0), (5, -8), (5, dir_job + 1)):
        bad = index.copy()
        bad[1, word] = value
        out, dirs, fold = run(bad)
        first_job_is_as_it_was(out, dirs, fold, (word, value))
        assert not dirs[dir_job:].any() and (fold[fold_job:] == 7.0).all(), (word, value)
    # the fold scratch: the rows are built, the fold is not done
    for value in (-8, fold_job + 1):
        bad = index.copy()
        bad[1, 7] = value
        out, dirs, fold = run(bad)
        first_job_is_as_it_was(out, dirs, fold, (7, value))
        assert np.array_equal(dirs, dirs_good) and (fold[fold_job:] == 7.0).all(), value
    # an ear whose rows would end outside the fold scratch is skipped by the band filters
    bad = ear.copy()
    bad[3, 7] = 2*fold_job - K*T + 1
    out, dirs, fold = run(index, bad)
    assert np.array_equal(out[:2*taps], good[:2*taps]) and np.array_equal(out[2*taps::2], good[2*taps::2])
    assert (out[2*taps + 1::2] == 7.0).all()
    # scratches that end inside the second job's rows: the job is skipped; too small for one job: refused
    out, dirs, fold = run(index, dir_len=2*dir_job - 1)
    first_job_is_as_it_was(out, dirs, fold, 'short direction scratch')
    assert (dirs[dir_job:-1] == 0.0).all() and dirs[-1] == 7.0 and (fold[fold_job:] == 7.0).all()
    out, dirs, fold = run(index, fold_len=2*fold_job - 1)
    first_job_is_as_it_was(out, dirs, fold, 'short fold scratch')
    assert np.array_equal(dirs, dirs_good) and (fold[fold_job:] == 7.0).all() and (out[2*taps + 1::2] == 7.0).all()
    with pytest.raises(RuntimeError, match='direction scratch is too small'):
        run(index, dir_len=dir_job - 1)
    with pytest.raises(RuntimeError, match='fold scratch is too small'):
        run(index, fold_len=fold_job - 1)


# -- resampling --------------------------------------------------------------------------------------------------
def test_a_48_khz_set_is_resampled_as_the_host_restatement_does():
    az, el = H.fixture_grid()
    high = rir.HrirSet.from_angles(az, el, H.fixture_hrirs(38, 96, 3), 48000)
    low = high.resample(FS, DEV)
    assert low is high.resample(FS, DEV) and low.fs == FS and low.taps == 32 and len(low) == 38       # cached
    assert np.array_equal(low.directions, high.directions)
    columns = high.hrirs.reshape(76, 96).T
    ref = resample_ref.resample(columns, 48000, FS)
    yard = resample_ref.rel(resample_ref.bluestein(columns, 48000, FS), ref)
    err = resample_ref.rel(low.hrirs.reshape(76, 32).T, ref)
    print(f'48 kHz to 16 kHz: rel-L2 {err:.3e}, yardstick {yard:.3e}')
    assert err <= 8*yard and err < 1e-13                   # the bound of tests/test_gpu_resample.py
    # and a room on the 48 kHz set is the room on the resampled one
    a = rir.simulate_brirs([_room('a257', BETA6, high)], fs=FS, device=DEV)[0][0]
    b = rir.simulate_brirs([_room('a257', BETA6, low)], fs=FS, device=DEV)[0][0]
    assert np.abs(a).max() > 1e-3 and a.tobytes() == b.tobytes()


# -- plumbing ----------------------------------------------------------------------------------------------------
def _tree(path):
    return {os.path.relpath(os.path.join(d, name), path): open(os.path.join(d, name), 'rb').read()
            for d, _, names in os.walk(path) for name in names}


def test_create_dataset_with_a_measured_ear(tmp_path):
    rng = np.random.default_rng(5)
    speech = [(0.1*rng.standard_normal(8000)).astype(np.float32) for _ in range(2)]
    rir.save_pool(str(tmp_path/'pool.npz'), [], speech, [(0.1*rng.standard_normal(16000)).astype(np.float32)])
    _grid_set(24).save(str(tmp_path/'set.npz'))

    def create(name, *flags, code=0):
        cmd = [sys.executable, 'scripts/create_dataset.py', '--pool', str(tmp_path/'pool.npz'), '--output',
               str(tmp_path/name), '--size', '4', '--simulate_rooms', '2', '--room_taps', '800', '--room_angles',
               '-30', '0', '30', '--noise_count', '1', '1', '--block_size', '1024', *flags]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        assert (out.returncode == 0) == (code == 0), out.stdout[-2000:] + out.stderr[-3000:]
        return _tree(str(tmp_path/name)) if code == 0 else out.stderr

    measured = create('hrir', '--room_ear_model', 'hrir', '--room_hrirs', str(tmp_path/'set.npz'))
    again = create('again', '--room_ear_model', 'hrir', '--room_hrirs', str(tmp_path/'set.npz'))
    sphere = create('sphere', '--room_ear_model', 'sphere')
    assert measured.keys() == again.keys() and len(measured) >= 1
    for name in measured:
        assert measured[name] == again[name], name
    assert [name for name in measured if measured[name] != sphere.get(name)], 'the sphere archive was written again'
    assert '--room_hrirs' in create('none', '--room_ear_model', 'hrir', code=2)
    assert '--room_hrirs' in create('both', '--room_ear_model', 'sphere', '--room_hrirs', str(tmp_path/'set.npz'),
                                    code=2)
