"""Octave-band walls and the spherical-head ear on the GPU (brever_amd/rir.py; csrc/rir/rir_bands.cuh on the walk of
rir_shell.cuh, the FIR tile of rir_fir.cuh and the host side of rir_host.h) against the fp64
restatement of tests/rir_bands_ref.py, bitwise repeatability, and the plumbing up to the dataset script.

Parity is the bound of tests/test_gpu_rir.py, ``rir_ref.bound``: ``|h - float32(h_ref)| <= 2^-23 max|h_ref|`` per tap.
It carries over because every sum, those of the filters included, is fp64 and the only fp32 rounding is the store."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rir_bands_ref as B
import rir_ref as R
from brever_amd import rir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
FS, RAD = 16000, 0.0875
BETA6 = (0.8, 0.7, 0.6, 0.75, 0.5, 0.65)
_REF = {}


def _beta(K, tilt=0.93):
    """Six different walls, different in every band."""
    return np.array([[b*tilt**k*(1.0 - 0.02*((k + w) % 3)) for w, b in enumerate(BETA6)] for k in range(K)])


def _ref_room(room, fs=FS, only=None, **kw):
    """The restatement's BRIRs of one room, computed once per argument set and left unchanged."""
    key = (repr(room), fs, only, tuple(sorted(kw.items())))
    if key not in _REF:
        beta = np.reshape(room.beta, (-1, 6))
        _REF[key] = [B.brir(room.dims, beta, room.head, room.yaw, angle, room.distance, room.taps, fs,
                            room.ear_model == 'sphere', room.ear_pattern, room.head_radius, **kw)
                     for a, angle in enumerate(room.angles) if only is None or a == only]
        for h in _REF[key]:
            h.setflags(write=False)
    return _REF[key]


def _hold(name, got, ref):
    """The parity bound on one response, figures printed before the assertion."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max())
    print(f'{name}: peak {np.abs(ref).max():.4e}, |h - f32(ref)| {err:.3e}, bound {R.bound(ref):.3e}')
    assert np.abs(ref).max() > 0 and err <= R.bound(ref), name


def _hold_room(name, got, ref):
    assert len(got) == len(ref)
    for a, (g, r) in enumerate(zip(got, ref)):
        for e, ear in enumerate(('left', 'right')):
            _hold(f'{name} angle {a} {ear}', np.ascontiguousarray(g[:, e]), r[:, e])


def _room_b(**over):
    kw = dict(dims=(3.2, 2.6, 2.4), beta=BETA6, head=(1.4, 1.2, 1.3), yaw=math.radians(20.0), distance=1.0,
              angles=(40.0,), taps=640)
    kw.update(over)
    return rir.ShoeboxRoom(**kw)


# -- parity ------------------------------------------------------------------------------------------------------
def test_equal_bands_tie_the_new_path_to_the_old_one():
    room = _room_b(beta=[BETA6]*6, taps=300)
    got = rir.simulate_brirs([room], fs=FS, window=64, device=DEV)[0]
    _hold_room('equal bands', got, _ref_room(room, window=64))
    old = rir.simulate_brirs([_room_b(taps=300)], fs=FS, window=64, device=DEV)[0][0]
    source, ears, sides = R.head_geometry(room.head, room.yaw, 40.0, 1.0)
    for e in range(2):
        one = R.rir(room.dims, BETA6, source, ears[e], sides[e], 0.75, 300, FS, window=64)
        _hold(f'equal bands against the single-band restatement, ear {e}', np.ascontiguousarray(got[0][:, e]), one)
        diff = float(np.abs(got[0][:, e].astype(np.float64) - old[:, e]).max())
        print(f'ear {e}: new path - old path {diff:.3e}')
        assert diff <= R.bound(one)
    # simulate_rirs with beta (K, 6) is the same path
    again = rir.simulate_rirs(room.dims, [BETA6]*6, [source], ears, sides, [0.75, 0.75], 300, FS, window=64,
                              device=DEV)
    assert again.shape == (1, 2, 300) and again.dtype == torch.float32 and again.is_cuda
    assert np.array_equal(again[0].cpu().numpy().T, got[0])


@pytest.mark.parametrize('K,fs,near', [(3, 16000, 0.2), (8, 48000, 0.1)])
def test_six_walls_different_in_every_band(K, fs, near):
    # the source `near` m from the left ear: less than half of the window of 33, so tap 0 is inside a window
    room = _room_b(beta=_beta(K), angles=(90.0,), distance=near + RAD, taps=333)
    ref = _ref_room(room, fs, window=33)
    assert abs(ref[0][0, 0]) > 1e-9 and abs(ref[0][332, 0]) > 1e-9
    assert np.abs(ref[0] - _ref_room(_room_b(beta=[_beta(K)[0]]*K, angles=(90.0,), distance=near + RAD, taps=333),
                                     fs, window=33)[0]).max() > 1e-4       # the bands matter
    _hold_room(f'K = {K}', rir.simulate_brirs([room], fs=fs, window=33, device=DEV)[0], ref)


@pytest.mark.parametrize('model', ['pattern', 'sphere'])
@pytest.mark.parametrize('K', range(1, 9))
def test_every_tile_kernel_the_dispatch_can_return(K, model):
    """All sixteen instantiations of ``rir_bands_tile_kernel``, which share one walk, one list entry and one tap weight
    (csrc/rir/rir_shell.cuh). The last band's centre has to lie below fs/2, so K = 7 and 8 run at 48 kHz. The taps are
    chosen so that the last tile of a channel row, which is not a whole tile, lists more than 256 images: a list of
    512 entries (C <= 4) is then flushed in the middle of the tile and a list of 256 many times. The count is taken
    from the job's own tables, so that the input cannot silently stop reaching the flush."""
    fs, taps = (FS, 600) if K <= 6 else (48000, 2900)
    room = _room_b(beta=_beta(K), taps=taps, ear_model=model)
    _, pad = rir.band_filters(fs, K, model)
    ears, side = room.ears(), room.side()
    geom = [rir._band_geom_row(room.dims, room.beta, room.source(40.0), room.head if model == 'sphere' else ears[e],
                               side if e == 0 else -side, room.ear_pattern) for e in range(2)]
    rows, index = rir.build_band_tables(geom, [[taps, e, 2] for e in range(2)],
                                        rir.band_opts(fs, K, model, window=33, pad=pad))
    widen = (0.5*math.pi*RAD, RAD) if model == 'sphere' else (0.0, 0.0)     # the range of the head's delay
    images = [R.last_tile_images(rows, index, e, taps + pad, fs, 33, *widen) for e in range(2)]
    print(f'K = {K} {model}: rows of {taps + pad} taps, {(taps + pad - 1)%rir.TILE + 1} in the last tile, which lists '
          f'{images} images')
    assert (taps + pad)%rir.TILE != 0 and min(images) > 256
    _hold_room(f'K = {K} {model}', rir.simulate_brirs([room], fs=fs, window=33, device=DEV)[0],
               _ref_room(room, fs, window=33))


def _envelope_peak(h):
    """Place of the peak of the analytic envelope, refined by a parabola through three samples."""
    n = len(h)
    w = np.zeros(n)
    w[0], w[1:n//2], w[n//2] = 1.0, 2.0, 1.0
    env = np.abs(np.fft.ifft(np.fft.fft(h)*w))
    i = int(env.argmax())
    a, b, c = env[i - 1], env[i], env[i + 1]
    return i + 0.5*(a - c)/(a - 2*b + c)


def test_sphere_mode_in_an_anechoic_room():
    angles = (0.0, 90.0, -90.0, 150.0)
    room = rir.ShoeboxRoom((6.0, 5.0, 3.0), np.zeros((6, 6)), (3.0, 2.5, 1.5), 0.0, 1.2, angles, 400,
                           ear_model='sphere')
    got = rir.simulate_brirs([room], fs=FS, device=DEV)[0]
    _hold_room('anechoic sphere', got, _ref_room(room))
    woodworth = lambda az: RAD*(math.sin(az) + az)*FS/343.0                       # noqa: E731, az in [0, pi/2]
    for a, az in ((1, math.pi/2), (3, math.pi/6)):          # 150 degrees is 30 degrees from the ears' axis
        left, right = _envelope_peak(got[a][:, 0].astype(np.float64)), _envelope_peak(got[a][:, 1].astype(np.float64))
        print(f'azimuth {angles[a]}: envelope peaks {left:.3f}, {right:.3f}: right - left {right - left:.3f}, '
              f'Woodworth {woodworth(az):.3f} samples')
        assert left < right and abs((right - left) - woodworth(az)) <= 0.5
    left, right = _envelope_peak(got[2][:, 0].astype(np.float64)), _envelope_peak(got[2][:, 1].astype(np.float64))
    assert right < left and abs((left - right) - woodworth(math.pi/2)) <= 0.5
    frontal = got[0].astype(np.float64)
    assert np.abs(frontal[:, 0] - frontal[:, 1]).max() <= 2*R.bound(frontal[:, 0])
    f = np.fft.rfftfreq(400, 1.0/FS)
    for a, near in ((1, 0), (2, 1)):
        power = np.abs(np.fft.rfft(got[a].astype(np.float64), axis=0))**2
        high = power[f > 2000.0].sum(axis=0)
        print(f'azimuth {angles[a]}: energy above 2 kHz, near ear {high[near]:.3e}, far ear {high[1 - near]:.3e}')
        assert high[near] > high[1 - near]


@pytest.mark.parametrize('angle,geometric,word', [(90.0, 130.0, 'shortened'), (-90.0, 124.0, 'lengthened')])
def test_the_head_delay_moves_an_image_across_a_tile_edge(angle, geometric, word):
    d = geometric*343.0/FS
    room = rir.ShoeboxRoom((8.0, 6.0, 3.0), np.zeros((1, 6)), (2.0, 3.0, 1.5), 0.0, d, (angle,), 300,
                           ear_model='sphere')
    delta = -RAD if angle > 0 else RAD*math.pi/2           # of the left ear
    tau = (d + delta)*FS/343.0
    print(f'{word}: geometric delay {geometric:.2f}, head-model delay {tau:.2f} samples, tile edge at {rir.TILE}')
    assert (geometric < rir.TILE) != (tau < rir.TILE) and abs(tau - geometric) > 4.0
    got = rir.simulate_brirs([room], fs=FS, window=33, device=DEV)[0]
    _hold_room(word, got, _ref_room(room, window=33))


def test_sphere_mode_in_a_reverberant_room_takes_several_rounds_and_list_flushes():
    """The room of the long-response test of tests/test_gpu_rir.py with K = 6 in sphere mode (C = 12): more (x, y)
    pairs than the workgroup has lanes, and more images in a tile than its list of 256 fat entries holds."""
    dims, taps, beta = (3.2, 2.6, 2.4), 2000, _beta(6, 0.985)
    source, centre, axis = (0.9, 1.7, 1.1), (2.4, 0.8, 1.6), (0.6, 0.0, 0.8)
    opts = rir.band_opts(FS, 6, 'sphere', RAD, 64)
    _, index = rir.build_band_tables(rir._band_geom_row(dims, beta, source, centre, axis, 0.5),
                                     np.array([[taps, 0, 1]]), opts)
    count = []
    ref = B.rir(dims, beta, source, centre, axis, 0.5, taps, FS, True, RAD, window=64, count=count)
    print(f'{count[0]} images, {index[0, 1]*index[0, 2]} pairs, {-(-(taps + 128)//rir.TILE)} tiles')
    assert index[0, 1]*index[0, 2] > 3*256 and count[0] > 8*512
    got = rir.simulate_rirs(dims, beta, [source], [centre], [axis], [0.5], taps, FS, window=64, device=DEV,
                            ear_model='sphere', head_radius=RAD)
    _hold('long sphere', got[0, 0].cpu().numpy(), ref)


def _ragged_rooms():
    return [rir.ShoeboxRoom((3.2, 2.6, 2.4), BETA6, (1.4, 1.2, 1.3), 0.3, 1.0, (25.0,), 257, ear_model='sphere'),
            rir.ShoeboxRoom((5.1, 4.3, 2.9), _beta(6, 0.97), (2.0, 2.2, 1.5), 2.0, 1.5, (-60.0, 35.0), 200),
            rir.ShoeboxRoom((2.5, 3.6, 2.2), _beta(6, 0.9), (1.2, 1.9, 1.1), 4.0, 0.6, (-45.0, 170.0), 131,
                            ear_model='sphere')]


@pytest.mark.parametrize('max_order', [-1, 0, 2])
def test_a_ragged_batch_of_three_rooms_in_three_groups(max_order):
    rooms = _ragged_rooms()
    got = rir.simulate_brirs(rooms, fs=FS, window=48, max_order=max_order, device=DEV)
    assert [[h.shape for h in room] for room in got] == [[(257, 2)], [(200, 2)]*2, [(131, 2)]*2]
    for i, room in enumerate(rooms):
        if max_order < 0 or i == 2:
            _hold_room(f'ragged room {i} max_order {max_order}', got[i],
                       _ref_room(room, window=48, max_order=max_order))
    if max_order >= 0:                                     # the orders differ: 0 from all, 2 from 0
        other = _ref_room(rooms[2], window=48, max_order=-1 if max_order == 0 else 0)
        assert np.abs(got[2][0] - other[0]).max() > 1e-4


# -- bitwise -----------------------------------------------------------------------------------------------------
def test_repeatable_alone_as_in_a_batch_and_whatever_the_chunks():
    rooms = _ragged_rooms()
    first = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    again = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    for a_room, b_room in zip(first, again):
        for a, b in zip(a_room, b_room):
            assert a.tobytes() == b.tobytes()
    for i, room in enumerate(rooms):
        for k, angle in enumerate(room.angles):
            alone = rir.ShoeboxRoom(room.dims, room.beta, room.head, room.yaw, room.distance, (angle,), room.taps,
                                    ear_model=room.ear_model)
            got = rir.simulate_brirs([alone], fs=FS, window=48, device=DEV)[0][0]
            assert got.tobytes() == first[i][k].tobytes(), (i, k)
    # the K = 6 sphere room has four jobs of 12 (131 + 128) doubles: room for two makes two chunks, for one four
    job = 8*12*(131 + 128)
    assert len(rir.chunk_jobs([131]*4, 12, 128, 2*job - 1)) == 4 and len(rir.chunk_jobs([131]*4, 12, 128, 2*job)) == 2
    rooms3 = [rooms[2], rir.ShoeboxRoom(rooms[2].dims, rooms[2].beta, rooms[2].head, 1.0, 0.5, (10.0,), 131,
                                        ear_model='sphere')]
    assert len(rir.chunk_jobs([131]*6, 12, 128, 2*job)) == 3
    whole = rir.simulate_brirs(rooms3, fs=FS, window=48, device=DEV)
    chunked = rir.simulate_brirs(rooms3, fs=FS, window=48, device=DEV, scratch_bytes=2*job)
    for a_room, b_room in zip(whole, chunked):
        for a, b in zip(a_room, b_room):
            assert np.abs(a).max() > 1e-3 and a.tobytes() == b.tobytes()


# -- a wrong index is not followed ---------------------------------------------------------------------------------
def test_a_job_that_points_outside_the_tables_or_the_scratch_is_skipped():
    room = _ragged_rooms()[1]
    source, ears, side = room.source(35.0), room.ears(), room.side()
    geom = [rir._band_geom_row(room.dims, room.beta, source, ears[e], side if e == 0 else -side, 0.75)
            for e in range(2)]
    shape = np.array([[200, 0, 1], [200, 200, 1]])
    filters, pad = rir.band_filters(FS, 6)
    opts = rir.band_opts(FS, 6, window=48, pad=pad)
    rows, index = rir.build_band_tables(geom, shape, opts)
    tables, filters_d = torch.from_numpy(rows).to(DEV), torch.tensor(filters, device=DEV)
    need = 2*6*(200 + pad)

    def run(ix, scratch_len=need):
        scratch = torch.zeros(need, dtype=torch.float64, device=DEV)
        out = torch.full((400,), 7.0, dtype=torch.float32, device=DEV)
        rir.launch_bands(tables, torch.from_numpy(ix).to(DEV), opts, -1, 200, scratch[:scratch_len], filters_d, out)
        torch.cuda.synchronize()
        return out.cpu().numpy(), scratch.cpu().numpy()

    good, rows_good = run(index)
    assert not (good == 7.0).any() and np.abs(rows_good).max() > 1e-3
    for word, value in ((0, len(rows)), (0, -1), (1, rir.MAX_AXIS_ROWS + 1), (3, len(rows)), (4, 0), (7, -8),
                        (7, need - 6*(200 + pad) + 1)):
        bad = index.copy()
        bad[1, word] = value
        out, scratch = run(bad)
        assert np.array_equal(out[:200], good[:200]), (word, value)                  # the other job is as it was
        assert np.array_equal(scratch[:need//2], rows_good[:need//2]), (word, value)
        assert not scratch[need//2:].any(), (word, value)                            # nothing of the job was written
        if word in (4, 7):
            assert (out[200:] == 7.0).all(), (word, value)                           # and the combine step skips it
    # a scratch that ends inside the second job's rows: the job is skipped by both kernels
    out, scratch = run(index, need - 1)
    assert np.array_equal(out[:200], good[:200]) and (out[200:] == 7.0).all() and not scratch[need//2:].any()
    # and one that cannot hold a job of max_taps is refused on the host
    with pytest.raises(RuntimeError, match='scratch is too small'):
        run(index, 6*(200 + pad) - 1)


# -- plumbing ----------------------------------------------------------------------------------------------------
def _signals():
    rng = np.random.default_rng(5)
    speech = [(0.1*rng.standard_normal(8000)).astype(np.float32) for _ in range(2)]
    return speech, [(0.1*rng.standard_normal(16000)).astype(np.float32)]


def test_banded_sphere_brirs_are_a_pool_of_the_mixture_maker():
    from brever_amd.mixture import PoolMixtureMaker
    speech, noises = _signals()
    rooms = rir.random_rooms(2, 0, bands=6, ear_model='sphere', taps=800, angles=(-30, 0, 30))
    brirs = rir.simulate_brirs(rooms, device=DEV)
    assert [[h.shape for h in room] for room in brirs] == [[(800, 2)]*3]*2
    assert all(h.dtype == np.float32 and np.isfinite(h).all() and np.abs(h).max() > 1e-3 for room in brirs for h in room)
    maker = PoolMixtureMaker(None, ['mixture', 'foreground'], 4, speech=speech, noises=noises, brirs=brirs, seed=1,
                             noise_count=(1, 1), device=DEV)
    maker.set_epoch(2)
    for i in range(4):
        for x in maker[i]:
            x = np.array(x)
            assert np.isfinite(x).all() and np.abs(x).max() > 0


def _tree(path):
    return {os.path.relpath(os.path.join(d, name), path): open(os.path.join(d, name), 'rb').read()
            for d, _, names in os.walk(path) for name in names}


def test_create_dataset_with_the_room_flags(tmp_path):
    from brever_amd.data import BreverDataset
    speech, noises = _signals()
    rir.save_pool(str(tmp_path/'pool.npz'), [], speech, noises)

    def create(name, *flags):
        cmd = [sys.executable, 'scripts/create_dataset.py', '--pool', str(tmp_path/'pool.npz'), '--output',
               str(tmp_path/name), '--size', '4', '--simulate_rooms', '2', '--room_taps', '800', '--room_angles',
               '-30', '0', '30', '--noise_count', '1', '1', '--block_size', '1024', *flags]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        assert '4 mixtures' in out.stdout
        return _tree(str(tmp_path/name))

    sphere = create('sphere', '--room_bands', '6', '--room_ear_model', 'sphere')
    data = BreverDataset(str(tmp_path/'sphere'))
    assert len(data) == 4
    item = data[0]
    assert torch.isfinite(item).all() and item.abs().max() > 0
    # the flags at their defaults take the code path that the script took before it had them: the same bytes
    absent = create('absent')
    defaults = create('defaults', '--room_bands', '0', '--room_band_tilt', '0.0', '0.25', '--room_ear_model', 'pattern')
    assert absent.keys() == defaults.keys() and len(absent) >= 1
    audio = [name for name in absent if absent[name] != sphere.get(name)]
    assert audio, 'the banded rooms wrote the archive of the plain ones'
    for name in absent:
        assert absent[name] == defaults[name], name
