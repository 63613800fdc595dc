"""The shoebox image-source simulator on the GPU (brever_amd/rir.py; csrc/rir/rir.hip on rir_shell.cuh and rir_host.h) against
the fp64 restatement of tests/rir_ref.py, its bitwise repeatability, and the simulated BRIRs as the pool of the mixture engine.

Parity is held on the fp32 output: ``|h - float32(h_ref)| <= 2^-23 max|h_ref|`` per tap, one output rounding with a
factor two of slack; the fp64 evaluation error of either side is orders of magnitude below it."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rir_ref as R
from brever_amd import rir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
FS = 16000
BETA6 = (0.8, 0.7, 0.6, 0.75, 0.5, 0.65)
_REF = {}


def _ref_brirs(key, rooms, fs=FS, **kw):
    """The restatement's BRIRs of ``rooms``, computed once per ``key`` and left unchanged."""
    if key not in _REF:
        _REF[key] = [[R.brir(room.dims, room.beta, room.head, room.yaw, angle, room.distance, room.taps, fs,
                             room.ear_pattern, room.head_radius, **kw) for angle in room.angles] for room in rooms]
        for room in _REF[key]:
            for h in room:
                h.setflags(write=False)
    return _REF[key]


def _hold(name, got, ref):
    """The parity bound on one response, figures printed before the assertion."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max())
    print(f'{name}: peak {np.abs(ref).max():.4e}, |h - f32(ref)| {err:.3e}, bound {R.bound(ref):.3e}')
    assert np.abs(ref).max() > 0 and err <= R.bound(ref), name


def _hold_rooms(name, got, ref):
    assert len(got) == len(ref) and [len(g) for g in got] == [len(r) for r in ref]
    for i, (g_room, r_room) in enumerate(zip(got, ref)):
        for a, (g, r) in enumerate(zip(g_room, r_room)):
            for e, ear in enumerate(('left', 'right')):
                _hold(f'{name} room {i} angle {a} {ear}', np.ascontiguousarray(g[:, e]), r[:, e])


def _room_b(**over):
    kw = dict(dims=(3.2, 2.6, 2.4), beta=BETA6, head=(1.4, 1.2, 1.3), yaw=math.radians(20.0), distance=1.0,
              angles=(40.0,), taps=640)
    kw.update(over)
    return rir.ShoeboxRoom(**kw)


def _ragged_rooms():
    return [rir.ShoeboxRoom((3.2, 2.6, 2.4), BETA6, (1.4, 1.2, 1.3), 0.3, 1.0, (25.0,), 257),
            rir.ShoeboxRoom((5.1, 4.3, 2.9), (0.9, 0.85, 0.8, 0.9, 0.6, 0.7), (2.0, 2.2, 1.5), 2.0, 1.5,
                            (-60.0, -20.0, 0.0, 35.0, 90.0), 400),
            rir.ShoeboxRoom((2.5, 3.6, 2.2), (0.6,)*6, (1.2, 1.9, 1.1), 4.0, 0.6, (-45.0, 10.0, 170.0), 131)]


# -- parity ------------------------------------------------------------------------------------------------------
def test_anechoic_exact_integer_delay():
    args = ((4.0, 3.0, 2.5), (0.0,)*6, [(1.0, 1.5, 1.2)], [(2.25, 1.5, 1.2)], [(1.0, 0.0, 0.0)], [1.0], 128, 16384)
    h = rir.simulate_rirs(*args, window=64, c=320.0, device=DEV)
    assert h.shape == (1, 1, 128) and h.dtype == torch.float32 and h.is_cuda
    ref = R.rir(args[0], args[1], args[2][0], args[3][0], args[4][0], 1.0, 128, 16384, window=64, c=320.0)
    _hold('anechoic', h[0, 0].cpu().numpy(), ref)
    assert h[0, 0, 64].item() == np.float32(1.0/(4*math.pi*1.25))


def test_a_small_room_with_six_different_walls():
    rooms = [_room_b()]
    count = []
    source, ears, sides = R.head_geometry(rooms[0].head, rooms[0].yaw, 40.0, 1.0)
    R.rir(rooms[0].dims, BETA6, source, ears[0], sides[0], 0.75, 640, FS, window=64, count=count)
    print(f'images of the left ear: {count[0]}')
    assert 400 <= count[0] <= 900
    _hold_rooms('small room', rir.simulate_brirs(rooms, fs=FS, window=64, device=DEV),
                _ref_brirs('b', rooms, window=64))


def test_a_window_clipped_at_both_ends_and_taps_off_the_tile():
    # the source 0.2 m from the left ear: 9.3 samples, less than half of the window of 33
    rooms = [_room_b(angles=(90.0,), distance=0.2 + 0.0875, taps=333)]
    assert abs(np.linalg.norm(rooms[0].source(90.0) - rooms[0].ears()[0]) - 0.2) < 1e-12
    ref = _ref_brirs('c', rooms, window=33)
    assert abs(ref[0][0][0, 0]) > 1e-6 and abs(ref[0][0][332, 0]) > 1e-9       # both ends are inside a window
    _hold_rooms('clipped', rir.simulate_brirs(rooms, fs=FS, window=33, device=DEV), ref)


def test_a_wall_that_reflects_nothing():
    rooms = [_room_b(beta=(0.8, 0.0, 0.6, 0.75, 0.5, 0.65), taps=400)]
    _hold_rooms('dead wall', rir.simulate_brirs(rooms, fs=FS, window=64, device=DEV),
                _ref_brirs('d', rooms, window=64))


@pytest.mark.parametrize('max_order', [0, 1, 2])
def test_max_order(max_order):
    rooms = [_room_b(taps=400)]
    ref = _ref_brirs(('e', max_order), rooms, window=64, max_order=max_order)
    _hold_rooms(f'max_order {max_order}', rir.simulate_brirs(rooms, fs=FS, window=64, max_order=max_order, device=DEV),
                ref)
    if max_order:
        assert np.abs(ref[0][0] - _ref_brirs(('e', max_order - 1), rooms, window=64, max_order=max_order - 1)[0][0]).max() > 1e-4


def test_a_ragged_batch_of_three_rooms():
    rooms = _ragged_rooms()
    got = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    assert [[h.shape for h in room] for room in got] == [[(257, 2)], [(400, 2)]*5, [(131, 2)]*3]
    _hold_rooms('ragged', got, _ref_brirs('f', rooms, window=48))


def test_several_receivers_with_mixed_patterns():
    dims, taps = (3.2, 2.6, 2.4), 300
    sources = [(0.9, 1.7, 1.1), (2.1, 0.6, 1.9)]
    receivers = [(2.4, 0.8, 1.6), (1.0, 1.0, 1.0), (1.6, 2.2, 0.4), (2.9, 2.3, 2.0)]
    orientations = [(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.6, 0.0, 0.8), (-0.6, 0.64, 0.48)]
    patterns = [1.0, 0.5, 0.75, 0.0]
    h = rir.simulate_rirs(dims, BETA6, sources, receivers, orientations, patterns, taps, FS, window=40, device=DEV)
    assert h.shape == (2, 4, taps)
    got = h.cpu().numpy()
    for s in range(2):
        for r in range(4):
            ref = R.rir(dims, BETA6, sources[s], receivers[r], orientations[r], patterns[r], taps, FS, window=40)
            _hold(f'source {s} receiver {r}', got[s, r], ref)


def test_a_long_response_takes_several_rounds_of_pairs_and_list_flushes():
    """The sizes at which the kernel takes its other paths: more (x, y) pairs than the workgroup has lanes, and more
    images in a tile than its list holds (512), so that the list is consumed and refilled."""
    dims, taps = (3.2, 2.6, 2.4), 2000
    args = (dims, BETA6, [(0.9, 1.7, 1.1)], [(2.4, 0.8, 1.6)], [(0.6, 0.0, 0.8)], [0.5], taps, FS)
    geom = rir._geom_row(dims, BETA6, args[2][0], args[3][0], args[4][0], 0.5)
    _, index, _ = rir.build_tables(geom, np.array([[taps, 0, 1]]), FS, window=64)
    assert index[0, 1]*index[0, 2] > 3*256
    count = []
    ref = R.rir(dims, BETA6, args[2][0], args[3][0], args[4][0], 0.5, taps, FS, window=64, count=count)
    print(f'{count[0]} images, {index[0, 1]*index[0, 2]} pairs, {-(-taps//rir.TILE)} tiles')
    assert count[0] > 8*512
    _hold('long', rir.simulate_rirs(*args, window=64, device=DEV)[0, 0].cpu().numpy(), ref)


# -- bitwise -----------------------------------------------------------------------------------------------------
def test_repeatable_and_a_job_alone_equals_the_job_in_a_batch():
    rooms = _ragged_rooms()
    first = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    again = rir.simulate_brirs(rooms, fs=FS, window=48, device=DEV)
    for a_room, b_room in zip(first, again):
        for a, b in zip(a_room, b_room):
            assert a.tobytes() == b.tobytes()
    for i, room in enumerate(rooms):
        for k, angle in enumerate(room.angles):
            alone = rir.ShoeboxRoom(room.dims, room.beta, room.head, room.yaw, room.distance, (angle,), room.taps)
            got = rir.simulate_brirs([alone], fs=FS, window=48, device=DEV)[0][0]
            assert got.tobytes() == first[i][k].tobytes(), (i, k)


# -- plumbing ----------------------------------------------------------------------------------------------------
def _signals():
    rng = np.random.default_rng(5)
    speech = [(0.1*rng.standard_normal(8000)).astype(np.float32) for _ in range(2)]
    return speech, [(0.1*rng.standard_normal(16000)).astype(np.float32)]


def test_simulated_brirs_are_a_pool_of_the_mixture_maker():
    from brever_amd.mixture import PoolMixtureMaker
    speech, noises = _signals()
    brirs = rir.simulate_brirs(rir.random_rooms(2, seed=0, taps=800, angles=(-30, 0, 30)), device=DEV)
    assert [[h.shape for h in room] for room in brirs] == [[(800, 2)]*3]*2
    assert all(h.dtype == np.float32 and np.isfinite(h).all() and np.abs(h).max() > 1e-3 for room in brirs for h in room)

    def epoch():
        maker = PoolMixtureMaker(None, ['mixture', 'foreground'], 4, speech=speech, noises=noises, brirs=brirs,
                                 seed=1, noise_count=(1, 1), device=DEV)
        maker.set_epoch(2)
        return [[np.array(x) for x in maker[i]] for i in range(4)]

    a, b = epoch(), epoch()
    assert len(a) == 4
    for item_a, item_b in zip(a, b):
        for x, y in zip(item_a, item_b):
            assert np.isfinite(x).all() and np.abs(x).max() > 0 and x.tobytes() == y.tobytes()


def test_create_dataset_with_simulated_rooms(tmp_path):
    from brever_amd.data import BreverDataset
    speech, noises = _signals()
    rir.save_pool(str(tmp_path/'pool.npz'), [], speech, noises)
    dset = tmp_path/'dset'
    cmd = [sys.executable, 'scripts/create_dataset.py', '--pool', str(tmp_path/'pool.npz'), '--output', str(dset),
           '--size', '4', '--simulate_rooms', '2', '--room_taps', '800', '--room_angles', '-30', '0', '30',
           '--noise_count', '1', '1', '--block_size', '1024']
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert '4 mixtures' in out.stdout
    data = BreverDataset(str(dset))
    assert len(data) == 4
    item = data[0]
    assert torch.isfinite(item).all() and item.abs().max() > 0
