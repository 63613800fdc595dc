"""Binaural room impulse responses of shoebox rooms by the image-source method, on the HIP path: the BRIR pool of
``mixture.PoolMixtureMaker`` without a measured database.

The kernels are in ``libbrever_rir.so`` (include/rir/brever_rir.h; csrc/rir/rir.hip). A room is a box
with one reflection coefficient per wall; every image of the source contributes a Hann-windowed sinc at its delay,
scaled by the walls it crossed, by ``1/(4 pi d)`` and by a first-order receiver pattern. An ear is such a receiver
(subcardioid by default) pointing outwards from the head; there is no head shadow beyond that. Geometry, window and
accumulation are fp64, the output is fp32; results are bitwise repeatable and a response is the same alone as in a
batch.

``simulate_brirs(random_rooms(n, seed))`` is the ``brirs=`` argument of ``PoolMixtureMaker``; ``save_pool`` writes the
``.npz`` its ``path`` argument reads. There is no CPU fallback: without the library or a ROCm device the calls raise.
"""
import math

import numpy as np
import torch

from . import hip

# the brv_rir_* entry points of include/rir/brever_rir.h
_LIB = hip.Library('rir/brever_rir.h', 'libbrever_rir.so', 'BRV_RIR_LIB_PATH',
                   'The room simulator has no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, query, last_error = _LIB.lib, _LIB.call, _LIB.query, _LIB.last_error
GEOM_DOUBLES, SHAPE_WORDS, OPT_DOUBLES, ROW_DOUBLES, INDEX_WORDS, TILE, MAX_AXIS_ROWS, MAX_TAPS, MAX_JOBS = (
    _LIB.constants['BRV_RIR_' + name] for name in (
        'GEOM_DOUBLES', 'SHAPE_WORDS', 'OPT_DOUBLES', 'ROW_DOUBLES', 'INDEX_WORDS', 'TILE', 'MAX_AXIS_ROWS',
        'MAX_TAPS', 'MAX_JOBS'))
SABINE = 0.161                                   # s/m


class ShoeboxRoom:
    """A room with a head in it: ``dims`` (3,) metres, ``beta`` (6,) wall reflection coefficients
    ``(x0, x1, y0, y1, z0, z1)``, ``head`` (3,) the head's centre, ``yaw`` radians (the head looks along
    ``(cos yaw, sin yaw, 0)``), a source at ``distance`` metres at the ears' height for every azimuth of ``angles``
    (degrees, counter-clockwise seen from above: positive is left), responses of ``taps`` samples."""

    def __init__(self, dims, beta, head, yaw, distance, angles, taps, ear_pattern=0.75, head_radius=0.0875):
        self.dims = tuple(float(v) for v in dims)
        self.beta = tuple(float(v) for v in beta)
        self.head = tuple(float(v) for v in head)
        self.yaw, self.distance, self.angles, self.taps = float(yaw), float(distance), \
            tuple(float(v) for v in angles), int(taps)
        self.ear_pattern, self.head_radius = float(ear_pattern), float(head_radius)
        if len(self.dims) != 3 or len(self.beta) != 6 or len(self.head) != 3 or not self.angles:
            raise ValueError('dims and head have 3 values, beta has 6, angles at least one')

    def side(self):
        """Unit vector from the head's centre to the left ear."""
        return np.array([-math.sin(self.yaw), math.cos(self.yaw), 0.0])

    def ears(self):
        """``(left, right)`` positions."""
        hc, off = np.array(self.head), self.head_radius*self.side()
        return hc + off, hc - off

    def source(self, angle):
        az = self.yaw + math.radians(angle)
        return np.array(self.head) + self.distance*np.array([math.cos(az), math.sin(az), 0.0])

    def __repr__(self):
        return (f'ShoeboxRoom(dims={self.dims}, beta={self.beta}, head={self.head}, yaw={self.yaw}, '
                f'distance={self.distance}, angles={self.angles}, taps={self.taps}, '
                f'ear_pattern={self.ear_pattern}, head_radius={self.head_radius})')


def beta_from_rt60(dims, rt60):
    """The one reflection coefficient of all six walls that gives ``rt60`` seconds by Sabine's formula: uniform
    absorption ``alpha = 0.161 V / (S rt60)``, ``beta = sqrt(1 - alpha)``. ``ValueError`` for an ``rt60`` the room
    cannot reach (``alpha >= 1``)."""
    alpha = min_rt60(dims)/rt60 if rt60 > 0 else math.inf
    if not alpha < 1.0:
        raise ValueError(f'rt60 {rt60} s is out of reach of a {tuple(dims)} m room: Sabine absorption {alpha:.3f} >= 1')
    return math.sqrt(1.0 - alpha)


def min_rt60(dims):
    """``0.161 V / S``: the rt60 at which Sabine's absorption reaches 1."""
    lx, ly, lz = (float(v) for v in dims)
    return SABINE*lx*ly*lz/(2.0*(lx*ly + lx*lz + ly*lz))


def default_window(fs):
    return float(round(0.008*fs))


def build_tables(geom, shape, fs, window=None, max_order=-1, c=343.0):
    """The two host steps of the library for ``geom`` (J, 19) float64 and ``shape`` (J, 3) int64 (the header says
    what they hold): ``(rows, index, opts)``, the per-axis candidate tables of every job, where each job's tables
    are, and the three options as the library takes them. Refused values raise with the library's message."""
    geom = np.ascontiguousarray(geom, dtype=np.float64).reshape(-1, GEOM_DOUBLES)
    shape = np.ascontiguousarray(shape, dtype=np.int64).reshape(-1, SHAPE_WORDS)
    jobs = len(geom)
    if len(shape) != jobs:
        raise ValueError('one shape row per job')
    opts = np.array([fs, c, default_window(fs) if window is None else window], dtype=np.float64)
    assert len(opts) == OPT_DOUBLES
    n_rows = query('brv_rir_table_rows', geom.ctypes.data, shape.ctypes.data, jobs, opts.ctypes.data, max_order)
    rows = np.empty((n_rows, ROW_DOUBLES), dtype=np.float64)
    index = np.empty((jobs, INDEX_WORDS), dtype=np.int64)
    call('brv_rir_build_tables', geom.ctypes.data, shape.ctypes.data, jobs, opts.ctypes.data, max_order,
         rows.ctypes.data, index.ctypes.data, n_rows)
    return rows, index, opts


def launch(tables, index, opts, max_order, max_taps, out):
    """``brv_rir_simulate`` on the current stream: ``tables`` and ``index`` as built, on the device of ``out``."""
    hip.require_device(tables, index, out)
    call('brv_rir_simulate', tables, index, len(index), len(tables), int(max_taps), opts.ctypes.data, int(max_order),
         out, out.numel(), hip.stream())


def _run(geom, shape, fs, window, max_order, c, device):
    """Tables, upload and launch; returns the flat fp32 output on the device, zeros where no job writes."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'brever_amd kernels run on a ROCm device only; got {device} (there is no CPU fallback)')
    max_order = int(max_order)
    rows, index, opts = build_tables(geom, shape, fs, window, max_order, c)
    out_len = int((index[:, 5] + (index[:, 4] - 1)*index[:, 6]).max()) + 1
    with torch.cuda.device(device):
        out = torch.zeros(out_len, dtype=torch.float32, device=device)
        launch(torch.from_numpy(rows).to(device), torch.from_numpy(index).to(device), opts, max_order,
               index[:, 4].max(), out)
    return out


def _geom_row(dims, beta, source, receiver, orientation, pattern):
    row = np.empty(GEOM_DOUBLES)
    row[0:3], row[3:9], row[9:12], row[12:15], row[15:18], row[18] = dims, beta, source, receiver, orientation, \
        pattern
    return row


def simulate_rirs(dims, beta, sources, receivers, orientations, patterns, taps, fs, window=None, max_order=-1,
                  c=343.0, device='cuda'):
    """Responses of one room from every source to every receiver: ``sources`` (S, 3), ``receivers`` (R, 3),
    ``orientations`` (R, 3) unit vectors, ``patterns`` (R,) in [0, 1] (1 omni, 0.5 cardioid). Returns a
    ``(S, R, taps)`` float32 tensor on ``device``."""
    sources, receivers, orientations = (np.asarray(v, dtype=np.float64).reshape(-1, 3)
                                        for v in (sources, receivers, orientations))
    patterns = np.asarray(patterns, dtype=np.float64).reshape(-1)
    if not len(receivers) == len(orientations) == len(patterns):
        raise ValueError('one orientation and one pattern per receiver')
    taps = int(taps)
    geom = [_geom_row(dims, beta, s, receivers[i], orientations[i], patterns[i])
            for s in sources for i in range(len(receivers))]
    shape = [(taps, j*taps, 1) for j in range(len(geom))]
    out = _run(np.array(geom), np.array(shape), fs, window, max_order, c, device)
    return out.view(len(sources), len(receivers), taps)


def simulate_brirs(rooms, fs=16000, window=None, max_order=-1, c=343.0, device='cuda'):
    """The BRIRs of every ``ShoeboxRoom`` of ``rooms`` in one launch: a list of rooms, each a list with one
    ``(taps, 2)`` float32 array (left, right) per angle -- the ``brirs=`` argument of ``PoolMixtureMaker``."""
    geom, shape, at = [], [], 0
    for room in rooms:
        ears, side = room.ears(), room.side()
        for angle in room.angles:
            source = room.source(angle)
            for e in range(2):
                geom.append(_geom_row(room.dims, room.beta, source, ears[e], side if e == 0 else -side,
                                      room.ear_pattern))
                shape.append((room.taps, at + e, 2))
            at += 2*room.taps
    if not geom:
        return []
    flat = _run(np.array(geom), np.array(shape), fs, window, max_order, c, device).cpu().numpy()
    out, at = [], 0
    for room in rooms:
        out.append([flat[at + 2*room.taps*i:at + 2*room.taps*(i + 1)].reshape(room.taps, 2)
                    for i in range(len(room.angles))])
        at += 2*room.taps*len(room.angles)
    return out


def random_rooms(n, seed, dims=((3, 3, 2.4), (10, 8, 4)), rt60=(0.2, 0.8), distance=(0.5, 3.0),
                 angles=range(-90, 91, 10), margin=0.3, taps=None, fs=16000, ear_pattern=0.75, head_radius=0.0875):
    """``n`` rooms drawn from ``np.random.default_rng([seed])``, a function of the arguments only. Per room, in this
    order: the three dimensions uniformly between ``dims[0]`` and ``dims[1]``; the source distance uniformly in
    ``distance``, capped so that a circle of that radius plus ``head_radius + margin`` fits the floor plan; the
    head's centre uniformly where that circle stays inside (no rejection); the ears' height uniformly in
    ``[1.0, min(1.8, Lz - margin)]``; the yaw uniformly in [0, 2 pi); ``rt60`` uniformly in its range, raised to 1.01
    times the least that Sabine's formula allows the room. ``taps`` defaults to ``ceil(rt60 fs)``."""
    rng = np.random.default_rng([int(seed)])
    lo, hi = np.asarray(dims[0], dtype=np.float64), np.asarray(dims[1], dtype=np.float64)
    rooms = []
    for _ in range(int(n)):
        L = rng.uniform(lo, hi)
        clear = head_radius + margin
        rho_max = 0.5*min(L[0], L[1]) - clear
        if not rho_max > 0.0 or L[2] - margin < 1.0:
            raise ValueError(f'a {tuple(L)} m room has no place for a head with margin {margin}')
        rho = min(float(rng.uniform(distance[0], distance[1])), rho_max)
        keep = rho + clear
        # (a capped distance leaves a span of 0 along the shorter side, which rounding may make -1e-16)
        hx, hy = keep + rng.uniform(size=2)*np.maximum(L[:2] - 2.0*keep, 0.0)
        hz = rng.uniform(1.0, min(1.8, L[2] - margin))
        yaw = rng.uniform(0.0, 2.0*math.pi)
        t60 = max(float(rng.uniform(rt60[0], rt60[1])), 1.01*min_rt60(L))
        rooms.append(ShoeboxRoom(L, (beta_from_rt60(L, t60),)*6, (hx, hy, hz), yaw, rho, angles,
                                 math.ceil(t60*fs) if taps is None else taps, ear_pattern, head_radius))
        rooms[-1].rt60 = t60
    return rooms


def save_pool(path, brirs, speech=(), noises=()):
    """Write the ``.npz`` that ``PoolMixtureMaker(path, ...)`` reads: ``brir_<room>_<angle>``, ``speech_<i>``,
    ``noise_<i>``."""
    arrays = {f'brir_{r}_{a}': np.asarray(h, dtype=np.float32) for r, room in enumerate(brirs)
              for a, h in enumerate(room)}
    arrays.update({f'speech_{i}': np.asarray(x, dtype=np.float32) for i, x in enumerate(speech)})
    arrays.update({f'noise_{i}': np.asarray(x, dtype=np.float32) for i, x in enumerate(noises)})
    np.savez(path, **arrays)
