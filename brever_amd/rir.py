"""Binaural room impulse responses of shoebox rooms by the image-source method, on the HIP path: the BRIR pool of
``mixture.PoolMixtureMaker`` without a measured database.

The kernels are in ``libbrever_rir.so`` (include/rir/brever_rir.h; csrc/rir/rir.hip). A room is a box
with one reflection coefficient per wall; every image of the source contributes a Hann-windowed sinc at its delay,
scaled by the walls it crossed, by ``1/(4 pi d)`` and by a first-order receiver pattern. An ear is such a receiver
(subcardioid by default) pointing outwards from the head; there is no head shadow beyond that. Geometry, window and
accumulation are fp64, the output is fp32; results are bitwise repeatable and a response is the same alone as in a
batch.

With ``beta`` of shape ``(K, 6)`` the walls have one coefficient per octave band (centres ``125 * 2^k`` Hz), and with
``ear_model='sphere'`` an ear is a point on a rigid sphere (Brown & Duda 1998): a delay that follows the path round
the head and a head shadow that grows with frequency (include/rir/brever_rir_bands.h; csrc/rir/rir_bands.cuh;
DESIGN.md 5n). Every image then has one amplitude per channel, the tile kernel accumulates the channels together and
a second kernel passes each through its fixed filter (``band_filters``).

With ``ear_model='hrir'`` the ear is a measured one: an ``HrirSet`` (``load_sofa``, ``load_hrirs``) gives a pair of
head-related impulse responses per measured direction, every image goes to the measured direction nearest to its
arrival, and the per-direction responses are folded with that direction's pair (include/rir/brever_rir_hrir.h;
csrc/rir/rir_hrir.cuh). Interpolation between measured directions, distance-dependent and near-field
HRTFs, head pitch and roll, SOFA conventions other than ``SimpleFreeFieldHRIR``, air absorption, source directivity and
other room shapes stay out of scope.

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
# the brv_rir_bands_* entry points of the same library (include/rir/brever_rir_bands.h)
_BANDS = hip.Library('rir/brever_rir_bands.h', 'libbrever_rir.so', 'BRV_RIR_LIB_PATH',
                     'The room simulator has no CPU fallback.')
bands_call, bands_query = _BANDS.call, _BANDS.query
MAX_BANDS, BANDS_GEOM_DOUBLES, BANDS_OPT_DOUBLES, PATTERN, SPHERE, MAX_FILTER, COMBINE_TILE = (
    _BANDS.constants['BRV_RIR_BANDS_' + name] for name in (
        'MAX_BANDS', 'GEOM_DOUBLES', 'OPT_DOUBLES', 'PATTERN', 'SPHERE', 'MAX_FILTER', 'COMBINE_TILE'))
EAR_MODELS = {'pattern': PATTERN, 'sphere': SPHERE}
# the brv_rir_hrir_* entry points of the same library (include/rir/brever_rir_hrir.h)
_HRIR = hip.Library('rir/brever_rir_hrir.h', 'libbrever_rir.so', 'BRV_RIR_LIB_PATH',
                    'The room simulator has no CPU fallback.')
hrir_call, hrir_query = _HRIR.call, _HRIR.query
HRIR_MAX_DIRS, HRIR_MAX_TAPS, HRIR_GEOM_DOUBLES, HRIR_SHAPE_WORDS, HRIR_OPT_DOUBLES, HRIR_FOLD_TILE = (
    _HRIR.constants['BRV_RIR_HRIR_' + name] for name in (
        'MAX_DIRS', 'MAX_TAPS', 'GEOM_DOUBLES', 'SHAPE_WORDS', 'OPT_DOUBLES', 'FOLD_TILE'))
ROOM_EAR_MODELS = sorted(EAR_MODELS) + ['hrir']  # of a ShoeboxRoom: the library's two modes and the measured ear
FILTER_MULTIPLE = 16                             # brv_rir_bands_combine takes the filter 16 taps at a time
SABINE = 0.161                                   # s/m


class HrirSet:
    """A measured ear: ``directions`` (D, 3) vectors in the head's frame (x front, y left, z up; any length but zero,
    stored as unit vectors), ``hrirs`` (D, 2, T_h) the left and right head-related impulse responses of each
    direction, ``fs`` their sampling rate. ``1 <= D <= 2048``, ``1 <= T_h <= 512``. The arrays are float64 and
    read-only. The simulator takes, per image, the direction with the largest cosine to the arrival (ties to the
    lowest index) and keeps the responses' own onset delay as measured."""

    def __init__(self, directions, hrirs, fs):
        directions = np.array(directions, dtype=np.float64)
        hrirs = np.array(hrirs, dtype=np.float64)
        if directions.ndim != 2 or directions.shape[1] != 3:
            raise ValueError(f'directions is (D, 3), not {directions.shape}')
        if hrirs.ndim != 3 or hrirs.shape[0] != len(directions) or hrirs.shape[1] != 2:
            raise ValueError(f'hrirs is (D, 2, T_h) with D = {len(directions)}, not {hrirs.shape}')
        if not 1 <= len(directions) <= HRIR_MAX_DIRS:
            raise ValueError(f'requires 1 <= D <= {HRIR_MAX_DIRS} directions, not {len(directions)}')
        if not 1 <= hrirs.shape[2] <= HRIR_MAX_TAPS:
            raise ValueError(f'requires 1 <= T_h <= {HRIR_MAX_TAPS} taps, not {hrirs.shape[2]}')
        if not np.isfinite(directions).all() or not np.isfinite(hrirs).all():
            raise ValueError('directions and hrirs must be finite')
        norm = np.sqrt((directions*directions).sum(axis=1))
        if not (norm > 0.0).all():
            raise ValueError(f'direction {int(np.argmin(norm > 0.0))} has zero length')
        if not (np.isfinite(fs) and fs > 0):
            raise ValueError(f'fs must be positive and finite, not {fs}')
        # (a vector that is unit to rounding is kept as given, so that a saved set loads with the same bits)
        norm = np.where(np.abs(norm - 1.0) <= 1e-15, 1.0, norm)
        self.directions, self.hrirs, self.fs = directions/norm[:, None], hrirs, float(fs)
        self.directions.setflags(write=False)
        self.hrirs.setflags(write=False)
        self._resampled = {}

    def __setattr__(self, name, value):
        if name in ('directions', 'hrirs', 'fs') and name in self.__dict__:
            raise AttributeError(f'an HrirSet is read-only: {name}')
        object.__setattr__(self, name, value)

    @classmethod
    def from_angles(cls, azimuth_deg, elevation_deg, hrirs, fs):
        """Directions by azimuth (degrees, counter-clockwise seen from above: 0 front, 90 left) and elevation
        (degrees, 90 up): ``p = (cos el cos az, cos el sin az, sin el)``, SOFA's spherical convention."""
        az, el = np.radians(np.asarray(azimuth_deg, dtype=np.float64)), \
            np.radians(np.asarray(elevation_deg, dtype=np.float64))
        if az.ndim != 1 or az.shape != el.shape:
            raise ValueError('one azimuth and one elevation per direction')
        return cls(np.stack([np.cos(el)*np.cos(az), np.cos(el)*np.sin(az), np.sin(el)], axis=1), hrirs, fs)

    def __len__(self):
        return len(self.directions)

    @property
    def taps(self):
        return self.hrirs.shape[2]

    def resample(self, fs, device='cuda'):
        """The set at ``fs``: every response through ``io.resample_batch`` (whole-signal Fourier resampling, fp64, on
        the device), cached per ``fs``. The set itself if ``fs`` is its own."""
        fs = float(fs)
        if fs == self.fs:
            return self
        if fs not in self._resampled:
            from . import io
            D, _, taps = self.hrirs.shape
            columns = np.ascontiguousarray(self.hrirs.reshape(2*D, taps).T)         # (samples, channels)
            with torch.cuda.device(_device(device)):
                out, = io.resample_batch([columns], self.fs, fs, dtype=torch.float64, device=_device(device))
            self._resampled[fs] = HrirSet(self.directions, out.cpu().numpy().T.reshape(D, 2, -1), fs)
        return self._resampled[fs]

    def save(self, path):
        """The ``.npz`` form that ``load_hrirs`` reads: ``directions``, ``hrirs``, ``fs``."""
        np.savez(path, directions=self.directions, hrirs=self.hrirs, fs=np.float64(self.fs))

    def __repr__(self):
        return f'HrirSet(D={len(self)}, taps={self.taps}, fs={self.fs:g})'


def load_hrirs(path):
    """The ``HrirSet`` that ``HrirSet.save`` wrote; a ``.sofa`` file goes to ``load_sofa``."""
    if str(path).lower().endswith('.sofa'):
        return load_sofa(path)
    with np.load(path) as z:
        missing = [k for k in ('directions', 'hrirs', 'fs') if k not in z.files]
        if missing:
            raise ValueError(f'{path}: no array {missing[0]!r}: not a file of HrirSet.save')
        return HrirSet(z['directions'], z['hrirs'], float(z['fs']))


def load_sofa(path):
    """The ``HrirSet`` of a SOFA file (AES69) of convention ``SimpleFreeFieldHRIR``: ``Data.IR`` (M, 2, N),
    ``Data.SamplingRate``, ``SourcePosition`` (M, 3) with its ``Type`` (``spherical``: azimuth and elevation in
    degrees and a radius that is not used, or ``cartesian``). Read with the HDF5 C library (``h5lite``);
    ``RuntimeError`` without it, ``ValueError`` naming the field for another convention, ``R != 2`` or a ``DataType``
    other than ``FIR``. The listener's own orientation (``ListenerView``) is taken as SOFA's default: x front, z up."""
    from . import h5lite
    if not h5lite.available():
        raise RuntimeError('load_sofa needs the HDF5 C library (libhdf5, libhdf5_hl), which could not be loaded; '
                           'convert the set to the .npz form of HrirSet.save')
    with h5lite.File(path, 'r') as f:
        convention = f.read_attr('/', 'SOFAConventions')
        if convention != 'SimpleFreeFieldHRIR':
            raise ValueError(f'{path}: SOFAConventions is {convention!r}, not SimpleFreeFieldHRIR')
        data_type = f.read_attr('/', 'DataType')
        if data_type != 'FIR':
            raise ValueError(f'{path}: DataType is {data_type!r}, not FIR')
        for key in ('Data.IR', 'Data.SamplingRate', 'SourcePosition'):
            if key not in f:
                raise ValueError(f'{path}: no {key}')
        ir, rate, position = f.read_array('Data.IR'), f.read_array('Data.SamplingRate'), f.read_array('SourcePosition')
        kind = f.read_attr('SourcePosition', 'Type')
    if ir.ndim != 3 or ir.shape[1] != 2:
        raise ValueError(f'{path}: Data.IR is (M, R, N) with R = 2 receivers, not {ir.shape}')
    if position.shape != (ir.shape[0], 3):
        raise ValueError(f'{path}: SourcePosition is (M, 3) with M = {ir.shape[0]}, not {position.shape}')
    if rate.size < 1 or not (rate.ravel() == rate.ravel()[0]).all():
        raise ValueError(f'{path}: Data.SamplingRate holds no rate or more than one')
    if kind == 'spherical':
        return HrirSet.from_angles(position[:, 0], position[:, 1], ir, float(rate.ravel()[0]))
    if kind == 'cartesian':
        return HrirSet(position, ir, float(rate.ravel()[0]))
    raise ValueError(f'{path}: SourcePosition Type is {kind!r}, neither spherical nor cartesian')


class ShoeboxRoom:
    """A room with a head in it: ``dims`` (3,) metres, ``beta`` (6,) wall reflection coefficients
    ``(x0, x1, y0, y1, z0, z1)`` or ``(K, 6)``, one row per octave band from 125 Hz upwards, ``head`` (3,) the head's
    centre, ``yaw`` radians (the head looks along ``(cos yaw, sin yaw, 0)``), a source at ``distance`` metres at the
    ears' height for every azimuth of ``angles`` (degrees, counter-clockwise seen from above: positive is left),
    responses of ``taps`` samples. ``ear_model``: ``'pattern'``, an ear is a first-order receiver ``ear_pattern`` at
    ``head_radius`` from the centre, ``'sphere'``, an ear is a point on a rigid sphere of that radius, or ``'hrir'``,
    the ears are the measured pair of the ``HrirSet`` ``hrirs`` (required then, refused otherwise) at the head's
    centre, and neither ``ear_pattern`` nor ``head_radius`` is used."""

    def __init__(self, dims, beta, head, yaw, distance, angles, taps, ear_pattern=0.75, head_radius=0.0875,
                 ear_model='pattern', hrirs=None):
        self.dims = tuple(float(v) for v in dims)
        banded = np.ndim(beta) == 2
        if banded:
            self.beta = tuple(tuple(float(v) for v in row) for row in beta)
            if not 1 <= len(self.beta) <= MAX_BANDS or any(len(row) != 6 for row in self.beta):
                raise ValueError(f'beta by band is (K, 6) with 1 <= K <= {MAX_BANDS}')
        else:
            self.beta = tuple(float(v) for v in beta)
        if ear_model not in ROOM_EAR_MODELS:
            raise ValueError(f'ear_model is one of {ROOM_EAR_MODELS}, not {ear_model!r}')
        if ear_model == 'hrir' and not isinstance(hrirs, HrirSet):
            raise ValueError("ear_model='hrir' requires hrirs, an HrirSet (load_sofa, load_hrirs)")
        if ear_model != 'hrir' and hrirs is not None:
            raise ValueError(f"hrirs goes with ear_model='hrir', not with {ear_model!r}")
        self.ear_model, self.hrirs = ear_model, hrirs
        self.head = tuple(float(v) for v in head)
        self.yaw, self.distance, self.angles, self.taps = float(yaw), float(distance), \
            tuple(float(v) for v in angles), int(taps)
        self.ear_pattern, self.head_radius = float(ear_pattern), float(head_radius)
        if len(self.dims) != 3 or (not banded and len(self.beta) != 6) or len(self.head) != 3 or not self.angles:
            raise ValueError('dims and head have 3 values, beta has 6, angles at least one')

    def bands(self):
        """Octave bands of ``beta``; 0 for one coefficient per wall."""
        return len(self.beta) if np.ndim(self.beta) == 2 else 0

    def side(self):
        """Unit vector from the head's centre to the left ear."""
        return np.array([-math.sin(self.yaw), math.cos(self.yaw), 0.0])

    def front(self):
        """Unit vector along which the head looks."""
        return np.array([math.cos(self.yaw), math.sin(self.yaw), 0.0])

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
                f'ear_pattern={self.ear_pattern}, head_radius={self.head_radius}' +
                ('' if self.ear_model == 'pattern' else f', ear_model={self.ear_model!r}') +
                ('' if self.hrirs is None else f', hrirs={self.hrirs!r}') + ')')


def beta_from_rt60(dims, rt60):
    """The one reflection coefficient of all six walls that gives ``rt60`` seconds by Sabine's formula: uniform
    absorption ``alpha = 0.161 V / (S rt60)``, ``beta = sqrt(1 - alpha)``. ``ValueError`` for an ``rt60`` the room
    cannot reach (``alpha >= 1``). A sequence of ``rt60`` (one per band) gives a tuple, one value per band."""
    if np.ndim(rt60) > 0:
        return tuple(beta_from_rt60(dims, float(v)) for v in rt60)
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


# -- octave bands and the spherical head (include/rir/brever_rir_bands.h) -----------------------------
def default_band_taps(fs):
    """``N = 2^ceil(log2(fs / 62.5))``: 256 at 16 kHz, 1 024 at 48 kHz -- a bin spacing of at most 62.5 Hz, half the
    centre of the lowest band."""
    return 1 << max(math.ceil(math.log2(fs/62.5)), 1)


def band_centres(bands):
    return 125.0*2.0**np.arange(int(bands))


def band_filter_bank(fs, bands, taps=None):
    """``(K, N)`` float64: the linear-phase band filters ``g_k``. On the ``N/2 + 1`` real-DFT bins the gains are
    raised cosines on a log-frequency axis (``G_k = cos^2(pi y / 2)``, ``G_{k+1} = sin^2(pi y / 2)`` with
    ``y = log2(f / fc_k)`` between two centres; the first band is 1 below its centre, the last 1 above its own), so
    they sum to one in every bin; ``g_k = fftshift(irfft(G_k)) * hann`` with the Hann window's peak at ``N/2``, so the
    ``g_k`` sum to the unit impulse at ``N/2``."""
    K, N = int(bands), default_band_taps(fs) if taps is None else int(taps)
    fc = band_centres(K)
    if not 1 <= K <= MAX_BANDS:
        raise ValueError(f'requires 1 <= bands <= {MAX_BANDS}')
    if not fc[-1] < 0.5*fs:
        raise ValueError(f'the centre of band {K - 1}, {fc[-1]:g} Hz, is not below fs/2 = {0.5*fs:g} Hz')
    if N < 2 or N % 2 or N > MAX_FILTER:
        raise ValueError(f'requires an even number of filter taps in [2, {MAX_FILTER}]')
    f = np.arange(N//2 + 1)*(fs/N)
    G = np.zeros((K, len(f)))
    G[0, f <= fc[0]] = 1.0
    G[K - 1, f >= fc[K - 1]] = 1.0
    for k in range(K - 1):
        m = (f >= fc[k]) & (f < fc[k + 1])
        y = np.log2(f[m]/fc[k])
        G[k, m], G[k + 1, m] = np.cos(0.5*np.pi*y)**2, np.sin(0.5*np.pi*y)**2
    hann = 0.5*(1.0 + np.cos(2.0*np.pi*(np.arange(N) - N//2)/N))
    return np.fft.fftshift(np.fft.irfft(G, N, axis=1), axes=1)*hann


def head_lowpass(fs, head_radius, c=343.0):
    """The head-shadow low-pass ``1 / (1 + s / (2 w0))``, ``w0 = c / rad``, by the bilinear transform
    (``y[n] = (x[n] + x[n-1]) / (1 + kk) - (1 - kk) / (1 + kk) y[n-1]``, ``kk = fs / w0``) as a FIR of
    ``ceil(40 ln 2 / -ln |pole|)`` taps: what is cut off is below ``2^-40``."""
    kk = fs*head_radius/c
    pole = -(1.0 - kk)/(1.0 + kk)
    if not 0.0 < abs(pole) < 1.0:
        raise ValueError(f'no low-pass for fs {fs}, head radius {head_radius}, c {c}')
    M = math.ceil(40.0*math.log(2.0)/-math.log(abs(pole)))
    lp = np.empty(M)
    lp[0] = 1.0/(1.0 + kk)
    if M > 1:
        lp[1:] = lp[0]*(1.0 + pole)*pole**np.arange(M - 1)
    return lp


_FILTERS = {}


def band_filters(fs, bands, ear_model='pattern', head_radius=0.0875, c=343.0, taps=None):
    """``(filters, pad)``: the ``(C, M_f)`` float64 channel filters of ``brv_rir_bands_combine`` and ``pad = N/2``.
    Pattern mode: channel ``k`` is ``g_k``. Sphere mode: channel ``k`` is ``g_k`` and channel ``K + k`` is ``g_k``
    convolved with the head's low-pass. ``M_f`` is padded with zeros to a multiple of 16. Cached per argument set;
    the array is read-only."""
    N = default_band_taps(fs) if taps is None else int(taps)
    sphere = EAR_MODELS[ear_model] == SPHERE
    key = (float(fs), int(bands), N, float(head_radius) if sphere else None, float(c) if sphere else None)
    if key not in _FILTERS:
        g = band_filter_bank(fs, bands, N)
        rows = list(g)
        if sphere:
            lp = head_lowpass(fs, head_radius, c)
            rows += [np.convolve(row, lp) for row in g]
        longest = max(len(row) for row in rows)
        m_f = -(-longest//FILTER_MULTIPLE)*FILTER_MULTIPLE
        if m_f > MAX_FILTER:
            raise ValueError(f'the channel filters have {longest} taps, more than {MAX_FILTER}')
        filters = np.zeros((len(rows), m_f))
        for i, row in enumerate(rows):
            filters[i, :len(row)] = row
        filters.setflags(write=False)
        _FILTERS[key] = (filters, N//2)
    return _FILTERS[key]


def _band_geom_row(dims, beta, source, receiver, orientation, pattern):
    row = np.zeros(BANDS_GEOM_DOUBLES)
    row[0:3], row[3:6], row[6:9], row[9:12], row[12] = dims, source, receiver, orientation, pattern
    beta = np.asarray(beta, dtype=np.float64).reshape(-1, 6)
    row[13:13 + beta.size] = beta.ravel()
    return row


def band_opts(fs, bands, ear_model='pattern', head_radius=0.0875, window=None, c=343.0, pad=None):
    """The seven options of the band entry points as the library takes them."""
    if ear_model not in EAR_MODELS:
        raise ValueError(f'ear_model is one of {sorted(EAR_MODELS)}, not {ear_model!r}')
    opts = np.array([fs, c, default_window(fs) if window is None else window, bands, EAR_MODELS[ear_model],
                     head_radius, default_band_taps(fs)//2 if pad is None else pad], dtype=np.float64)
    assert len(opts) == BANDS_OPT_DOUBLES
    return opts


def build_band_tables(geom, shape, opts, max_order=-1):
    """The two host steps of the band entry points for ``geom`` (J, 61) float64, ``shape`` (J, 3) int64 and ``opts``
    of ``band_opts``: ``(rows, index)`` with rows of ``3 + K`` doubles; ``index[:, 7]`` is where a job's channel rows
    begin in the scratch. Refused values raise with the library's message."""
    geom = np.ascontiguousarray(geom, dtype=np.float64).reshape(-1, BANDS_GEOM_DOUBLES)
    shape = np.ascontiguousarray(shape, dtype=np.int64).reshape(-1, SHAPE_WORDS)
    jobs = len(geom)
    if len(shape) != jobs:
        raise ValueError('one shape row per job')
    n_rows = bands_query('brv_rir_bands_table_rows', geom.ctypes.data, shape.ctypes.data, jobs, opts.ctypes.data,
                         max_order)
    rows = np.empty((n_rows, 3 + int(opts[3])), dtype=np.float64)
    index = np.empty((jobs, INDEX_WORDS), dtype=np.int64)
    bands_call('brv_rir_bands_build_tables', geom.ctypes.data, shape.ctypes.data, jobs, opts.ctypes.data, max_order,
               rows.ctypes.data, index.ctypes.data, n_rows)
    return rows, index


def channels_of(opts):
    return int(opts[3])*(2 if int(opts[4]) == SPHERE else 1)


def launch_bands(tables, index, opts, max_order, max_taps, scratch, filters, out):
    """``brv_rir_bands_channels`` and ``brv_rir_bands_combine`` on the current stream; everything but ``opts`` on the
    device of ``out``."""
    hip.require_device(tables, index, scratch, filters, out)
    bands_call('brv_rir_bands_channels', tables, index, len(index), len(tables), int(max_taps), opts.ctypes.data,
               int(max_order), scratch, scratch.numel(), hip.stream())
    bands_call('brv_rir_bands_combine', scratch, scratch.numel(), index, len(index), int(max_taps),
               opts.ctypes.data, filters, filters.shape[1], out, out.numel(), hip.stream())


def chunk_jobs(taps, channels, pad, scratch_bytes):
    """``[(first, end), ...]``: consecutive jobs whose channel rows (``channels * (taps + pad)`` doubles each) stay
    within ``scratch_bytes`` together; a job that alone is larger has a chunk of its own."""
    chunks, first, used = [], 0, 0
    for j, t in enumerate(taps):
        need = 8*channels*(int(t) + pad)
        if j > first and used + need > scratch_bytes:
            chunks.append((first, j))
            first, used = j, 0
        used += need
    chunks.append((first, len(taps)))
    return chunks


def _run_bands(geom, shape, out, fs, bands, ear_model, head_radius, window, max_order, c, scratch_bytes,
               band_taps=None):
    """Tables, upload and the launch pair, chunk by chunk, into the flat fp32 ``out`` on the device."""
    max_order, scratch_bytes = int(max_order), int(scratch_bytes)
    if scratch_bytes < 1:
        raise ValueError('scratch_bytes must be positive')
    filters, pad = band_filters(fs, bands, ear_model, head_radius, c, band_taps)
    opts = band_opts(fs, bands, ear_model, head_radius, window, c, pad)
    geom, shape = np.asarray(geom, dtype=np.float64), np.asarray(shape, dtype=np.int64)
    channels = channels_of(opts)
    with torch.cuda.device(out.device):
        filters_d = torch.tensor(filters, device=out.device)         # (a copy: the cached array is read-only)
        for first, end in chunk_jobs(shape[:, 0], channels, pad, scratch_bytes):
            rows, index = build_band_tables(geom[first:end], shape[first:end], opts, max_order)
            scratch = torch.empty(int(index[-1, 7]) + channels*(int(index[-1, 4]) + pad), dtype=torch.float64,
                                  device=out.device)
            launch_bands(torch.from_numpy(rows).to(out.device), torch.from_numpy(index).to(out.device), opts,
                         max_order, index[:, 4].max(), scratch, filters_d, out)


# -- a measured ear (include/rir/brever_rir_hrir.h) ---------------------------------------------------
def _hrir_geom_row(dims, beta, source, head, front, left):
    row = np.zeros(HRIR_GEOM_DOUBLES)
    row[0:3], row[3:6], row[6:9], row[9:12], row[12:15] = dims, source, head, front, left
    beta = np.asarray(beta, dtype=np.float64).reshape(-1, 6)
    row[15:15 + beta.size] = beta.ravel()
    return row


def hrir_opts(fs, bands, hrirs, window=None, c=343.0, pad=None):
    """The seven options of the measured-ear entry points as the library takes them, for the ``HrirSet`` ``hrirs``."""
    opts = np.array([fs, c, default_window(fs) if window is None else window, bands,
                     default_band_taps(fs)//2 if pad is None else pad, len(hrirs), hrirs.taps], dtype=np.float64)
    assert len(opts) == HRIR_OPT_DOUBLES
    return opts


def build_hrir_tables(geom, shape, opts, directions, max_order=-1):
    """The two host steps of the measured-ear entry points for ``geom`` (J, 63) float64, ``shape`` (J, 4) int64,
    ``opts`` of ``hrir_opts`` and ``directions`` (D, 3): ``(rows, index, ear_index)``. ``index[:, 5]`` and
    ``index[:, 7]`` are where a job's rows begin in the direction scratch and in the fold scratch; ``ear_index``
    (2 J, 8) holds one job of ``brv_rir_bands_combine`` per (job, ear). Refused values raise with the library's
    message."""
    geom = np.ascontiguousarray(geom, dtype=np.float64).reshape(-1, HRIR_GEOM_DOUBLES)
    shape = np.ascontiguousarray(shape, dtype=np.int64).reshape(-1, HRIR_SHAPE_WORDS)
    directions = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    jobs = len(geom)
    if len(shape) != jobs:
        raise ValueError('one shape row per job')
    if len(directions) != int(opts[5]):
        raise ValueError('opts holds another number of directions')
    n_rows = hrir_query('brv_rir_hrir_table_rows', geom.ctypes.data, shape.ctypes.data, jobs, opts.ctypes.data,
                        directions.ctypes.data, max_order)
    rows = np.empty((n_rows, 3 + int(opts[3])), dtype=np.float64)
    index = np.empty((jobs, INDEX_WORDS), dtype=np.int64)
    ear_index = np.empty((2*jobs, INDEX_WORDS), dtype=np.int64)
    hrir_call('brv_rir_hrir_build_tables', geom.ctypes.data, shape.ctypes.data, jobs, opts.ctypes.data,
              directions.ctypes.data, max_order, rows.ctypes.data, index.ctypes.data, ear_index.ctypes.data, n_rows)
    return rows, index, ear_index


def padded_hrirs(hrirs):
    """``(D, 2, n_filter)`` float64: the responses of an ``HrirSet`` padded with zeros to a multiple of 16 taps, as
    ``brv_rir_hrir_fold`` takes them."""
    D, _, taps = hrirs.hrirs.shape
    out = np.zeros((D, 2, -(-taps//FILTER_MULTIPLE)*FILTER_MULTIPLE))
    out[:, :, :taps] = hrirs.hrirs
    return out


def launch_hrir(tables, index, ear_index, opts, combine_opts, max_order, max_taps, directions, responses,
                dir_scratch, fold_scratch, filters, out):
    """``brv_rir_hrir_channels``, ``brv_rir_hrir_fold`` and ``brv_rir_bands_combine`` on the current stream;
    everything but the two ``opts`` on the device of ``out``."""
    hip.require_device(tables, index, ear_index, directions, responses, dir_scratch, fold_scratch, filters, out)
    hrir_call('brv_rir_hrir_channels', tables, index, len(index), len(tables), int(max_taps), opts.ctypes.data,
              int(max_order), directions, dir_scratch, dir_scratch.numel(), hip.stream())
    hrir_call('brv_rir_hrir_fold', dir_scratch, dir_scratch.numel(), index, len(index), int(max_taps),
              opts.ctypes.data, responses, responses.shape[2], fold_scratch, fold_scratch.numel(), hip.stream())
    bands_call('brv_rir_bands_combine', fold_scratch, fold_scratch.numel(), ear_index, len(ear_index), int(max_taps),
               combine_opts.ctypes.data, filters, filters.shape[1], out, out.numel(), hip.stream())


def _run_hrir(geom, shape, out, fs, bands, hrirs, window, max_order, c, scratch_bytes, band_taps=None):
    """Tables, upload and the three launches, chunk by chunk, into the flat fp32 ``out`` on the device. A chunk's
    jobs keep their direction rows (``K D (taps + pad)`` doubles each) and their fold rows (``2 K (taps + pad)``)
    within ``scratch_bytes`` together."""
    max_order, scratch_bytes = int(max_order), int(scratch_bytes)
    if scratch_bytes < 1:
        raise ValueError('scratch_bytes must be positive')
    filters, pad = band_filters(fs, bands, 'pattern', c=c, taps=band_taps)
    opts = hrir_opts(fs, bands, hrirs, window, c, pad)
    combine_opts = band_opts(fs, bands, 'pattern', 0.0, window, c, pad)
    geom, shape = np.asarray(geom, dtype=np.float64), np.asarray(shape, dtype=np.int64)
    D = len(hrirs)
    with torch.cuda.device(out.device):
        filters_d = torch.tensor(filters, device=out.device)         # (a copy: the cached array is read-only)
        directions_d = torch.tensor(hrirs.directions, device=out.device)
        responses_d = torch.from_numpy(padded_hrirs(hrirs)).to(out.device)
        for first, end in chunk_jobs(shape[:, 0], bands*(D + 2), pad, scratch_bytes):
            rows, index, ear_index = build_hrir_tables(geom[first:end], shape[first:end], opts, hrirs.directions,
                                                       max_order)
            last = int(index[-1, 4]) + pad
            dir_scratch = torch.empty(int(index[-1, 5]) + bands*D*last, dtype=torch.float64, device=out.device)
            fold_scratch = torch.empty(int(index[-1, 7]) + 2*bands*last, dtype=torch.float64, device=out.device)
            launch_hrir(torch.from_numpy(rows).to(out.device), torch.from_numpy(index).to(out.device),
                        torch.from_numpy(ear_index).to(out.device), opts, combine_opts, max_order,
                        index[:, 4].max(), directions_d, responses_d, dir_scratch, fold_scratch, filters_d, out)


def _device(device):
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'brever_amd kernels run on a ROCm device only; got {device} (there is no CPU fallback)')
    return device


def simulate_rirs(dims, beta, sources, receivers, orientations, patterns, taps, fs, window=None, max_order=-1,
                  c=343.0, device='cuda', scratch_bytes=1 << 30, band_taps=None, ear_model='pattern',
                  head_radius=0.0875):
    """Responses of one room from every source to every receiver: ``sources`` (S, 3), ``receivers`` (R, 3),
    ``orientations`` (R, 3) unit vectors, ``patterns`` (R,) in [0, 1] (1 omni, 0.5 cardioid). Returns a
    ``(S, R, taps)`` float32 tensor on ``device``. ``beta`` is (6,) or, by octave band, ``(K, 6)``: the responses of
    the bands are then accumulated together and filtered (``band_filters``), with at most ``scratch_bytes`` of
    channel rows on the device at a time. With ``ear_model='sphere'`` a receiver is the centre of a head of
    ``head_radius``, its orientation the outward axis of the ear, and ``patterns`` is not used."""
    sources, receivers, orientations = (np.asarray(v, dtype=np.float64).reshape(-1, 3)
                                        for v in (sources, receivers, orientations))
    patterns = np.asarray(patterns, dtype=np.float64).reshape(-1)
    if ear_model == 'hrir':
        raise ValueError("simulate_rirs returns (S, R, taps), which has no ear axis: a measured ear "
                         "(ear_model='hrir') is simulated by simulate_brirs with ShoeboxRoom(..., hrirs=SET)")
    if not len(receivers) == len(orientations) == len(patterns):
        raise ValueError('one orientation and one pattern per receiver')
    taps = int(taps)
    if np.ndim(beta) == 2 or ear_model != 'pattern':
        geom = [_band_geom_row(dims, beta, s, receivers[i], orientations[i], patterns[i])
                for s in sources for i in range(len(receivers))]
        shape = [(taps, j*taps, 1) for j in range(len(geom))]
        out = torch.zeros(len(geom)*taps, dtype=torch.float32, device=_device(device))
        _run_bands(geom, shape, out, fs, len(np.reshape(beta, (-1, 6))), ear_model, head_radius, window, max_order, c,
                   scratch_bytes, band_taps)
        return out.view(len(sources), len(receivers), taps)
    geom = [_geom_row(dims, beta, s, receivers[i], orientations[i], patterns[i])
            for s in sources for i in range(len(receivers))]
    shape = [(taps, j*taps, 1) for j in range(len(geom))]
    out = _run(np.array(geom), np.array(shape), fs, window, max_order, c, device)
    return out.view(len(sources), len(receivers), taps)


def simulate_brirs(rooms, fs=16000, window=None, max_order=-1, c=343.0, device='cuda', scratch_bytes=1 << 30):
    """The BRIRs of every ``ShoeboxRoom`` of ``rooms``: a list of rooms, each a list with one ``(taps, 2)`` float32
    array (left, right) per angle -- the ``brirs=`` argument of ``PoolMixtureMaker``. The rooms with one coefficient
    per wall and ``ear_model='pattern'`` take one launch of ``brv_rir_simulate``; the others are grouped by
    ``(bands, ear_model, head_radius)`` and take one launch pair of the band entry points per group and per chunk of
    jobs whose channel rows fit ``scratch_bytes``. The rooms with ``ear_model='hrir'`` are grouped by ``(bands, set)``,
    a set of another ``fs`` is resampled (``HrirSet.resample``), one job is one (room, angle) and gives both ears, and
    a chunk takes three launches: the direction rows, their fold with the HRIRs, and the band filters; both
    scratches count against ``scratch_bytes``. The responses keep the onset delay of the measured HRIRs."""
    rooms = list(rooms)
    plain, groups, measured = [], {}, {}
    for i, room in enumerate(rooms):
        if room.ear_model == 'hrir':
            measured.setdefault((max(room.bands(), 1), id(room.hrirs)), []).append(i)
        elif room.bands() == 0 and room.ear_model == 'pattern':
            plain.append(i)
        else:
            groups.setdefault((max(room.bands(), 1), room.ear_model, room.head_radius), []).append(i)
    out = [None]*len(rooms)

    def jobs(members, row):
        """``geom``, ``shape`` and the output length of the rooms ``members``: per angle two jobs, interleaved."""
        geom, shape, at = [], [], 0
        for i in members:
            room = rooms[i]
            ears, side = room.ears(), room.side()
            for angle in room.angles:
                source = room.source(angle)
                for e in range(2):
                    # the sphere's receiver is the head's centre, and the ear is where its axis leaves the sphere
                    geom.append(row(room.dims, room.beta, source, room.head if room.ear_model == 'sphere' else ears[e],
                                    side if e == 0 else -side, room.ear_pattern))
                    shape.append((room.taps, at + e, 2))
                at += 2*room.taps
        return np.array(geom), np.array(shape), at

    def split(members, flat):
        at = 0
        for i in members:
            room = rooms[i]
            out[i] = [flat[at + 2*room.taps*k:at + 2*room.taps*(k + 1)].reshape(room.taps, 2)
                      for k in range(len(room.angles))]
            at += 2*room.taps*len(room.angles)

    if plain:
        geom, shape, _ = jobs(plain, _geom_row)
        split(plain, _run(geom, shape, fs, window, max_order, c, device).cpu().numpy())
    for (bands, ear_model, head_radius), members in groups.items():
        geom, shape, length = jobs(members, _band_geom_row)
        flat = torch.zeros(length, dtype=torch.float32, device=_device(device))
        _run_bands(geom, shape, flat, fs, bands, ear_model, head_radius, window, max_order, c, scratch_bytes)
        split(members, flat.cpu().numpy())
    for (bands, _), members in measured.items():
        geom, shape, at = [], [], 0
        for i in members:
            room = rooms[i]
            for angle in room.angles:
                geom.append(_hrir_geom_row(room.dims, room.beta, room.source(angle), room.head, room.front(),
                                           room.side()))
                shape.append((room.taps, at, 2, 1))
                at += 2*room.taps
        flat = torch.zeros(at, dtype=torch.float32, device=_device(device))
        _run_hrir(np.array(geom), np.array(shape), flat, fs, bands, rooms[members[0]].hrirs.resample(fs, device),
                  window, max_order, c, scratch_bytes)
        split(members, flat.cpu().numpy())
    return out


def random_rooms(n, seed, dims=((3, 3, 2.4), (10, 8, 4)), rt60=(0.2, 0.8), distance=(0.5, 3.0),
                 angles=range(-90, 91, 10), margin=0.3, taps=None, fs=16000, ear_pattern=0.75, head_radius=0.0875,
                 bands=0, band_tilt=(0.0, 0.25), ear_model='pattern', hrirs=None):
    """``n`` rooms drawn from ``np.random.default_rng([seed])``, a function of the arguments only. Per room, in this
    order: the three dimensions uniformly between ``dims[0]`` and ``dims[1]``; the source distance uniformly in
    ``distance``, capped so that a circle of that radius plus ``head_radius + margin`` fits the floor plan; the
    head's centre uniformly where that circle stays inside (no rejection); the ears' height uniformly in
    ``[1.0, min(1.8, Lz - margin)]``; the yaw uniformly in [0, 2 pi); ``rt60`` uniformly in its range, raised to 1.01
    times the least that Sabine's formula allows the room. ``taps`` defaults to ``ceil(rt60 fs)``.

    With ``bands = K > 0`` the walls get one coefficient per octave band: a tilt ``u`` per room, uniform in
    ``band_tilt`` from a generator of its own (``np.random.default_rng([seed, 1])``, so that nothing above changes),
    ``rt60_k = max(rt60 2^(-u (k - 2)), 1.01 min_rt60)`` (the drawn ``rt60`` holds at 500 Hz and falls by ``u``
    octaves per octave) and all six walls of a band from Sabine's formula. ``ear_model`` and ``hrirs`` (the
    ``HrirSet`` of ``ear_model='hrir'``) go to every room; neither changes a draw."""
    rng = np.random.default_rng([int(seed)])
    tilt_rng = np.random.default_rng([int(seed), 1])
    bands = int(bands)
    if not 0 <= bands <= MAX_BANDS:
        raise ValueError(f'requires 0 <= bands <= {MAX_BANDS}')
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
        beta = (beta_from_rt60(L, t60),)*6
        if bands:
            u = float(tilt_rng.uniform(band_tilt[0], band_tilt[1]))
            t60_bands = tuple(max(t60*2.0**(-u*(k - 2)), 1.01*min_rt60(L)) for k in range(bands))
            beta = tuple((b,)*6 for b in beta_from_rt60(L, t60_bands))
        rooms.append(ShoeboxRoom(L, beta, (hx, hy, hz), yaw, rho, angles,
                                 math.ceil(t60*fs) if taps is None else taps, ear_pattern, head_radius, ear_model,
                                 hrirs))
        rooms[-1].rt60 = t60
        if bands:
            rooms[-1].rt60_bands = t60_bands
    return rooms


def save_pool(path, brirs, speech=(), noises=()):
    """Write the ``.npz`` that ``PoolMixtureMaker(path, ...)`` reads: ``brir_<room>_<angle>``, ``speech_<i>``,
    ``noise_<i>``."""
    arrays = {f'brir_{r}_{a}': np.asarray(h, dtype=np.float32) for r, room in enumerate(brirs)
              for a, h in enumerate(room)}
    arrays.update({f'speech_{i}': np.asarray(x, dtype=np.float32) for i, x in enumerate(speech)})
    arrays.update({f'noise_{i}': np.asarray(x, dtype=np.float32) for i, x in enumerate(noises)})
    np.savez(path, **arrays)
