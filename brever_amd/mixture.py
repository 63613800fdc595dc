"""Batched mixture synthesis on the GPU: ``brever.mixture.mixture.Mixture`` for a batch of ragged mixtures.

The reference builds one mixture at a time on the CPU (``RandomMixtureMaker.make_from_metadata``): add_speech
with the early / late windows of ``split_brir``, add_noises, the diffuse sum, set_ndr, set_snr over
``speech_idx``, set_tmr, ``set_rms(get_rms() + jitter)`` -- six or more long ``oaconvolve`` calls. Here a whole
batch goes through one fixed launch sequence with no host round trip (the gains stay on the device):

    gather signals / BRIRs from pools, split_brir        brv_mix_pack_signals, brv_mix_pack_brirs
    block DFTs of signals and BRIR partitions            brv_dft64_forward   (main library, fp64 matrix pipe)
    per-bin partition multiply-accumulate, both ears     brv_mix_partition_mac
    inverse block DFTs, the valid half only              brv_dft64_synthesis
    energy sums in fp64, gains and labels                brv_mix_energies, brv_mix_gains
    gain-and-sum of the requested components             brv_mix_compose

The convolution is a uniformly partitioned overlap-save product with block ``B``: frames of ``2B`` samples at
hop ``B``; the BRIR partitions are transformed with the first ``B`` columns of the same DFT basis (their zero
padding costs nothing) and only the last ``B`` samples of every output frame are synthesised.

Reference quirks kept: every spatialised signal is truncated to its input length; with ``padding > 0`` the
speech is padded before AND after spatialisation, so a target of L samples gives L + 4 n_pad and ``speech_idx =
(n_pad, n_pad + L)``; energies are those of the channel mean; a zero target or noise energy is a ValueError
(raised by ``MixtureBatch.check``, after the batch has run).

``PoolMixtureMaker`` plugs this into ``BreverDataset(dynamic_mixing=True)`` (``data.set_mixture_maker``).
There is no CPU fallback: without ``libbrever_mix.so`` or a ROCm device the calls raise.
"""
import collections
import os
import time

import numpy as np
import torch

from . import hip

COMPONENTS = ('mixture', 'foreground', 'background', 'speech', 'noise', 'early_speech', 'late_speech',
              'dir_noise', 'diffuse')

# the brv_mix_* entry points of include/brever_mix.h
_LIB = hip.Library('brever_mix.h', 'libbrever_mix.so', 'BRV_MIX_LIB_PATH', 'The mixture engine has no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES, lib, call = _LIB.path, _LIB.header_path, _LIB.signatures, _LIB.lib, _LIB.call
EN_CHUNK = _LIB.constants['BRV_MIX_ENERGY_CHUNK']       # samples per partial energy sum
MAX_PARTS = _LIB.constants['BRV_MIX_MAX_PARTS']         # partitions per impulse response the product's LDS tile holds
# the brv_mixfx_* entry points of include/brever_mixfx.h: colouring, LTAS matching, BRIR decay
_FX = hip.Library('brever_mixfx.h', 'libbrever_mixfx.so', 'BRV_MIXFX_LIB_PATH',
                  'The mixture engine has no CPU fallback.')
FX_LIB_PATH, FX_HEADER_PATH, FX_SIGNATURES = _FX.path, _FX.header_path, _FX.signatures
fx_lib, fx_call = _FX.lib, _FX.call


_tables = {}


def dft_tables(block, device):
    """float64 DFT bases of the overlap-save transform of size ``2*block``, rows (re_k, im_k) interleaved as
    ``brv_dft64_forward`` takes them: ``signal`` (2 bins, 2B) for the signal frames, ``partition`` (2 bins, B) =
    its first B columns (a partition is B taps and B zeros), ``inverse`` (2 bins, B) = the columns of the
    inverse one-sided transform for the last B samples of a frame (the ones overlap-save keeps)."""
    key = (int(block), str(device))
    if key not in _tables:
        n, bins = 2*block, block + 1
        k = np.arange(bins)[:, None]
        m = np.arange(n)[None, :]
        ang = 2*np.pi*((k*m) % n)/n
        fwd = np.empty((2*bins, n))
        fwd[0::2], fwd[1::2] = np.cos(ang), -np.sin(ang)
        w = np.full((bins, 1), 2.0/n)
        w[0] = w[-1] = 1.0/n
        inv = np.empty((2*bins, n))
        inv[0::2], inv[1::2] = w*np.cos(ang), -w*np.sin(ang)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
        _tables[key] = dict(signal=up(fwd), partition=up(fwd[:, :block]), inverse=up(inv[:, block:]))
    return _tables[key]


class MixtureBatch:
    """What one batch gave, all on the device: ``components[name]`` (mixtures, max length, 2) float32 with
    zeros behind each mixture's length, ``lengths`` and ``speech_idx`` (host lists), ``labels`` (mixtures, 3)
    float64 = (tmr, tnr, trr), ``gains`` (mixtures, 8) float64 = the factors of (early, late, dir, diffuse) and
    the reference's (ndr, snr, tmr, rms) gains, ``status`` (mixtures) int32."""

    def __init__(self, components, lengths, speech_idx, labels, gains, status):
        self.components, self.lengths, self.speech_idx = components, lengths, speech_idx
        self.labels, self.gains, self.status = labels, gains, status

    def check(self):
        """Wait for the batch and raise the reference's ValueError for a zero energy."""
        return self.raise_for(self.status.cpu().tolist())

    def raise_for(self, status):
        """The same for status words already on the host."""
        for i, st in enumerate(status):
            if st == 1:
                raise ValueError(f'mixture {i}: cannot scale noise signal if target signal is 0')
            if st == 2:
                raise ValueError(f'mixture {i}: cannot scale noise signal if it equals 0')
            if st in (3, 4):                       # a BRIR decay job of the mixture (PoolMixtureMaker)
                raise ValueError(f'mixture {i}: {DECAY_MESSAGES[st]}')
        return self

    def item(self, i, name):
        """Component ``name`` of mixture ``i``, (frames, 2)."""
        return self.components[name][i, :self.lengths[i]]


def _nan(v):
    return float('nan') if v is None else float(v)


# -- signal effects: colored_noise, match_ltas / calc_ltas, BRIRDecay ---------------------------------------------
COLORS = dict(brown=2, pink=1, white=0, blue=-1, violet=-2)      # alpha of the 1/f**alpha power spectral density
N_FFT, HOP = 512, 256                                              # the reference's match_ltas / calc_ltas framing


def _up(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(device, non_blocking=True)


class FilterCache:
    """Device-resident colouring filters ``h_m = irfft(s, m)`` per ``(colour, m)``, least recently used out first
    once ``max_bytes`` are held. A miss costs a float64 inverse FFT of ``m`` points on the host (``taps``);
    ``miss_seconds`` adds up what the misses took there, upload call included."""

    def __init__(self, max_bytes=256 << 20):
        self.max_bytes, self.bytes, self.hits, self.misses, self.miss_seconds = int(max_bytes), 0, 0, 0, 0.0
        self._held = collections.OrderedDict()

    @staticmethod
    def taps(color, m):
        """``h_m = irfft(s, m)`` in float64, rounded to float32: ``s_k = (k/m)^(-alpha/2)``, ``s_0 := s_1``."""
        f = np.arange(m//2 + 1)/m
        f[0] = f[1]
        return np.fft.irfft(f**(-COLORS[color]/2), m).astype(np.float32)

    def get(self, color, m, device):
        key = (color, int(m), str(device))
        h = self._held.get(key)
        if h is not None:
            self._held.move_to_end(key)
            self.hits += 1
            return h
        self.misses += 1
        t0 = time.perf_counter()
        h = torch.from_numpy(self.taps(color, int(m))).to(device)
        self.miss_seconds += time.perf_counter() - t0
        self._held[key] = h
        self.bytes += 4*int(m)
        while self.bytes > self.max_bytes and len(self._held) > 1:
            _, old = self._held.popitem(last=False)
            self.bytes -= 4*old.numel()
        return h

    def clear(self):
        self._held.clear()
        self.bytes = 0


color_filters = FilterCache()


def colorize_rows(pool, rows, block=256, dst=None, dst_offsets=None, cache=None):
    """``colored_noise`` on white rows of ``pool`` (1-D float32 device tensor). ``rows``: ``(src, m, colour)``, no
    colour white. The circular convolution ``irfft(rfft(x) s, m)`` is the linear one of the periodic extension
    ``[x, x]`` with the ``m`` taps ``h_m = irfft(s, m)``, samples ``[m, 2m)``: one partitioned overlap-save product
    per row (the ear pair of the product kernel is ``(h_m, zeros)``). The coloured rows go to ``dst`` at
    ``dst_offsets`` (default: a new tensor, back to back). Returns ``(dst, dst_offsets)``.

    Only the taps are cached: the zero-padded filter rows and their block DFTs are rebuilt per call. Working set of
    a call with ``R`` rows of at most ``m`` samples, ``F = ceil(2m/B)``: ``R F (B+1) 8`` bytes of signal spectra,
    twice that of output spectra (the ear pair), ``8 R F B`` of output rows -- about 4.1 MB per row at 4 s and block
    256, 21 MB per row for a decay tail of 163 200 samples (block 512)."""
    hip.require_device(pool, dst)
    cache = color_filters if cache is None else cache
    device, B, R = pool.device, int(block), len(rows)
    if not 1 <= R <= 32767:
        raise ValueError('needs 1 to 32767 rows')
    for src, m, color in rows:
        if color not in COLORS or color == 'white':
            raise ValueError(f'colour must be one of {sorted(set(COLORS) - {"white"})}, got {color!r}')
        if m < 2 or src < 0 or src + m > pool.numel():
            raise ValueError('a row has fewer than 2 samples or lies outside the pool')
    Pmax = max(-(-m//B) for _, m, _ in rows)
    if Pmax > MAX_PARTS:
        raise ValueError(f'a coloured signal spans {Pmax} blocks of {B}; at most {MAX_PARTS}: use a larger block')
    if dst is None:
        dst_offsets = np.cumsum([0] + [m for _, m, _ in rows]).tolist()[:-1]
        dst = torch.empty(sum(m for _, m, _ in rows), dtype=torch.float32, device=device)
    for (_, m, _), off in zip(rows, dst_offsets):
        if off < 0 or off + m > dst.numel():
            raise ValueError('a coloured row lies outside dst')
    F = max(-(-2*m//B) for _, m, _ in rows)
    bins, st, tb = B + 1, hip.stream(), dft_tables(B, device)
    f32 = dict(dtype=torch.float32, device=device)
    xs = torch.empty(R, F*B, **f32)
    fx_call('brv_mixfx_pack_periodic', pool, _up([r[:2] for r in rows], np.int64, device), xs, pool.numel(), R,
            F*B, st)
    filters = {}
    for _, m, color in rows:
        filters.setdefault((color, m), len(filters))
    U = len(filters)
    hs = torch.zeros(2*U, Pmax*B, **f32)
    for (color, m), u in filters.items():
        hs[2*u, :m] = cache.get(color, m, device)
    xspec = torch.empty(R, bins, F, 2, **f32)
    hip.call('brv_dft64_forward', xs, tb['signal'], xspec, R, F*B, 2*B, B, B, F, bins, 1.0, 1.0, st)
    hspec = torch.empty(2*U, bins, Pmax, 2, **f32)
    hip.call('brv_dft64_forward', hs, tb['partition'], hspec, 2*U, Pmax*B, B, B, 0, Pmax, bins, 1.0, 1.0, st)
    slots = [(r, r + 1, -(-2*m//B)) for r, (_, m, _) in enumerate(rows)]
    jobs = [(r, 2*filters[(color, m)], -(-m//B)) for r, (_, m, color) in enumerate(rows)]
    yspec = torch.empty(2*R, bins, F, 2, **f32)
    call('brv_mix_partition_mac', xspec, hspec, yspec, _up(slots, np.int32, device), _up(jobs, np.int32, device), R,
         R, R, F, 2*U, Pmax, bins, F, Pmax, st)
    y = torch.empty(2*R, F*B, **f32)
    hip.call('brv_dft64_synthesis', yspec, tb['inverse'], y, 2*R, F, B, bins, 1.0, 1.0, st)
    copies = [(2*r, m, m, off, m) for r, ((_, m, _), off) in enumerate(zip(rows, dst_offsets))]
    fx_call('brv_mixfx_copy_rows', y, _up(copies, np.int64, device), dst, R, 2*R, F*B, dst.numel(), st)
    return dst, list(dst_offsets)


def colorize(xs, color, block=256):
    """``colored_noise(color, len(x))`` with ``x`` as its white draw, for a list of 1-D device tensors; ``color`` one
    name or one per tensor. White is the identity."""
    colors = [color]*len(xs) if isinstance(color, str) else list(color)
    for c in colors:
        if c not in COLORS:
            raise ValueError(f'color must be either one of {tuple(COLORS)}')
    flat = [x.reshape(-1).float() for x in xs]
    todo = [i for i, c in enumerate(colors) if c != 'white']
    out = list(flat)
    if todo:
        off = np.cumsum([0] + [flat[i].numel() for i in todo]).tolist()
        res, at = colorize_rows(torch.cat([flat[i] for i in todo]),
                                [(off[k], flat[i].numel(), colors[i]) for k, i in enumerate(todo)], block)
        for k, i in enumerate(todo):
            out[i] = res[at[k]:at[k] + flat[i].numel()]
    return out


_ltas_tabs = {}


def ltas_tables(device):
    """The bases of the reference's STFT pair (periodic Hann of 512 at hop 256), window and window sum folded in:
    ``forward`` (2 bins, 512) gives spectrum / window sum, ``inverse`` (2 bins, 512) the inverse transform times
    window times window sum; ``window`` float32 for the overlap-add's envelope."""
    key = str(device)
    if key not in _ltas_tabs:
        n, bins = N_FFT, N_FFT//2 + 1
        w = 0.5 - 0.5*np.cos(2*np.pi*np.arange(n)/n)
        k = np.arange(bins)[:, None]
        ang = 2*np.pi*((k*np.arange(n)[None, :]) % n)/n
        fwd = np.empty((2*bins, n))
        fwd[0::2], fwd[1::2] = np.cos(ang)*w/w.sum(), -np.sin(ang)*w/w.sum()
        c = np.full((bins, 1), 2.0/n)
        c[0] = c[-1] = 1.0/n
        inv = np.empty((2*bins, n))
        inv[0::2], inv[1::2] = c*np.cos(ang)*w*w.sum(), -c*np.sin(ang)*w*w.sum()
        _ltas_tabs[key] = dict(forward=_up(fwd, np.float64, device), inverse=_up(inv, np.float64, device),
                               window=_up(w, np.float32, device))
    return _ltas_tabs[key]


def _ltas_frames(n):
    return -(-n//HOP) + 1


def _check_signals(x, sigs):
    R, T = x.shape
    for row0, nrows, n in sigs:
        if n < N_FFT:
            raise ValueError(f'LTAS framing needs at least {N_FFT} samples per signal, got {n}')
        if nrows not in (1, 2) or row0 < 0 or row0 + nrows > R or n > T:
            raise ValueError('a signal lies outside the rows')
    if not 1 <= len(sigs) <= 65535 or R > 65535:
        raise ValueError('needs 1 to 65535 signals and rows')


def ltas_power(x, sigs):
    """Spectra of the rows ``x`` (rows, T) float32 (zeros behind each signal's length) in the reference's framing
    and the per-signal mean ``|X|^2`` over frames and rows. ``sigs``: ``(first row, rows (1 or 2), length)``.
    Returns ``(spec, descriptors, power (signals, 257) float64, frames)``."""
    hip.require_device(x)
    _check_signals(x, sigs)
    device, (R, T), st, tab = x.device, x.shape, hip.stream(), ltas_tables(x.device)
    bins, F = N_FFT//2 + 1, max(_ltas_frames(n) for _, _, n in sigs)
    spec = torch.empty(R, bins, F, 2, dtype=torch.float32, device=device)
    hip.call('brv_dft64_forward', x, tab['forward'], spec, R, T, N_FFT, HOP, HOP, F, bins, 1.0, 1.0, st)
    d = _up([(r, k, _ltas_frames(n)) for r, k, n in sigs], np.int32, device)
    power = torch.empty(len(sigs), bins, dtype=torch.float64, device=device)
    fx_call('brv_mixfx_ltas_power', spec, d, power, len(sigs), R, bins, F, st)
    return spec, d, power, F


def match_rows(x, sigs, ltas):
    """``match_ltas`` on the signals of ``x`` (rows, T): contiguous float32, zeros behind each signal's length.
    ``sigs`` as in ``ltas_power`` (an ear pair is matched jointly); ``ltas`` (257,) float64 on the device.
    Returns a new (rows, T) tensor, zeros behind each signal's length."""
    hip.require_device(ltas)
    if ltas.dtype != torch.float64 or ltas.numel() != N_FFT//2 + 1 or not ltas.is_contiguous():
        raise ValueError(f'ltas is a contiguous float64 vector of {N_FFT//2 + 1} bins')
    spec, d, power, F = ltas_power(x, sigs)
    device, (R, T), st, tab, bins = x.device, x.shape, hip.stream(), ltas_tables(x.device), N_FFT//2 + 1
    fx_call('brv_mixfx_ltas_equalize', spec, d, power, ltas, len(sigs), R, bins, F, st)
    frames = torch.empty(R, F, N_FFT, dtype=torch.float32, device=device)
    hip.call('brv_dft64_synthesis', spec, tab['inverse'], frames, R, F, N_FFT, bins, 1.0, 1.0, st)
    y = torch.empty(R, T, dtype=torch.float32, device=device)
    hip.call('brv_overlap_add', frames, tab['window'], y, R, F, N_FFT, HOP, HOP, T, st)
    out = torch.zeros(R, T, dtype=torch.float32, device=device)
    copies = [(r0 + e, 0, n, (r0 + e)*T, T) for r0, k, n in sigs for e in range(k)]
    fx_call('brv_mixfx_copy_rows', y, _up(copies, np.int64, device), out, len(copies), R, T, R*T, st)
    return out


def _pack_rows(xs):
    """Device tensors (n,) or (n, channels <= 2) -> (rows (R, T) zero filled, sigs, shapes)."""
    cols, sigs = [], []
    for x in xs:
        x2 = x.float().reshape(x.shape[0], -1)
        if x2.shape[1] not in (1, 2):
            raise ValueError('a signal is (n,), (n, 1) or (n, 2)')
        sigs.append((len(cols), x2.shape[1], x2.shape[0]))
        cols.extend(x2[:, e].contiguous() for e in range(x2.shape[1]))
    T = max(c.numel() for c in cols)
    pool = torch.cat(cols)
    off = np.cumsum([0] + [c.numel() for c in cols]).tolist()
    rows = torch.empty(len(cols), T, dtype=torch.float32, device=pool.device)
    call('brv_mix_pack_signals', pool, _up([(off[r], c.numel(), 0) for r, c in enumerate(cols)], np.int64, pool.device),
         rows, pool.numel(), len(cols), T, hip.stream())
    return rows, sigs


def match_ltas(xs, ltas):
    """``match_ltas(x, ltas)`` of the reference for a list of device tensors (n,) or (n, 2) (the two channels share
    one equalisation); ``ltas`` 257 values (array or device tensor). Fewer than 512 samples: ValueError."""
    for x in xs:
        if x.shape[0] < N_FFT:
            raise ValueError(f'LTAS framing needs at least {N_FFT} samples per signal, got {x.shape[0]}')
    hip.require_device(*xs)
    rows, sigs = _pack_rows(xs)
    if not torch.is_tensor(ltas):
        ltas = _up(ltas, np.float64, rows.device)
    out = match_rows(rows, sigs, ltas.to(rows.device, torch.float64).contiguous())
    res = []
    for x, (r0, k, n) in zip(xs, sigs):
        y = out[r0:r0 + k, :n].T
        res.append(y.reshape(x.shape).contiguous())
    return res


def smooth_ltas(ltas, n_oct=3):
    """The reference's 1/3-octave Gaussian smoothing of bins 1.. (host, float64): column j of the kernel has the
    width of bin j and is divided by the sum of ROW j, as ``calc_ltas`` does."""
    f = np.arange(1, len(ltas))
    sigma = (f/n_oct)/np.pi
    g = np.exp(-0.5*(np.subtract.outer(f, f)/sigma)**2)/(sigma*(2*np.pi)**0.5)
    g = g/g.sum(axis=1)
    out = np.array(ltas, dtype=np.float64)
    out[1:] = g@out[1:]
    return out


def speech_ltas(xs, chunk=64):
    """``AudioFileLoader.calc_ltas`` over a list of 1-D device tensors: the sum over files of the frame-mean
    ``|X|^2`` (device, fp64), smoothed on the host. Returns 257 float64 values (NumPy)."""
    total = np.zeros(N_FFT//2 + 1)
    for i in range(0, len(xs), chunk):
        rows, sigs = _pack_rows([x.reshape(-1) for x in xs[i:i + chunk]])
        power = ltas_power(rows, sigs)[2].cpu().numpy()
        for p in power:                                     # file order: fixed
            total += p
    return smooth_ltas(total)


DECAY_MESSAGES = {1: 'cannot scale noise signal if target signal is 0', 2: 'cannot scale noise signal if it equals 0',
                  3: 'the decay tail does not have the claimed length', 4: 'a decay descriptor is out of range'}


def decay_jobs(brir_pool, noise_pool, jobs, fs=16000):
    """``BRIRDecay`` for BRIRs of ``brir_pool`` with tail noises of ``noise_pool`` (1-D float32 device tensors).
    ``jobs``: ``(brir offset, taps, noise offset, noise samples, rt60, drr, delay, claimed tail length or None)``,
    ``rt60 > 0``. Returns ``(pool of the decayed BRIRs, [(offset, n)], status (jobs) int32)``; nothing comes back
    to the host."""
    hip.require_device(brir_pool, noise_pool)
    device, desc, params, refs, total = brir_pool.device, [], [], [], 0
    for boff, taps, noff, nn, rt60, drr, delay, claimed in jobs:
        if not rt60 > 0:
            raise ValueError('rt60 must be positive (rt60 = 0 leaves the BRIR as it is)')
        n = max(int(round(2*(rt60 + delay)*fs)), taps)
        desc.append((boff, taps, noff, nn, total, n, int(round(delay*fs)), -1 if claimed is None else claimed))
        params.append((rt60, drr, fs))
        refs.append((total, n))
        total += 2*n
    out = torch.empty(total, dtype=torch.float32, device=device)
    status = torch.empty(len(jobs), dtype=torch.int32, device=device)
    fx_call('brv_mixfx_decay_brirs', brir_pool, noise_pool, _up(desc, np.int64, device),
            _up(params, np.float64, device), out, status, brir_pool.numel(), noise_pool.numel(), total, len(jobs),
            hip.stream())
    return out, refs, status


def decay_brirs(brirs, noises, rt60, drr, delay, fs=16000, tail_lengths=None):
    """``BRIRDecay(rt60, drr, delay, color, fs)(brir)`` for lists of device tensors: ``brirs[i]`` (taps, 2),
    ``noises[i]`` the tail noise (white, or coloured at the tail's length) with at least ``n - i0`` samples;
    ``rt60``, ``drr``, ``delay`` one number or one per BRIR. ``tail_lengths[i]``: the length the caller took the
    tail to have, checked on the device. Returns (n, 2) tensors; ``rt60 == 0`` returns the BRIR itself. Waits
    for the result and raises the reference's ValueError for a zero BRIR or tail."""
    K = len(brirs)
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]*K            # noqa: E731
    rt60, drr, delay = per(rt60), per(drr), per(delay)
    todo = [i for i in range(K) if rt60[i] != 0]
    out = list(brirs)
    if not todo:
        return out
    for i in todo:
        if brirs[i].dim() != 2 or brirs[i].shape[1] != 2:
            raise ValueError('a BRIR is (taps, 2)')
    hh = [brirs[i].float().reshape(-1) for i in todo]
    nn = [noises[i].float().reshape(-1) for i in todo]
    hoff = np.cumsum([0] + [h.numel() for h in hh]).tolist()
    noff = np.cumsum([0] + [x.numel() for x in nn]).tolist()
    jobs = [(hoff[k], hh[k].numel()//2, noff[k], nn[k].numel(), rt60[i], drr[i], delay[i],
             None if tail_lengths is None else tail_lengths[i]) for k, i in enumerate(todo)]
    pool, refs, status = decay_jobs(torch.cat(hh), torch.cat(nn), jobs, fs)
    for k, st in enumerate(status.cpu().tolist()):
        if st:
            raise ValueError(f'BRIR {todo[k]}: {DECAY_MESSAGES.get(st, st)}')
    for k, i in enumerate(todo):
        off, n = refs[k]
        out[i] = pool[off:off + 2*n].view(n, 2)
    return out


def synthesize(pools, brir_pool, specs, components=COMPONENTS, padding=0.0, fs=16000, reflection_boundary=50e-3,
               max_itd=1e-3, block=256, ltas=None):
    """Run one batch. ``pools``: list of 1-D float32 device tensors holding signals; ``brir_pool``: 1-D float32
    device tensor holding interleaved (taps, 2) BRIRs. ``specs``: one dict per mixture --

        target=(pool, offset, n)  brir=(offset, taps)
        noises=[((pool, offset, n), (offset, taps)), ...]        directional noises, n = the mixture's length
        diffuse=[((pool, offset, n), (offset, taps)), ...]       diffuse noise signals drawn by the caller
        ndr=, snr=, tmr=, rms_jitter=                             None / absent: step not taken (jitter 0)
        n_pad=                                                    zeros around the speech, else round(padding*fs)
        diffuse_ltas=True                                         match_ltas(diffuse, ltas) on the summed ear pair

    ``ltas``: (257,) float64 device tensor, needed when a spec asks for ``diffuse_ltas``.

    Only descriptors go to the device; nothing comes back. Returns a ``MixtureBatch``."""
    pools = list(pools)
    hip.require_device(brir_pool, *pools)
    for t in pools + [brir_pool]:
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() < 1:
            raise ValueError('pools are non-empty contiguous 1-D float32 tensors')
    comp_ids = [COMPONENTS.index(c) for c in components]
    if not specs or not comp_ids:
        raise ValueError('needs at least one mixture and one component')
    device, B = brir_pool.device, int(block)
    M = len(specs)
    sig_rows = [[] for _ in pools]      # per pool: (src, n, dst, key)
    hdesc, jobs, slots, mixd, params, lengths, idx = [], [], [], [], [], [], []
    pending = []                        # (slot jobs as (signal key, h job, parts)) resolved once rows are numbered
    for s, spec in enumerate(specs):
        pool, off, n = spec['target']
        n_pad = spec['n_pad'] if spec.get('n_pad') is not None else round(padding*fs)
        T = n + 4*n_pad
        frames = -(-T//B)
        lengths.append(T)
        idx.append((n_pad, n_pad + n))
        mixd.append((T, T - n_pad, n_pad, n_pad + n))
        params.append([_nan(spec.get('ndr')), _nan(spec.get('snr')), _nan(spec.get('tmr')),
                       float(spec.get('rms_jitter') or 0.0)])
        sig_rows[pool].append((off, n, 2*n_pad, (s, 't')))
        groups = [[], [], [], []]
        for mode, g in ((1, 0), (2, 1)):
            boff, taps = spec['brir']
            hdesc.append((boff, taps, mode))
            groups[g].append(((s, 't'), len(hdesc) - 1, min(-(-taps//B), frames)))
        for g, name in ((2, 'noises'), (3, 'diffuse')):
            for j, ((pool, off, n), (boff, taps)) in enumerate(spec.get(name) or []):
                if n != T:
                    raise ValueError(f'mixture {s}: {name}[{j}] has {n} samples, the mixture has {T}')
                sig_rows[pool].append((off, n, 0, (s, name, j)))
                hdesc.append((boff, taps, 0))
                groups[g].append(((s, name, j), len(hdesc) - 1, min(-(-taps//B), frames)))
        pending.append((groups, frames))
    for boff, taps, _ in hdesc:
        if taps < 1 or boff < 0 or boff + 2*taps > brir_pool.numel():
            raise ValueError('a BRIR lies outside brir_pool')
    row_of, r = {}, 0
    for pool, rows in enumerate(sig_rows):
        for off, n, dst, key in rows:
            if n < 1 or off < 0 or off + n > pools[pool].numel():
                raise ValueError(f'a signal lies outside pool {pool}')
            row_of[key] = r
            r += 1
    for groups, frames in pending:
        for g in groups:
            slots.append((len(jobs), len(jobs) + len(g), frames))
            jobs.extend((row_of[key], 2*h, parts) for key, h, parts in g)
    xrows, hjobs = r, len(hdesc)
    Tmax = max(lengths)
    F = -(-Tmax//B)
    Pmax = max(j[2] for j in jobs)
    if Pmax > MAX_PARTS:
        raise ValueError(f'a BRIR spans {Pmax} blocks of {B}; at most {MAX_PARTS}: use a larger block')
    if max(xrows, 2*hjobs, 8*M) > 65535:
        raise ValueError('batch too large: at most 65535 signal rows, BRIR rows and 8 x mixtures')
    bins, st = B + 1, hip.stream()
    tb = dft_tables(B, device)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(device, non_blocking=True)

    f32 = dict(dtype=torch.float32, device=device)
    xs = torch.empty(xrows, Tmax, **f32)
    r = 0
    for pool, rows in enumerate(sig_rows):
        if rows:
            d = up([row[:3] for row in rows], np.int64)
            call('brv_mix_pack_signals', pools[pool], d, xs[r:], pools[pool].numel(), len(rows), Tmax, st)
            r += len(rows)
    hs = torch.empty(2*hjobs, Pmax*B, **f32)
    call('brv_mix_pack_brirs', brir_pool, up(hdesc, np.int64), hs, brir_pool.numel(), hjobs, Pmax*B,
         round(reflection_boundary*fs), max(round(max_itd*fs), 1), st)
    xspec = torch.empty(xrows, bins, F, 2, **f32)
    hip.call('brv_dft64_forward', xs, tb['signal'], xspec, xrows, Tmax, 2*B, B, B, F, bins, 1.0, 1.0, st)
    hspec = torch.empty(2*hjobs, bins, Pmax, 2, **f32)
    hip.call('brv_dft64_forward', hs, tb['partition'], hspec, 2*hjobs, Pmax*B, B, B, 0, Pmax, bins, 1.0, 1.0, st)
    yspec = torch.empty(8*M, bins, F, 2, **f32)
    call('brv_mix_partition_mac', xspec, hspec, yspec, up(slots, np.int32), up(jobs, np.int32), 4*M, len(jobs),
         xrows, F, 2*hjobs, Pmax, bins, F, Pmax, st)
    y = torch.empty(8*M, F*B, **f32)
    hip.call('brv_dft64_synthesis', yspec, tb['inverse'], y, 8*M, F, B, bins, 1.0, 1.0, st)
    eq = [s for s, spec in enumerate(specs) if spec.get('diffuse_ltas') and spec.get('diffuse')]
    if eq:
        # the summed diffuse ear pair of a mixture, zeros from its length on, is matched jointly and put back
        if ltas is None:
            raise ValueError('a spec asks for diffuse_ltas: pass ltas')
        Td = max(lengths[s] for s in eq)
        pairs = torch.empty(2*len(eq), Td, **f32)
        d = [(8*s + 6 + e, 0, lengths[s], (2*k + e)*Td, Td) for k, s in enumerate(eq) for e in range(2)]
        fx_call('brv_mixfx_copy_rows', y, up(d, np.int64), pairs, len(d), 8*M, F*B, pairs.numel(), st)
        matched = match_rows(pairs, [(2*k, 2, lengths[s]) for k, s in enumerate(eq)], ltas)
        d = [(2*k + e, 0, lengths[s], (8*s + 6 + e)*F*B, lengths[s]) for k, s in enumerate(eq) for e in range(2)]
        fx_call('brv_mixfx_copy_rows', matched, up(d, np.int64), y, len(d), 2*len(eq), Td, y.numel(), st)
    chunks = -(-F*B//EN_CHUNK)
    mix_d = up(mixd, np.int32)
    f64 = dict(dtype=torch.float64, device=device)
    partials = torch.empty(M, chunks, 40, **f64)
    call('brv_mix_energies', y, mix_d, partials, M, F*B, chunks, st)
    gains, labels = torch.empty(M, 8, **f64), torch.empty(M, 3, **f64)
    status = torch.empty(M, dtype=torch.int32, device=device)
    call('brv_mix_gains', partials, mix_d, up(params, np.float64), gains, labels, status, M, chunks, st)
    out = torch.empty(len(comp_ids), M, Tmax, 2, **f32)
    call('brv_mix_compose', y, gains, mix_d, up(comp_ids, np.int32), out, len(comp_ids), M, F*B, Tmax, st)
    return MixtureBatch({c: out[k] for k, c in enumerate(components)}, lengths, idx, labels, gains, status)


def mix(targets, brirs, noises=None, noise_brirs=None, diffuse=None, diffuse_brirs=None, ndr=None, snr=None,
        tmr=None, rms_jitter=None, padding=0.0, fs=16000, diffuse_ltas=None, **kw):
    """``synthesize`` for lists of device tensors, one entry per mixture: ``targets[i]`` (n,), ``brirs[i]``
    (taps, 2), ``noises[i]`` / ``noise_brirs[i]`` and ``diffuse[i]`` / ``diffuse_brirs[i]`` lists of signals of
    the mixture's length and their BRIRs, ``ndr[i]`` ... ``rms_jitter[i]`` numbers or None, ``padding`` one
    number or one per mixture, ``diffuse_ltas[i]`` whether the diffuse sum is matched to ``ltas=``."""
    M = len(targets)
    sig, sig_off, hh, h_off = [], [0], [], [0]

    def add_signal(x):
        x = x.reshape(-1).float()
        sig.append(x)
        sig_off.append(sig_off[-1] + x.numel())
        return (0, sig_off[-2], x.numel())

    def add_brir(h):
        if h.dim() != 2 or h.shape[1] != 2:
            raise ValueError('a BRIR is (taps, 2)')
        hh.append(h.float().reshape(-1))
        h_off.append(h_off[-1] + 2*h.shape[0])
        return (h_off[-2], h.shape[0])

    specs = []
    for i in range(M):
        spec = dict(target=add_signal(targets[i]), brir=add_brir(brirs[i]))
        for name, xs, hs in (('noises', noises, noise_brirs), ('diffuse', diffuse, diffuse_brirs)):
            xi, hi = (xs[i] if xs else []) or [], (hs[i] if hs else []) or []
            if len(xi) != len(hi):
                raise ValueError('xs and brirs must have same number of elements')
            spec[name] = [(add_signal(x), add_brir(h)) for x, h in zip(xi, hi)]
        for name, v in (('ndr', ndr), ('snr', snr), ('tmr', tmr), ('rms_jitter', rms_jitter)):
            spec[name] = None if v is None else v[i]
        spec['diffuse_ltas'] = bool(diffuse_ltas[i]) if diffuse_ltas else False
        spec['n_pad'] = round((padding[i] if isinstance(padding, (list, tuple)) else padding)*fs)
        specs.append(spec)
    return synthesize([torch.cat(sig)], torch.cat(hh), specs, fs=fs, **kw)


class PoolMixtureMaker:
    """Mixture maker in the ``set_mixture_maker`` protocol that synthesises every epoch on the GPU from
    in-memory pools: ``speech`` and ``noises`` lists of 1-D arrays, ``brirs`` a list of rooms, each a list of
    (taps, 2) arrays (one per angle) -- passed in, or loaded from ``path`` (a ``.npz`` with ``speech_<i>``,
    ``noise_<i>``, ``brir_<room>_<angle>`` arrays).

    Per epoch a host RNG seeded with ``(seed, epoch)`` draws, per mixture: target, room, target angle, the
    number of directional noises with their file, start and angle, SNR, NDR (with ``diffuse=True``: one white
    noise per angle of the room, drawn on the device from a seed of the mixture's own) and the RMS jitter. ``set_epoch``
    synthesises the epoch in batches and keeps the requested sources in pinned host memory; the same
    ``(seed, epoch)`` gives bitwise the same mixtures.

    The reference's remaining options, all off by default (then the draws and the mixtures are what they were
    without them): ``diffuse_color`` colours the diffuse noises; ``diffuse_ltas_eq`` matches the diffuse sum to
    the speech pool's long-term average spectrum (computed once, at the first synthesis); ``decay`` draws one
    ``(rt60, drr, delay)`` per mixture from the three uniform ranges and adds a decaying noise tail
    (``decay_color``) to the target's and every directional noise's BRIR, each with a tail seed of its own, not
    to the diffuse BRIRs; ``synthetic_noises`` (``'colored_<colour>'``, ``'ssn'``) join the noise files as
    choices for a directional noise. Every device draw comes from a generator seeded per mixture. A coloured
    tail longer than 512 blocks, or an LTAS over a signal shorter than 512 samples, is a ValueError.

    Out of scope: corpus scanning and SOFA / audio file input."""

    def __init__(self, path, sources, size, speech=None, noises=None, brirs=None, seed=0, fs=16000, padding=0.0,
                 noise_count=(0, 3), snr=(-5.0, 10.0), ndr=(0.0, 30.0), diffuse=False, rms_jitter=(0.0, 0.0),
                 batch=64, block=256, device='cuda', diffuse_color='white', diffuse_ltas_eq=False, decay=False,
                 decay_color='white', decay_rt60=(0.1, 5.0), decay_drr=(5.0, 35.0), decay_delay=(0.075, 0.100),
                 synthetic_noises=()):
        if speech is None:
            speech, noises, brirs = self._load(path)
        self.sources, self.size, self.seed, self.fs = list(sources), int(size), int(seed), fs
        for s in self.sources:
            if s not in COMPONENTS:
                raise ValueError(f'unknown source {s!r}; one of {COMPONENTS}')
        self.padding, self.noise_count, self.snr, self.ndr = padding, tuple(noise_count), tuple(snr), tuple(ndr)
        self.diffuse, self.rms_jitter, self.batch, self.block = bool(diffuse), tuple(rms_jitter), int(batch), block
        self.device = device
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)                    # noqa: E731
        self._speech = [f32(x).reshape(-1) for x in speech]
        self._noises = [f32(x).reshape(-1) for x in (noises or [])]
        self._brirs = [[f32(h) for h in room] for room in brirs]
        if not self._speech or not self._brirs or any(not room for room in self._brirs):
            raise ValueError('needs at least one speech signal and one room with one BRIR')
        if any(h.ndim != 2 or h.shape[1] != 2 for room in self._brirs for h in room):
            raise ValueError('a BRIR is (taps, 2)')
        # offsets of every pooled array in the two flat device tensors (uploaded on first use)
        self._sig_off = np.cumsum([0] + [len(x) for x in self._speech + self._noises]).tolist()
        flat = [h for room in self._brirs for h in room]
        off = np.cumsum([0] + [h.size for h in flat]).tolist()
        self._brir_ref, k = [], 0
        for room in self._brirs:
            self._brir_ref.append([(off[k + a], room[a].shape[0]) for a in range(len(room))])
            k += len(room)
        self.diffuse_color, self.diffuse_ltas_eq = diffuse_color, bool(diffuse_ltas_eq)
        self.decay, self.decay_color = bool(decay), decay_color
        self.decay_rt60, self.decay_drr, self.decay_delay = tuple(decay_rt60), tuple(decay_drr), tuple(decay_delay)
        self.synthetic_noises = tuple(synthetic_noises)
        for c in (diffuse_color, decay_color):
            if c not in COLORS:
                raise ValueError(f'color must be either one of {tuple(COLORS)}')
        for t in self.synthetic_noises:
            if t != 'ssn' and not (t.startswith('colored_') and t[8:] in COLORS):
                raise ValueError(f"a synthetic noise is 'ssn' or 'colored_<colour>', got {t!r}")
        self._needs_ltas = (self.diffuse and self.diffuse_ltas_eq) or 'ssn' in self.synthetic_noises
        if self._needs_ltas and min(len(x) for x in self._speech) < N_FFT:
            raise ValueError(f'LTAS framing needs at least {N_FFT} samples per signal: the shortest speech signal '
                             f'has {min(len(x) for x in self._speech)}')
        # numpy's first-maximum rule per ear, the smaller of the two: where BRIRDecay starts counting its delay
        self._brir_onset = [[int(np.argmax(np.abs(h), axis=0).min()) for h in room] for room in self._brirs]
        self._pools, self._ltas = None, None
        self._epoch, self._meta, self._items = 0, self.draw(0), None

    @staticmethod
    def _load(path):
        with np.load(path) as z:
            def numbered(prefix):
                keys = sorted((k for k in z.files if k.startswith(prefix)), key=lambda k: int(k[len(prefix):]))
                return [z[k] for k in keys]
            rooms = {}
            for k in z.files:
                if k.startswith('brir_'):
                    room, angle = (int(v) for v in k[5:].split('_'))
                    rooms.setdefault(room, {})[angle] = z[k]
            brirs = [[rooms[r][a] for a in sorted(rooms[r])] for r in sorted(rooms)]
            return numbered('speech_'), numbered('noise_'), brirs

    # -- the epoch's draws (host only) ------------------------------------------------------------------------
    def draw(self, epoch):
        """The metadata of every mixture of ``epoch``: a list of dicts, a function of ``(seed, epoch)`` only."""
        rng = np.random.default_rng([self.seed, int(epoch)])
        n_pad = round(self.padding*self.fs)
        meta = []
        for _ in range(self.size):
            t = int(rng.integers(len(self._speech)))
            room = int(rng.integers(len(self._brirs)))
            angles = len(self._brirs[room])
            m = dict(target=t, room=room, angle=int(rng.integers(angles)), frames=len(self._speech[t]) + 4*n_pad)
            fits = [i for i, x in enumerate(self._noises) if len(x) >= m['frames']]
            choices = len(fits) + len(self.synthetic_noises)
            count = int(rng.integers(self.noise_count[0], self.noise_count[1] + 1)) if choices else 0
            m['noises'] = []
            for _ in range(count):
                c = int(rng.integers(choices))
                if c >= len(fits):                 # a synthetic noise: a white draw of its own, coloured or matched
                    m['noises'].append(dict(type=self.synthetic_noises[c - len(fits)], seed=int(rng.integers(2**62)),
                                            angle=int(rng.integers(angles))))
                    continue
                f = fits[c]
                m['noises'].append(dict(file=f, i_start=int(rng.integers(len(self._noises[f]) - m['frames'] + 1)),
                                        angle=int(rng.integers(angles))))
            m['diffuse'] = self.diffuse
            # the white noises of a mixture come from a generator of its own: no function of the batch it is in
            m['diffuse_seed'] = int(rng.integers(2**62)) if self.diffuse else None
            m['snr'] = float(rng.uniform(*self.snr)) if (count or self.diffuse) else None
            m['ndr'] = float(rng.uniform(*self.ndr)) if (count and self.diffuse) else None
            m['rms_jitter'] = float(rng.uniform(*self.rms_jitter))
            # the options below draw, and add keys, only when they are on
            if self.diffuse and self.diffuse_color != 'white':
                m['diffuse_color'] = self.diffuse_color
            if self.diffuse and self.diffuse_ltas_eq:
                m['diffuse_ltas_eq'] = True
            if self.decay:                         # one decay per mixture; a tail seed per decayed BRIR
                m['decay'] = dict(rt60=float(rng.uniform(*self.decay_rt60)), drr=float(rng.uniform(*self.decay_drr)),
                                  delay=float(rng.uniform(*self.decay_delay)), color=self.decay_color,
                                  seeds=[int(rng.integers(2**62)) for _ in range(1 + count)])
            if self._needs_ltas and m['frames'] < N_FFT:
                raise ValueError(f'LTAS framing needs at least {N_FFT} samples per signal, a mixture has '
                                 f"{m['frames']}")
            meta.append(m)
        return meta

    @property
    def file_lengths(self):
        return [m['frames'] for m in self._meta]

    # -- synthesis ------------------------------------------------------------------------------------------------
    def _spec(self, m, diffuse_refs, noise_refs, brir_refs):
        """``noise_refs[j]``: where a synthetic noise lies in the pool of generated signals, None for a noise file;
        ``brir_refs``: the (decayed) BRIRs of the target and the directional noises."""
        ns = len(self._speech)
        spec = dict(target=(0, self._sig_off[m['target']], len(self._speech[m['target']])),
                    brir=brir_refs[0], snr=m['snr'], ndr=m['ndr'], rms_jitter=m['rms_jitter'])
        spec['noises'] = [(ref or (0, self._sig_off[ns + n['file']] + n['i_start'], m['frames']), h)
                          for n, ref, h in zip(m['noises'], noise_refs, brir_refs[1:])]
        spec['diffuse'] = list(zip(diffuse_refs, self._brir_ref[m['room']])) if m['diffuse'] else []
        if m.get('diffuse_ltas_eq'):
            spec['diffuse_ltas'] = True
        return spec

    def _upload(self):
        dev = torch.device(self.device)
        if self._pools is None:
            self._pools = (torch.from_numpy(np.concatenate(self._speech + self._noises)).to(dev),
                           torch.from_numpy(np.concatenate([h.reshape(-1) for room in self._brirs for h in room])).to(dev))
        if self._needs_ltas and self._ltas is None:
            signals = self._pools[0]
            files = [signals[self._sig_off[i]:self._sig_off[i + 1]] for i in range(len(self._speech))]
            self._ltas = torch.from_numpy(speech_ltas(files)).to(dev)
        return self._pools

    def synthesize(self, meta):
        """One batch of drawn mixtures on the device (``MixtureBatch`` of ``self.sources``)."""
        signals, brir_pool = self._upload()
        dev = signals.device
        # pool 1: what is generated for this batch -- per mixture its diffuse white noises (one draw from the
        # mixture's generator, as ever), then one white draw per synthetic noise, then one per decay tail
        refs, noise_refs, drawn, total = [], [], [], 0
        color_rows, tail_rows, ssn_rows, decays = [], [], [], []

        def draw(seed, n):
            nonlocal total
            g = torch.Generator(device=dev).manual_seed(seed)
            drawn.append(torch.randn(n, generator=g, device=dev, dtype=torch.float32))
            total += n
            return total - n

        for i, m in enumerate(meta):
            k = len(self._brirs[m['room']]) if m['diffuse'] else 0
            refs.append([(1, total + a*m['frames'], m['frames']) for a in range(k)])
            if k:
                draw(m['diffuse_seed'], k*m['frames'])
                if m.get('diffuse_color'):
                    color_rows += [(off, n, m['diffuse_color']) for _, off, n in refs[-1]]
            noise_refs.append([])
            for n in m['noises']:
                if 'type' not in n:
                    noise_refs[-1].append(None)
                    continue
                off = draw(n['seed'], m['frames'])
                noise_refs[-1].append((1, off, m['frames']))
                if n['type'] == 'ssn':
                    ssn_rows.append((off, m['frames']))
                elif n['type'] != 'colored_white':
                    color_rows.append((off, m['frames'], n['type'][8:]))
            d = m.get('decay')
            if d and d['rt60'] != 0:
                for j, angle in enumerate([m['angle']] + [n['angle'] for n in m['noises']]):
                    boff, taps = self._brir_ref[m['room']][angle]
                    n_out = max(int(round(2*(d['rt60'] + d['delay'])*self.fs)), taps)
                    tail = n_out - int(round(d['delay']*self.fs)) - self._brir_onset[m['room']][angle]
                    if tail < 1:
                        raise ValueError(f'mixture {i}: the decay tail would start behind the BRIR')
                    off = draw(d['seeds'][j], tail)
                    if d['color'] != 'white':
                        tail_rows.append((off, tail, d['color']))
                    decays.append((i, j, (boff, taps, off, tail, d['rt60'], d['drr'], d['delay'], tail)))
        generated = torch.cat(drawn) if drawn else None
        # colouring in place: mixture-length rows and the (longer, rarely repeating) tails in calls of their own
        for rows in (color_rows, tail_rows):
            if rows:
                colorize_rows(generated, rows, self.block, dst=generated, dst_offsets=[r[0] for r in rows])
        if ssn_rows:                               # speech-shaped noise: white, matched to the speech LTAS
            T = max(n for _, n in ssn_rows)
            x = torch.empty(len(ssn_rows), T, dtype=torch.float32, device=dev)
            call('brv_mix_pack_signals', generated, _up([(off, n, 0) for off, n in ssn_rows], np.int64, dev), x,
                 generated.numel(), len(ssn_rows), T, hip.stream())
            y = match_rows(x, [(r, 1, n) for r, (_, n) in enumerate(ssn_rows)], self._ltas)
            back = [(r, 0, n, off, n) for r, (off, n) in enumerate(ssn_rows)]
            fx_call('brv_mixfx_copy_rows', y, _up(back, np.int64, dev), generated, len(back), len(ssn_rows), T,
                    generated.numel(), hip.stream())
        brir_refs = [[self._brir_ref[m['room']][a] for a in [m['angle']] + [n['angle'] for n in m['noises']]]
                     for m in meta]
        decay_status = None
        if decays:                                 # the decayed BRIRs lie behind the pool's own
            pool, where, decay_status = decay_jobs(brir_pool, generated, [job for _, _, job in decays], self.fs)
            for (i, j, _), (off, n) in zip(decays, where):
                brir_refs[i][j] = (brir_pool.numel() + off, n)
            brir_pool = torch.cat([brir_pool, pool])
        pools = [signals] + ([generated] if drawn else [])
        specs = [self._spec(m, r, nr, br) for m, r, nr, br in zip(meta, refs, noise_refs, brir_refs)]
        res = synthesize(pools, brir_pool, specs, components=self.sources, padding=self.padding, fs=self.fs,
                         block=self.block, ltas=self._ltas)
        if decay_status is not None:               # a mixture takes the largest status word of its decay jobs
            owner = torch.tensor([i for i, _, _ in decays], dtype=torch.int64).to(dev, non_blocking=True)
            worst = torch.zeros(len(meta), dtype=torch.int32, device=dev)
            worst.scatter_reduce_(0, owner, decay_status, 'amax')
            res.status = torch.where(worst != 0, worst, res.status)
        return res

    def set_epoch(self, epoch):
        self._epoch, self._meta = int(epoch), self.draw(epoch)
        self._items, queue = [None]*self.size, []

        def finish(res, host, start, status, event):   # wait for ONE batch; only its pinned copies stay alive
            event.synchronize()
            res.raise_for(status.tolist())
            for j, T in enumerate(res.lengths):
                self._items[start + j] = [host[name][j, :T].numpy() for name in self.sources]

        for start in range(0, self.size, self.batch):
            res = self.synthesize(self._meta[start:start + self.batch])
            host = {}
            for name in self.sources:
                dev = res.components[name]
                host[name] = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
                host[name].copy_(dev, non_blocking=True)
            status = torch.empty(res.status.shape, dtype=res.status.dtype, pin_memory=True)
            status.copy_(res.status, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            queue.append((res, host, start, status, event))
            if len(queue) > 2:                 # two batches stay queued behind the one being waited for
                finish(*queue.pop(0))
        while queue:
            finish(*queue.pop(0))

    def __getitem__(self, i):
        if self._items is None:
            self.set_epoch(self._epoch)
        return self._items[i]

    # -- a fixed dataset on disk ------------------------------------------------------------------------------
    def write_dataset(self, path, epoch=0, bits_per_sample=16, tar=True, block_size=4096, lpc_order=8):
        """Freeze ``epoch`` as a dataset ``BreverDataset(path)`` reads: ``path/audio.tar`` with members
        ``audio/NNNNN_<source>.flac`` (``tar=False``: the directory ``path/audio/``) and ``path/mixture_info.json``,
        the list ``draw(epoch)`` returns. The epoch is synthesised batch by batch and every source is encoded on
        the device (``flac_enc.FlacBatchEncoder``): the float32 components never go to the host. Two batches
        stay queued behind the one whose bytes are being downloaded and written, as in ``set_epoch``. Member names,
        order, mode, owner and mtime (0) are fixed, so ``(seed, epoch)`` gives byte-identical archives. The maker's
        own epoch is left as it is. Returns the seconds spent per stage (``synthesis`` and ``encode`` are the
        host's time to queue them; the device's time shows up in ``wait``)."""
        import io
        import json
        import tarfile
        from .flac_enc import FlacBatchEncoder, status_message
        meta = self.draw(epoch)
        encoder = FlacBatchEncoder(self.device)
        os.makedirs(path, exist_ok=True)
        seconds = dict(synthesis=0.0, encode=0.0, wait=0.0, copy=0.0, write=0.0)
        if tar:
            archive = tarfile.open(os.path.join(path, 'audio.tar'), 'w', format=tarfile.GNU_FORMAT)
        else:
            archive = None
            os.makedirs(os.path.join(path, 'audio'), exist_ok=True)

        def finish(res, pending, start):
            t0 = time.perf_counter()
            res.check()                            # waits for the batch's synthesis
            seconds['wait'] += time.perf_counter() - t0
            for name, p in zip(self.sources, pending):
                streams = p.result(check=False)
                seconds['wait'] += p.seconds['wait']
                seconds['copy'] += p.seconds['copy']
                for j, st in enumerate(p.status):
                    if st:
                        raise ValueError(f'mixture {start + j}, source {name}: {status_message(st)}')
                t0 = time.perf_counter()
                for j, blob in enumerate(streams):
                    member = f'audio/{start + j:05d}_{name}.flac'
                    if archive is None:
                        with open(os.path.join(path, member), 'wb') as f:
                            f.write(blob)
                    else:
                        info = tarfile.TarInfo(member)
                        info.size, info.mtime, info.mode = len(blob), 0, 0o644
                        info.uid = info.gid = 0
                        info.uname = info.gname = ''
                        archive.addfile(info, io.BytesIO(blob))
                seconds['write'] += time.perf_counter() - t0

        try:
            queue = []
            for start in range(0, self.size, self.batch):
                t0 = time.perf_counter()
                res = self.synthesize(meta[start:start + self.batch])
                t1 = time.perf_counter()
                # components are (mixtures, frames, 2): the encoder takes (rows, channels, frames)
                pending = [encoder.submit(res.components[name].transpose(1, 2), res.lengths, fs=self.fs,
                                          bits_per_sample=bits_per_sample, block_size=block_size,
                                          lpc_order=lpc_order) for name in self.sources]
                seconds['synthesis'] += t1 - t0
                seconds['encode'] += time.perf_counter() - t1
                queue.append((res, pending, start))
                if len(queue) > 2:
                    finish(*queue.pop(0))
            while queue:
                finish(*queue.pop(0))
        finally:
            if archive is not None:
                archive.close()

        def clean(v):                              # numpy scalars and tuples out, NaN never occurs in a draw
            if isinstance(v, dict):
                return {str(k): clean(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return [clean(x) for x in v]
            if isinstance(v, (np.integer, np.bool_)):
                return int(v)
            if isinstance(v, np.floating):
                return float(v)
            return v
        with open(os.path.join(path, 'mixture_info.json'), 'w') as f:
            json.dump(clean(meta), f, indent=1, sort_keys=True)
            f.write('\n')
        return seconds
