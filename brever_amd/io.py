"""``brever.io.resample`` on the GPU: exact Fourier resampling of whole signals, in fp64.

The reference resamples every file that is not at the working rate with ``scipy.signal.resample`` over the whole
signal: a real DFT of all ``N`` samples, the lowest ``min(N, M)//2 + 1`` bins kept, an inverse of ``M = ceil(N
new_fs/old_fs)`` points. ``N`` is whatever the file holds. Here a ragged batch of signals goes through
``libbrever_resample.so`` (include/brever_resample.h; csrc/resample/resample.hip): two Bluestein chirp transforms
per signal on a power-of-two length ``L``, all signals of one ``L`` in the same launches:

    chirp spectra of the (N, L) and (M, L) the cache misses      brv_rs_chirp_spectra
    N-point analysis, the kept bins weighted for the inverse     brv_rs_analysis
    M-point synthesis, the real part, float64 or float32 out     brv_rs_synthesis

The result of a signal is bitwise the same alone or in any batch, with a cold or a warm cache. There is no CPU
fallback: without the library or a ROCm device the calls raise. A signal longer than ``max_length()`` samples (in
or out) is refused, never truncated.
"""
import collections

import numpy as np
import torch

from . import hip

WORK_BYTES = 2 << 30                   # scratch per launch group: columns of one L are chunked to fit

# the brv_rs_* entry points of include/brever_resample.h
_LIB = hip.Library('brever_resample.h', 'libbrever_resample.so', 'BRV_RESAMPLE_LIB_PATH',
                   'The resampler has no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, last_error = _LIB.lib, _LIB.call, _LIB.last_error
MAX_COLUMNS = _LIB.constants['BRV_RS_MAX_COLUMNS']      # columns per launch


def max_length():
    """The longest signal, in samples in and out, the library takes."""
    return int(lib().brv_rs_max_length())


def out_length(n, old_fs, new_fs):
    """Samples ``n`` samples at ``old_fs`` become at ``new_fs``: the reference's rule, in doubles as it writes it."""
    ratio = new_fs/old_fs
    m = np.ceil(n*ratio)                       # (an array of lengths gives an array)
    return int(m) if np.ndim(m) == 0 else m.astype(np.int64)


def fft_length(n, m):
    """The convolution length ``L`` of a signal of ``n`` samples in and ``m`` out; ``ValueError`` with the limit's
    name when the library does not take the signal."""
    L = int(lib().brv_rs_fft_length(int(n), int(m)))
    if L < 0:
        raise ValueError(f'cannot resample: {last_error()} (brv_rs_max_length() = {max_length()})')
    return L


def plan(n, old_fs, new_fs):
    """``(M, L)`` of a signal of ``n`` samples: host arithmetic only, nothing is allocated."""
    if n < 1:
        raise ValueError('cannot resample an empty signal')
    m = out_length(n, old_fs, new_fs)
    return m, fft_length(n, m)


class ChirpCache:
    """Device-resident chirp spectra per ``(kind, n, L)``: one slab of ``slots`` rows of ``L`` complex128 per
    ``(device, L)``, the least recently used slot of a slab reused first, the least recently used slab dropped once
    ``max_bytes`` are held. A slab takes at most a quarter of ``max_bytes`` and always has at least one slot; a batch
    is served in chunks of at most ``slots`` columns. A miss costs one fill and one transform on the device (``brv_rs_chirp_spectra``); nothing waits, so the
    calls that share a cache must be made on one stream: a slot is refilled in stream order behind its last reader."""

    MAX_SLOTS = 256

    def __init__(self, max_bytes=4 << 30):
        self.max_bytes, self.hits, self.misses, self.evictions = int(max_bytes), 0, 0, 0
        self._slabs = collections.OrderedDict()            # (device, L) -> [tensor, OrderedDict key -> slot, free]

    @property
    def bytes(self):
        return sum(s[0].numel()*8 for s in self._slabs.values())

    def slots(self, L):
        return int(max(1, min(self.MAX_SLOTS, self.max_bytes//4//(16*L))))

    def slab(self, L, device):
        key = (str(device), int(L))
        if key not in self._slabs:
            n = self.slots(L)
            self._slabs[key] = [torch.empty((n, L, 2), dtype=torch.float64, device=device),
                                collections.OrderedDict(), list(range(n - 1, -1, -1))]
        self._slabs.move_to_end(key)
        while self.bytes > self.max_bytes and len(self._slabs) > 1:
            _, old = self._slabs.popitem(last=False)
            self.evictions += len(old[1])
        return self._slabs[key]

    def acquire(self, keys, L, device):
        """Slots of the ``(kind, n)`` in ``keys`` (at most ``slots(L)`` distinct ones) in the slab of ``L``:
        ``(slab, {key: slot}, [(slot, n, kind) to fill])``."""
        slab, held, free = self.slab(L, device)
        wanted = list(dict.fromkeys(keys))
        if len(wanted) > slab.shape[0]:
            raise ValueError(f'{len(wanted)} chirp spectra wanted at once, the slab holds {slab.shape[0]}')
        for key in wanted:
            if key in held:
                held.move_to_end(key)
        fill = []
        for key in wanted:
            if key in held:
                self.hits += 1
                continue
            self.misses += 1
            if not free:
                _, slot = held.popitem(last=False)          # never one of `wanted`: those sit at the end
                self.evictions += 1
                free.append(slot)
            held[key] = free.pop()
            fill.append((held[key], key[1], key[0]))
        return slab, {key: held[key] for key in wanted}, fill

    def clear(self):
        self._slabs.clear()


chirps = ChirpCache()
_tw = {}


def _factors(device):
    """exp(-2 pi i j/4096), j < 2048, float64 (2048, 2): the butterfly factors of the LDS transforms."""
    key = str(device)
    if key not in _tw:
        ang = 2*np.pi*np.arange(2048)/4096
        _tw[key] = torch.from_numpy(np.stack([np.cos(ang), -np.sin(ang)], axis=1)).to(device)
    return _tw[key]


def _as_tensor(x):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if t.dim() not in (1, 2):
        raise ValueError(f'a signal is 1-D or (samples, channels), got shape {tuple(t.shape)}')
    return t


def resample_batch(xs, old_fs, new_fs, dtype=torch.float64, cache=None, device=None):
    """``resample`` of every signal of ``xs`` (1-D or ``(samples, channels)``; NumPy or torch, host or device) from
    ``old_fs`` (a scalar or one value per signal) to ``new_fs``: a list of device tensors of ``dtype`` (float64 or
    float32, rounded once from the fp64 result), each of the shape of its input with ``M`` samples. Launches only:
    the call does not wait for the device."""
    if dtype not in (torch.float64, torch.float32):
        raise ValueError('dtype is torch.float64 or torch.float32')
    cache = chirps if cache is None else cache
    xs = [_as_tensor(x) for x in xs]
    rates = list(old_fs) if np.ndim(old_fs) else [old_fs]*len(xs)
    if len(rates) != len(xs):
        raise ValueError('old_fs is a scalar or one value per signal')
    if device is None:
        device = next((x.device for x in xs if x.is_cuda), None) or torch.device('cuda', torch.cuda.current_device())
    plans = [plan(x.shape[0], fs, new_fs) for x, fs in zip(xs, rates)]          # refusals first: nothing allocated yet
    if not xs:
        return []
    in_dtype = torch.float32 if all(x.dtype == torch.float32 for x in xs) else torch.float64
    if all(not x.is_cuda for x in xs):
        pool = torch.cat([x.to(in_dtype).reshape(-1) for x in xs]).to(device)
    else:
        pool = torch.cat([x.to(device=device, dtype=in_dtype).reshape(-1) for x in xs])
    hip.require_device(pool)
    out_sizes = [m*(x.shape[1] if x.dim() == 2 else 1) for x, (m, _) in zip(xs, plans)]
    out = torch.empty(max(1, sum(out_sizes)), dtype=dtype, device=device)
    classes, outs, x_at, out_at = {}, [], 0, 0
    for x, (m, L), size in zip(xs, plans, out_sizes):
        n, ch = x.shape[0], (x.shape[1] if x.dim() == 2 else 1)
        view = out[out_at:out_at + size].view(m, ch) if x.dim() == 2 else out[out_at:out_at + size]
        if m == n:                                                                # the reference returns x itself
            view.copy_(pool[x_at:x_at + n*ch].view_as(view))
        else:
            classes.setdefault(L, []).extend((x_at + c, ch, n, m, out_at + c, ch) for c in range(ch))
        outs.append(view)
        x_at, out_at = x_at + n*ch, out_at + size
    tw = _factors(device)
    with torch.cuda.device(device):
        stream = hip.stream()
        for L in sorted(classes):
            cols = classes[L]
            step = int(max(1, min(cache.slots(L), WORK_BYTES//(16*L), MAX_COLUMNS)))
            for at in range(0, len(cols), step):
                _run(cols[at:at + step], L, pool, out, tw, cache, device, stream)
    return outs


def _run(cols, L, pool, out, tw, cache, device, stream):
    """One chunk of columns of one ``L``: the two halves, each after the chirp spectra it needs."""
    work = torch.empty((len(cols), L, 2), dtype=torch.float64, device=device)
    for kind in (0, 1):
        keys = [(kind, c[2 + kind]) for c in cols]
        slab, slots, fill = cache.acquire(keys, L, device)
        desc = np.array([c + (slots[k], L) for c, k in zip(cols, keys)], dtype=np.int64)
        desc = torch.from_numpy(desc).to(device)
        if fill:
            fdesc = torch.from_numpy(np.array(fill, dtype=np.int64)).to(device)
            call('brv_rs_chirp_spectra', slab, fdesc, tw, slab.shape[0], L, len(fill), stream)
        if kind == 0:
            call('brv_rs_analysis', pool, desc, slab, tw, work, pool.numel(), int(pool.dtype == torch.float32),
                 slab.shape[0], L, len(cols), stream)
        else:
            call('brv_rs_synthesis', work, desc, slab, tw, out, out.numel(), int(out.dtype == torch.float32),
                 slab.shape[0], L, len(cols), stream)


def resample(x, old_fs, new_fs, axis=0, cache=None):
    """Resample ``x`` along ``axis`` from ``old_fs`` to ``new_fs`` (``brever.io.resample``). A NumPy array gives a
    float64 NumPy array, a host tensor a float64 host tensor, a device tensor a device tensor: float32 for a float32
    one, else float64."""
    is_numpy = not isinstance(x, torch.Tensor)
    t = torch.from_numpy(np.asarray(x)) if is_numpy else x
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    dtype = torch.float32 if (t.is_cuda and t.dtype == torch.float32) else torch.float64
    moved = t.movedim(axis, 0)
    flat = moved.reshape(moved.shape[0], -1)
    y = resample_batch([flat], old_fs, new_fs, dtype=dtype, cache=cache)[0]
    y = y.reshape((y.shape[0],) + tuple(moved.shape[1:])).movedim(0, axis)
    if t.is_cuda:
        return y
    y = y.cpu()
    return y.numpy() if is_numpy else y
