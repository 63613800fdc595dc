"""Test-side references of the Fourier resampler (brever_amd/io.py, csrc/resample/resample.hip). NumPy only.

``resample``: the fp64 restatement of the reference's ``brever.io.resample`` (``scipy.signal.resample`` over the
whole signal), the yardstick of every value test.

``bluestein``: the algorithm of the kernels in NumPy complex128 -- the same convolution length L, the same
four-step decomposition (column transforms of at most 256, factors, row transforms of at most 4096), the same
radix-2 decimation-in-frequency short transforms with a factor table, the same integer reduction of the chirp
phases. Its error against ``resample`` is what the device's precision leaves of this algorithm; the GPU test bounds
the kernels' error by 8 times it.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resample.npz')

# (N, old_fs, new_fs, channels) of the fixture: the small cases
GOLDEN_CASES = [(1, 48000, 16000, 1), (2, 48000, 16000, 1), (3, 48000, 16000, 1), (7, 16000, 48000, 1),
                (8, 16000, 48000, 1), (16, 48000, 16000, 1), (2, 8000, 16000, 1), (3, 16000, 48000, 1),
                (7, 48000, 16000, 1), (8, 48000, 16000, 1), (16, 8000, 16000, 1), (16, 44100, 16000, 1),
                (441, 44100, 16000, 1), (442, 44100, 16000, 1), (4800, 48000, 16000, 1), (4801, 48000, 16000, 1),
                (4802, 48000, 16000, 1), (4801, 48000, 16000, 2), (441, 8000, 16000, 1), (442, 16000, 48000, 1)]
# the cases of the GPU tests beyond the fixture; their reference is ``resample`` below
LARGE_CASES = [(9973, 8000, 16000, 1), (30000, 16000, 48000, 1), (65537, 48000, 16000, 1),
               (70001, 48000, 16000, 1), (70001, 44100, 16000, 1), (131101, 48000, 16000, 1),
               ((1 << 20) + 3, 48000, 16000, 1)]
CASES = GOLDEN_CASES + LARGE_CASES
PCM_CASES = [c for c in CASES if c[0] >= 441]
SEED = 2          # seed 0 leaves a sample of the largest case 3.1e-8 from a rounding tie; with 2 the closest is 1.4e-6


def case_key(case):
    return '{}_{}_{}_{}'.format(*case)


def case_input(case):
    """The input of a case on the int16 grid, as a decoded 16-bit WAV is. Each case has its own stream."""
    n, old_fs, new_fs, ch = case
    rng = np.random.default_rng([SEED, n, old_fs, new_fs, ch])
    x = np.round(0.3*rng.standard_normal((n, ch) if ch > 1 else n)*32768)/32768
    return x


def out_length(n, old_fs, new_fs):
    """The reference's rule, in doubles exactly as it writes it."""
    ratio = new_fs/old_fs
    return int(np.ceil(n*ratio))


def resample(x, old_fs, new_fs, axis=0):
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    n = x.shape[0]
    m = out_length(n, old_fs, new_fs)
    if m == n:
        return np.moveaxis(x, 0, axis)
    X = np.fft.rfft(x, axis=0)
    k = min(n, m)
    Y = np.zeros((m//2 + 1,) + x.shape[1:], dtype=np.complex128)
    Y[:k//2 + 1] = X[:k//2 + 1]
    if k % 2 == 0:
        if m < n:
            Y[k//2] *= 2
        elif n < m:
            Y[k//2] *= 0.5
    y = np.fft.irfft(Y, m, axis=0)*(m/n)
    return np.moveaxis(y, 0, axis)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def reference(case):
    """The expected output of a case: the reference's own where the fixture holds it, else the restatement."""
    z = golden()
    key = 'y_' + case_key(case)
    if key in z:
        return z[key]
    return resample(case_input(case), case[1], case[2])


# ---- the kernels' algorithm ------------------------------------------------------------------------------------------
def fft_length(n, m):
    need = max(n, m) + min(n, m)//2
    L = 16
    while L < need:
        L *= 2
    return L


def _table():
    j = np.arange(2048)
    return np.cos(2*np.pi*j/4096) - 1j*np.sin(2*np.pi*j/4096)


TW = _table()


@functools.lru_cache(maxsize=None)
def _bitrev(logt):
    k, rev = np.arange(1 << logt), np.zeros(1 << logt, dtype=np.int64)
    for b in range(logt):
        rev |= ((k >> b) & 1) << (logt - 1 - b)
    return rev


def _short(a, inv):
    """Radix-2 decimation in frequency over the middle axis of ``a`` (pre, T, post), natural order in and out."""
    pre, T, post = a.shape
    a = a.copy()
    half = T//2
    while half >= 1:
        w = TW[np.arange(half)*(2048//half)]
        if inv:
            w = w.conj()
        v = a.reshape(pre, T//(2*half), 2, half, post)
        u, d = v[:, :, 0] + v[:, :, 1], v[:, :, 0] - v[:, :, 1]
        v[:, :, 0] = u
        v[:, :, 1] = d*w[:, None]
        half //= 2
    return a[:, _bitrev(T.bit_length() - 1)]


def _plan(L):
    logl = L.bit_length() - 1
    logs = min(logl, 12)
    rem = logl - logs
    return ([rem - 8, 8] if rem > 8 else [rem] if rem else []), logs


def _factor(R, Sp, inv):
    p = (np.arange(R)[:, None]*np.arange(Sp)[None, :]).astype(np.float64)
    ang = 2*p/(R*Sp)                          # exact; sincospi of it
    return np.cos(np.pi*ang) + (1j if inv else -1j)*np.sin(np.pi*ang)


def transform(a, inv):
    """The length-L transform of the kernels, bins left in the decomposition's order (forward), or its inverse
    from that order (unscaled)."""
    L = len(a)
    levels, logs = _plan(L)
    shapes, rest = [], L
    for logr in levels:
        shapes.append((L//rest, 1 << logr, rest >> logr))
        rest >>= logr
    if not inv:
        for outer, R, Sp in shapes:
            a = _short(a.reshape(outer, R, Sp), False)*_factor(R, Sp, False)
        return _short(a.reshape(-1, 1 << logs, 1), False).reshape(-1)
    a = _short(a.reshape(-1, 1 << logs, 1), True)
    for outer, R, Sp in reversed(shapes):
        a = _short(a.reshape(outer, R, Sp)*_factor(R, Sp, True), True)
    return a.reshape(-1)


def chirp(j, n, sign):
    j = np.asarray(j, dtype=np.uint64)
    r = (j*j) % np.uint64(2*n)
    ang = r.astype(np.float64)/float(n)
    return np.cos(np.pi*ang) + sign*1j*np.sin(np.pi*ang)


def chirp_spectrum(n, L, kind):
    j = np.arange(L)
    split = n if kind else L - n + 1
    return transform(chirp(np.where(j < split, j, L - j), n, -1.0 if kind else 1.0), False)


def bluestein(x, old_fs, new_fs):
    """``resample`` of a 1-D or (samples, channels) signal by the kernels' algorithm."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        return np.stack([bluestein(x[:, c], old_fs, new_fs) for c in range(x.shape[1])], axis=1)
    n = len(x)
    m = out_length(n, old_fs, new_fs)
    if m == n:
        return x
    L = fft_length(n, m)
    K = min(n, m)
    kb = K//2 + 1
    a = np.zeros(L, dtype=np.complex128)
    a[:n] = x*chirp(np.arange(n), n, -1.0)
    a = transform(transform(a, False)*chirp_spectrum(n, L, 0), True)
    k = np.arange(kb)
    g = np.where((k == 0) | (2*k == m), 1.0, 2.0)
    if K % 2 == 0:
        g[K//2] *= 2.0 if m < n else 0.5 if n < m else 1.0
    g = g*(1.0/L)/n
    c = np.zeros(L, dtype=np.complex128)
    c[:kb] = chirp(k, n, -1.0)*chirp(k, m, 1.0)*a[:kb]*g
    c = transform(transform(c, False)*chirp_spectrum(m, L, 1), True)
    return (chirp(np.arange(m), m, 1.0)*c[:m]).real*(1.0/L)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b)/nb) if nb else float(np.linalg.norm(a - b))


@functools.lru_cache(maxsize=None)
def yardstick(case):
    """rel-L2 error of ``bluestein`` against the case's reference: the yardstick of the GPU value test."""
    return rel(bluestein(case_input(case), case[1], case[2]), reference(case))


def pcm16(y):
    """What the files hold: clip to [-1, 1), times 2^15, round to nearest."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64)*32768.0), -32768, 32767).astype(np.int16)
