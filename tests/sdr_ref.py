"""fp64 restatements of the BSS-eval signal-to-distortion ratio for the tests of the ``sdr`` metric
and criterion. Two independent formulations of the same definition:

(a) ``sdr_lstsq``: the explicit ``(T + L - 1) x L`` shift matrix of the reference, ``numpy.linalg.lstsq`` for the
    allowed distortion filter, SDR from ``|s_target|^2 / |x_pad - s_target|^2``;
(b) ``sdr_toeplitz``: the ``L`` correlation lags, ``scipy.linalg.toeplitz`` and ``scipy.linalg.solve``, SDR from
    ``q = b^T h`` and ``E``.

Both apply the floors of the definition (``eps = 2^-52`` of ``E``) and give NaN for a degenerate row. ``grad_closed``
is the closed-form gradient of ``-SDR`` with respect to the estimate, ``grad_autograd`` the torch-fp64 autograd
gradient through (a). ``signals`` is the recipe of the GPU tests. NumPy / SciPy / torch on the CPU only.
"""
import numpy as np
import scipy.linalg
import scipy.signal
import torch

EPS = 2.0**-52
K10 = 10.0/np.log(10.0)
KINDS = ('white', 'ar2', 'lowpass')
NOISE_DB = (0.0, 40.0)
# the 4-tap filtering of the reference that every estimate carries
TAPS = np.array([0.9, 0.35, -0.2, 0.1])


def signals(kind, T, noise_db, seed=0):
    """``(reference, estimate)`` of ``T`` samples, float64 holding fp32-representable values: the reference is
    white, AR(2) ``1/(1 - 1.8 z^-1 + 0.9 z^-2)`` or 6th-order Butterworth low-pass at 0.25 noise, the estimate its
    4-tap filtering plus white noise ``noise_db`` below it."""
    rng = np.random.default_rng([seed, KINDS.index(kind), T, int(noise_db)])
    w = rng.standard_normal(T + 200)
    if kind == 'ar2':
        w = scipy.signal.lfilter([1.0], [1.0, -1.8, 0.9], w)
    elif kind == 'lowpass':
        w = scipy.signal.lfilter(*scipy.signal.butter(6, 0.25), w)
    s = w[200:]/max(np.sqrt(np.mean(w[200:]**2)), 1e-30)*0.1
    f = np.convolve(s, TAPS)[:T]
    n = rng.standard_normal(T)
    n *= np.linalg.norm(f)/max(np.linalg.norm(n), 1e-30)*10.0**(-noise_db/20.0)
    return s.astype(np.float32).astype(np.float64), (f + n).astype(np.float32).astype(np.float64)


def lags(s, x, L):
    """``r[k] = sum_t s[t] s[t + k]``, ``b[k] = sum_t s[t] x[t + k]`` for ``k < L``; exactly 0 from ``k = T`` on."""
    T = len(s)
    r, b = np.zeros(L), np.zeros(L)
    for k in range(min(L, T)):
        r[k] = np.dot(s[:T - k], s[k:])
        b[k] = np.dot(s[:T - k], x[k:])
    return r, b


def shift_matrix(s, L):
    """``S[t, k] = s[t - k]`` (0 outside the signal), ``(T + L - 1, L)``: ``S h`` is the full convolution."""
    T = len(s)
    S = np.zeros((T + L - 1, L))
    for k in range(L):
        S[k:k + T, k] = s
    return S


def _ratio(q, E):
    return 10.0*np.log10(max(q, EPS*E)/max(E - q, EPS*E))


def sdr_lstsq(s, x, L=512, load_diag=0.0):
    """Formulation (a). Returns ``(sdr, h)``. With ``load_diag`` the least-squares problem carries the rows
    ``sqrt(load_diag r[0]) I`` (the same normal equations as (b)) and ``q = x_pad^T S h``."""
    s, x = np.asarray(s, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T = len(s)
    E = float(np.dot(x, x))
    if not np.dot(s, s) > 0 or not E > 0:
        return float('nan'), np.zeros(L)
    S = shift_matrix(s, L)
    x_pad = np.concatenate([x, np.zeros(L - 1)])
    if load_diag:
        A = np.concatenate([S, np.sqrt(load_diag*np.dot(s, s))*np.eye(L)])
        h = np.linalg.lstsq(A, np.concatenate([x_pad, np.zeros(L)]), rcond=None)[0]
        return _ratio(float(np.dot(x_pad, S @ h)), E), h
    h = np.linalg.lstsq(S, x_pad, rcond=None)[0]
    target = S @ h
    num, den = float(np.dot(target, target)), float(np.dot(x_pad - target, x_pad - target))
    return 10.0*np.log10(max(num, EPS*E)/max(den, EPS*E)), h


def sdr_toeplitz(s, x, L=512, load_diag=0.0):
    """Formulation (b). Returns ``(sdr, h, q, E, cond(R))``."""
    s, x = np.asarray(s, dtype=np.float64), np.asarray(x, dtype=np.float64)
    r, b = lags(s, x, L)
    E = float(np.dot(x, x))
    if not r[0] > 0 or not E > 0:
        return float('nan'), np.zeros(L), 0.0, E, float('nan')
    R = scipy.linalg.toeplitz(r) + load_diag*r[0]*np.eye(L)
    h = scipy.linalg.solve(R, b, assume_a='pos')
    q = float(np.dot(b, h))
    return _ratio(q, E), h, q, E, float(np.linalg.cond(R))


def grad_closed(s, x, L=512, load_diag=0.0, h=None):
    """Closed-form gradient of ``-SDR`` with respect to ``x`` (length ``T``) from formulation (b): one FIR pass of
    ``s`` through ``h`` plus elementwise work. A term whose floor is active contributes 0; a degenerate row gives
    zeros. ``h`` overrides the filter (the misalignment measurement of the host test)."""
    s, x = np.asarray(s, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T = len(s)
    value, h_ref, q, E, _ = sdr_toeplitz(s, x, L, load_diag)
    if np.isnan(value):
        return np.zeros(T)
    if h is None:
        h = h_ref
    target = np.convolve(s, h)[:T]
    g = np.zeros(T)
    if q > EPS*E:
        g += 2.0*target/q
    if E - q > EPS*E:
        g -= 2.0*(x - target)/(E - q)
    return -K10*g


def grad_autograd(s, x, L=512):
    """Gradient of ``-SDR`` with respect to ``x`` by torch-fp64 autograd through formulation (a) (no floors: for
    rows on which neither is active)."""
    S = torch.from_numpy(shift_matrix(np.asarray(s, dtype=np.float64), L))
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    x_pad = torch.cat([xt, torch.zeros(L - 1, dtype=torch.float64)])
    h = torch.linalg.lstsq(S, x_pad[:, None]).solution[:, 0]
    target = S @ h
    loss = -10.0*torch.log10(target.dot(target)/(x_pad - target).dot(x_pad - target))
    grad, = torch.autograd.grad(loss, xt)
    return grad.numpy()


# the (T, L) cases of tests/test_gpu_sdr.py; CHUNK is the chunk length of the correlation kernel (csrc/sdr/sdr.hip,
# brv_sdr_chunk()): 3000 and 16000 are no multiples of it, 2047 / 2048 / 2049 sit at it and beside it
CHUNK = 2048
CASES = ((3000, 32), (3000, 512), (700, 512), (300, 512), (3000, 1), (3000, 33), (CHUNK - 1, 512), (CHUNK, 512),
         (CHUNK + 1, 512), (16000, 512))

# The reference spread: the largest |(a) - (b)| in dB over CASES x KINDS x NOISE_DB (tests/test_sdr_host.py prints
# every one; 7.43e-11 dB at T 3000, L 512, AR(2), 40 dB). The GPU's forward is held to 8 times it against (a).
REF_SPREAD = 7.5e-11
FORWARD_BOUND = 8*REF_SPREAD
# The gradient leaves the GPU in fp32. Rounding a vector to fp32 moves it by at most 2^-24 in rel-L2 (measured on
# the closed form: 2.6e-8 to 2.9e-8); the cap is 16 floors, and the host test checks that it lies at least two
# orders of magnitude below what a one-tap misalignment of h does to the gradient.
GRAD_FLOOR = 2.0**-24
GRAD_CAP = 1e-6
