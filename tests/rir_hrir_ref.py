"""The measured-ear model of DESIGN.md 5o restated in fp64 NumPy: the plain loop over the lattice vector ``n`` and
the parity vector ``p``, one image at a time, no tables, no tiles and no sorting; no code of ``brever_amd``. The GPU
tests compare ``brever_amd.rir`` with it; tests/test_rir_hrir_host.py holds it against tests/rir_bands_ref.py.

    x = (1 - 2p) s + 2 n L        e0 = |n - p|, e1 = |n|        A_k = prod b_k0^e0 b_k1^e1   (0^0 = 1), beta (K, 6)
    v = x - r, d = |v|, q = (v . f, v . l, v . u) with f = (cos yaw, sin yaw, 0), l = (-sin yaw, cos yaw, 0), u = z
    j* = argmax_j q . p_j (the first of equals), tau = d fs / c
    x_{k,j*}[t] += A_k / (4 pi d) sinc(t - tau) (1 + cos(2 pi (t - tau) / W)) / 2   for |t - tau| < W/2, 0 <= t < T
    y_{k,e}[t] = sum_j sum_m H[j, e, m] x_{k,j}[t - m],  0 <= t < T = taps + N/2
    h_e[t] = sum_k sum_m g_k[m] y_{k,e}[t + N/2 - m],  0 <= t < taps
"""
import itertools
import math

import numpy as np

import rir_bands_ref as B


def unit(azimuth_deg, elevation_deg):
    """``(D, 3)``: x front, y left, z up; azimuth counter-clockwise seen from above."""
    az = np.radians(np.asarray(azimuth_deg, dtype=np.float64))
    el = np.radians(np.asarray(elevation_deg, dtype=np.float64))
    return np.stack([np.cos(el)*np.cos(az), np.cos(el)*np.sin(az), np.sin(el)], axis=1)


def fixture_grid():
    """``(azimuth, elevation)`` in degrees of the tests' 38 directions: rings at elevation -45, 0 and 45 every 30
    degrees, then the two poles. The ring at 0 is needed: the source is at the ears' height, so every image reflected
    in x and y only arrives at elevation 0 exactly and would tie between two symmetric rings."""
    az = [float(a) for _ in (-45, 0, 45) for a in range(0, 360, 30)] + [0.0, 0.0]
    el = [float(e) for e in (-45, 0, 45) for _ in range(0, 360, 30)] + [-90.0, 90.0]
    return np.array(az), np.array(el)


def fixture_hrirs(D, taps, seed):
    """``(D, 2, taps)``: seeded normal values under an envelope that decays by e every ``taps / 4`` samples."""
    rng = np.random.default_rng([int(seed), int(D), int(taps)])
    return rng.standard_normal((D, 2, taps))*np.exp(-np.arange(taps)/(taps/4.0))


def fibonacci_sphere(D, seed):
    """``(D, 3)`` unit vectors: the Fibonacci lattice turned by a seeded angle about z, so that no point is a pole or
    on the horizontal plane by construction."""
    i = np.arange(D) + 0.5
    z = 1.0 - 2.0*i/D
    phi = i*math.pi*(3.0 - math.sqrt(5.0)) + np.random.default_rng([int(seed), int(D)]).uniform(0.0, 2.0*math.pi)
    rho = np.sqrt(1.0 - z*z)
    return np.stack([rho*np.cos(phi), rho*np.sin(phi), z], axis=1)


def direction_rows(dims, beta, source, head, yaw, taps, fs, directions, window=None, max_order=-1, c=343.0, N=None,
                   margins=None, used=None):
    """``(K, D, taps + N/2)`` float64: the direction rows ``x_{k,j}``. ``margins``: an optional list that receives,
    per image that touches a tap, the least of ``(q . p_j* - q . p_j) / d`` over the directions ``p_j`` that differ
    from ``p_j*`` (infinite if there is none); ``used``: an optional set that receives every ``j*``."""
    L = np.asarray(dims, dtype=np.float64)
    b = np.asarray(beta, dtype=np.float64).reshape(-1, 3, 2)
    K = len(b)
    s, r = np.asarray(source, dtype=np.float64), np.asarray(head, dtype=np.float64)
    P = np.asarray(directions, dtype=np.float64)
    front = np.array([math.cos(yaw), math.sin(yaw), 0.0])
    left = np.array([-math.sin(yaw), math.cos(yaw), 0.0])
    W = B.default_window(fs) if window is None else float(window)
    N = B.default_n(fs) if N is None else N
    T = taps + N//2
    x = np.zeros((K, len(P), T))
    reach = (T - 1 + W/2)*c/fs
    M = [int(math.ceil(reach/(2*L[k]))) + 1 for k in range(3)]
    for n in itertools.product(*(range(-M[k], M[k] + 1) for k in range(3))):
        n = np.array(n)
        for p in itertools.product((0, 1), repeat=3):
            p = np.array(p)
            e0, e1 = np.abs(n - p), np.abs(n)
            if max_order >= 0 and int(e0.sum() + e1.sum()) > max_order:
                continue
            A = np.prod(b[:, :, 0]**e0, axis=1)*np.prod(b[:, :, 1]**e1, axis=1)         # numpy: 0.0**0 = 1.0
            if not A.any():
                continue
            v = (1 - 2*p)*s + 2*n*L - r
            d = math.sqrt(float(v[0]*v[0] + v[1]*v[1] + v[2]*v[2]))
            tau = d*fs/c
            first, last = max(int(math.floor(tau - W/2)), 0), min(int(math.ceil(tau + W/2)), T - 1)
            if first > last:
                continue
            t = np.arange(first, last + 1)
            u = t - tau
            inside = np.abs(u) < W/2
            if not inside.any():
                continue
            q = np.array([float(v @ front), float(v @ left), float(v[2])])
            dots = (P @ q)/d
            j = int(np.argmax(dots))                                                    # the first of equals
            if margins is not None:
                other = (P != P[j]).any(axis=1)
                margins.append(float(dots[j] - dots[other].max()) if other.any() else math.inf)
            if used is not None:
                used.add(j)
            x[:, j, t[inside]] += (A/(4*math.pi*d))[:, None]*(np.sinc(u[inside])*(1 + np.cos(2*math.pi*u[inside]/W))/2)
    return x


def fold(x, hrirs):
    """``(K, 2, T)``: ``y_{k,e}[t] = sum_j sum_m H[j, e, m] x_{k,j}[t - m]``."""
    K, D, T = x.shape
    y = np.zeros((K, 2, T))
    for k in range(K):
        for e in range(2):
            for j in range(D):
                if x[k, j].any():
                    y[k, e] += np.convolve(x[k, j], hrirs[j, e])[:T]
    return y


def brir(dims, beta, head, yaw, angle, distance, taps, fs, directions, hrirs, window=None, max_order=-1, c=343.0,
         N=None, used=None):
    """``((taps, 2) float64, margins)``: left and right, and the per-image margins of ``direction_rows``. ``beta`` is
    (6,) or (K, 6); the source is at azimuth ``angle`` degrees (positive is left) at ``distance`` from ``head``, at
    its height."""
    N = B.default_n(fs) if N is None else N
    beta = np.asarray(beta, dtype=np.float64).reshape(-1, 6)
    az = yaw + math.radians(angle)
    source = np.asarray(head, dtype=np.float64) + distance*np.array([math.cos(az), math.sin(az), 0.0])
    margins = []
    x = direction_rows(dims, beta, source, head, yaw, taps, fs, directions, window, max_order, c, N, margins, used)
    y = fold(x, np.asarray(hrirs, dtype=np.float64))
    g = B.bank(fs, len(beta), N)
    return np.stack([B.combine(y[:, e], g, taps, N) for e in range(2)], axis=1), np.array(margins)
