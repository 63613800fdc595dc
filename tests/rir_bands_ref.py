"""The band model of DESIGN.md 5n restated in fp64 NumPy: the plain loop over the lattice vector ``n`` and the parity
vector ``p``, one image at a time, with a filter design of its own; no code of ``brever_amd``. The GPU tests compare
``brever_amd.rir`` with it; tests/test_rir_bands_host.py holds it against closed forms.

    x = (1 - 2p) s + 2 n L        e0 = |n - p|, e1 = |n|        A_k = prod b_k0^e0 b_k1^e1   (0^0 = 1), beta (K, 6)
    v = x - r, d = |v|
    pattern   g = a + (1 - a) (v . o) / d, tau = d fs / c, channels k: A_k g / (4 pi d)
    sphere    theta = acos(clamp((v . o) / d)), alpha = 1.05 + 0.95 cos(1.2 theta),
              delta = -rad cos(theta) if theta < pi/2 else rad (theta - pi/2), tau = (d + delta) fs / c,
              channels k: A_k alpha / (4 pi d), channels K + k: A_k (1 - alpha) / (4 pi d)
    x_c[t] += amplitude_c sinc(t - tau) (1 + cos(2 pi (t - tau) / W)) / 2     for |t - tau| < W/2, 0 <= t < taps + N/2
    h[t] = sum_c sum_m f_c[m] x_c[t + N/2 - m],  0 <= t < taps;   f_c = g_k, and g_k * lp for the channels K + k
"""
import itertools
import math

import numpy as np

AMIN, THETA_MIN = 0.1, 150.0


def default_window(fs):
    return float(round(0.008*fs))


def default_n(fs):
    return 2**math.ceil(math.log2(fs/62.5))


def bank(fs, K, N=None):
    """``(K, N)``: the band filters ``g_k``."""
    N = default_n(fs) if N is None else N
    fc = [125.0*2**k for k in range(K)]
    G = np.zeros((K, N//2 + 1))
    for b in range(N//2 + 1):
        f = b*fs/N
        if f <= fc[0]:
            G[0, b] = 1.0
        elif f >= fc[K - 1]:
            G[K - 1, b] = 1.0
        else:
            k = max(i for i in range(K) if fc[i] <= f)
            y = math.log2(f/fc[k])
            G[k, b], G[k + 1, b] = math.cos(math.pi*y/2)**2, math.sin(math.pi*y/2)**2
    m = np.arange(N)
    hann = (1 + np.cos(2*np.pi*(m - N/2)/N))/2
    return np.stack([np.fft.fftshift(np.fft.irfft(G[k], N))*hann for k in range(K)])


def lowpass(fs, rad, c=343.0, taps=None):
    """The head low-pass by running its recurrence on an impulse; ``taps`` overrides the truncation."""
    kk = fs*rad/c
    a1 = (1 - kk)/(1 + kk)
    M = math.ceil(40*math.log(2)/-math.log(abs(a1))) if taps is None else taps
    x = np.zeros(M + 1)
    x[0] = 1.0
    y = np.zeros(M)
    for n in range(M):
        y[n] = (x[n] + (x[n - 1] if n else 0.0))/(1 + kk) - (a1*y[n - 1] if n else 0.0)
    return y


def channel_filters(fs, K, sphere, rad=0.0875, c=343.0, N=None):
    g = bank(fs, K, N)
    if not sphere:
        return list(g)
    lp = lowpass(fs, rad, c)
    return list(g) + [np.convolve(gk, lp) for gk in g]


def head_terms(cosang, rad):
    """``(alpha, delta)`` of the spherical head for the cosine of the angle between the ear's axis and the image."""
    theta = math.acos(min(max(cosang, -1.0), 1.0))
    alpha = (1 + AMIN/2) + (1 - AMIN/2)*math.cos(theta*180.0/THETA_MIN)
    delta = -rad*math.cos(theta) if theta < math.pi/2 else rad*(theta - math.pi/2)
    return alpha, delta


def channels(dims, beta, source, receiver, orientation, pattern, taps, fs, sphere=False, rad=0.0875, window=None,
             max_order=-1, c=343.0, N=None, count=None):
    """``(C, taps + N/2)`` float64: the channel responses ``x_c``."""
    L = np.asarray(dims, dtype=np.float64)
    b = np.asarray(beta, dtype=np.float64).reshape(-1, 3, 2)
    K = len(b)
    s, r, o = (np.asarray(v, dtype=np.float64) for v in (source, receiver, orientation))
    W = default_window(fs) if window is None else float(window)
    N = default_n(fs) if N is None else N
    T = taps + N//2
    x = np.zeros((2*K if sphere else K, T))
    reach = (T - 1 + W/2)*c/fs + (rad if sphere else 0.0)
    M = [int(math.ceil(reach/(2*L[k]))) + 1 for k in range(3)]
    images = 0
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
            cosang = float(v @ o)/d
            if sphere:
                alpha, delta = head_terms(cosang, rad)
                tau = (d + delta)*fs/c
                amps = np.concatenate([A*alpha, A*(1 - alpha)])/(4*math.pi*d)
            else:
                tau = d*fs/c
                amps = A*(pattern + (1 - pattern)*cosang)/(4*math.pi*d)
            first, last = max(int(math.floor(tau - W/2)), 0), min(int(math.ceil(tau + W/2)), T - 1)
            if first > last:
                continue
            t = np.arange(first, last + 1)
            u = t - tau
            inside = np.abs(u) < W/2
            if not inside.any():
                continue
            x[:, t[inside]] += amps[:, None]*(np.sinc(u[inside])*(1 + np.cos(2*math.pi*u[inside]/W))/2)[None, :]
            images += 1
    if count is not None:
        count.append(images)
    return x


def combine(x, filters, taps, N):
    """``h[t] = sum_c sum_m f_c[m] x_c[t + N/2 - m]`` for ``0 <= t < taps``."""
    h = np.zeros(taps)
    for xc, f in zip(x, filters):
        full = np.convolve(xc, f)                        # full[j] = sum_m f[m] xc[j - m]
        h += full[N//2:N//2 + taps]
    return h


def rir(dims, beta, source, receiver, orientation, pattern, taps, fs, sphere=False, rad=0.0875, window=None,
        max_order=-1, c=343.0, N=None, count=None):
    """``(taps,)`` float64. ``beta`` is (K, 6); in sphere mode ``receiver`` is the head's centre and ``orientation``
    the ear's outward axis."""
    N = default_n(fs) if N is None else N
    K = len(np.asarray(beta, dtype=np.float64).reshape(-1, 6))
    x = channels(dims, beta, source, receiver, orientation, pattern, taps, fs, sphere, rad, window, max_order, c, N,
                 count)
    return combine(x, channel_filters(fs, K, sphere, rad, c, N), taps, N)


def head_geometry(head, yaw, angle, distance, head_radius=0.0875):
    """``(source, (left ear, right ear), (left axis, right axis))``: a head at ``head`` looking along
    ``(cos yaw, sin yaw, 0)``, a source at azimuth ``angle`` degrees (positive is left) at ``distance``."""
    hc = np.asarray(head, dtype=np.float64)
    side = np.array([-math.sin(yaw), math.cos(yaw), 0.0])
    az = yaw + math.radians(angle)
    source = hc + distance*np.array([math.cos(az), math.sin(az), 0.0])
    return source, (hc + head_radius*side, hc - head_radius*side), (side, -side)


def brir(dims, beta, head, yaw, angle, distance, taps, fs, sphere=False, ear_pattern=0.75, head_radius=0.0875, **kw):
    """``(taps, 2)`` float64: left, right. Pattern mode: the ears are receivers at ``head_radius`` from the centre.
    Sphere mode: the receiver is the centre for both ears."""
    source, ears, sides = head_geometry(head, yaw, angle, distance, head_radius)
    return np.stack([rir(dims, beta, source, head if sphere else ears[e], sides[e], ear_pattern, taps, fs, sphere,
                         head_radius, **kw) for e in range(2)], axis=1)
