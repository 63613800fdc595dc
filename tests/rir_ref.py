"""The image-source model of DESIGN.md 5m restated in fp64 NumPy: the plain loop over the lattice vector ``n`` and the
parity vector ``p``, one image at a time, no tables and no tiles. The GPU tests compare ``brever_amd.rir`` with it;
tests/test_rir_host.py holds it against closed forms.

    x = (1 - 2p) s + 2 n L          e0 = |n - p|, e1 = |n|          A = prod b0^e0 b1^e1   (0^0 = 1)
    v = x - r, d = |v|, tau = d fs / c, g = a + (1 - a) (v . o) / d
    h[t] += A g / (4 pi d) sinc(t - tau) (1 + cos(2 pi (t - tau) / W)) / 2      for |t - tau| < W/2, 0 <= t < taps
"""
import itertools
import math

import numpy as np


def default_window(fs):
    return float(round(0.008*fs))


def rir(dims, beta, source, receiver, orientation, pattern, taps, fs, window=None, max_order=-1, c=343.0,
        count=None):
    """``(taps,)`` float64. ``count``: an optional list that receives the number of images that touched a tap."""
    L = np.asarray(dims, dtype=np.float64)
    b = np.asarray(beta, dtype=np.float64).reshape(3, 2)
    s, r, o = (np.asarray(v, dtype=np.float64) for v in (source, receiver, orientation))
    W = default_window(fs) if window is None else float(window)
    h = np.zeros(taps)
    reach = (taps - 1 + W/2)*c/fs
    # every image nearer than `reach` has |n| within these bounds: |x - r| >= 2 |n| L - 2 L per axis
    N = [int(math.ceil(reach/(2*L[k]))) + 1 for k in range(3)]
    images = 0
    for n in itertools.product(*(range(-N[k], N[k] + 1) for k in range(3))):
        n = np.array(n)
        for p in itertools.product((0, 1), repeat=3):
            p = np.array(p)
            e0, e1 = np.abs(n - p), np.abs(n)
            if max_order >= 0 and int(e0.sum() + e1.sum()) > max_order:
                continue
            A = float(np.prod(b[:, 0]**e0)*np.prod(b[:, 1]**e1))            # numpy: 0.0**0 = 1.0
            if A == 0.0:
                continue
            v = (1 - 2*p)*s + 2*n*L - r
            d = math.sqrt(float(v[0]*v[0] + v[1]*v[1] + v[2]*v[2]))
            tau = d*fs/c
            first, last = max(int(math.floor(tau - W/2)), 0), min(int(math.ceil(tau + W/2)), taps - 1)
            if first > last:
                continue
            t = np.arange(first, last + 1)
            u = t - tau
            inside = np.abs(u) < W/2
            if not inside.any():
                continue
            g = pattern + (1 - pattern)*float(v @ o)/d
            h[t[inside]] += A*g/(4*math.pi*d)*np.sinc(u[inside])*(1 + np.cos(2*math.pi*u[inside]/W))/2
            images += 1
    if count is not None:
        count.append(images)
    return h


def head_geometry(head, yaw, angle, distance, head_radius=0.0875):
    """``(source, (left ear, right ear), (left orientation, right orientation))`` of a head at ``head`` looking along
    ``(cos yaw, sin yaw, 0)`` with a source at azimuth ``angle`` degrees (counter-clockwise from above: positive is
    left) at ``distance`` and at the ears' height."""
    hc = np.asarray(head, dtype=np.float64)
    side = np.array([-math.sin(yaw), math.cos(yaw), 0.0])
    az = yaw + math.radians(angle)
    source = hc + distance*np.array([math.cos(az), math.sin(az), 0.0])
    return source, (hc + head_radius*side, hc - head_radius*side), (side, -side)


def brir(dims, beta, head, yaw, angle, distance, taps, fs, ear_pattern=0.75, head_radius=0.0875, **kw):
    """``(taps, 2)`` float64: left, right."""
    source, ears, sides = head_geometry(head, yaw, angle, distance, head_radius)
    return np.stack([rir(dims, beta, source, ears[e], sides[e], ear_pattern, taps, fs, **kw) for e in range(2)], axis=1)


def bound(h_ref):
    """The parity bound of the GPU tests: one fp32 output rounding with a factor two of slack, relative to the
    response's peak."""
    return 2.0**-23*float(np.abs(h_ref).max())


def last_tile_images(rows, index, job, taps, fs, window, less=0.0, more=0.0, c=343.0, tile=128):
    """Images of a job's band tables (rows of ``3 + K`` doubles, the squared offset in column 2) that the tile kernels
    list for the last tile of a row of ``taps`` taps: those at a distance that can land inside a window of a tap of
    that tile, an image at distance ``d`` arriving at ``(d + delta) fs / c`` with ``-less <= delta <= more``."""
    hdr, nx, ny, nz = (int(v) for v in index[job, :4])
    x, y, z = (rows[first:first + n, 2] for first, n in ((hdr + 1, nx), (hdr + 1 + nx, ny), (hdr + 1 + nx + ny, nz)))
    t0 = (taps - 1)//tile*tile
    lo = max((t0 - window/2 - 1e-6)*c/fs - less, 0.0)
    hi = (taps - 1 + window/2 + 1e-6)*c/fs + more
    d2 = x[:, None, None] + y[None, :, None] + z[None, None, :]
    return int(((d2 >= lo*lo) & (d2 <= hi*hi)).sum())
