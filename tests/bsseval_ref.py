"""fp64 restatements of the BSS-eval triple SDR / SIR / SAR with an allowed distortion filter of ``L`` taps per
reference for the tests of ``bss_eval`` and the ``sir`` / ``sar`` metrics. Two independent formulations
of the same definition:

(a) ``tables_lstsq``: the explicit ``(T + L - 1) x J L`` shift matrix of all references, ``numpy.linalg.lstsq`` for
    the projection on their span and on the span of each reference alone, and the energies of ``P_j x``,
    ``P_all x - P_j x`` and ``x - P_all x``;
(b) ``tables_gram``: the correlation lags, the assembled ``J L x J L`` block-Toeplitz matrix and
    ``scipy.linalg.solve``, giving ``qJ`` and ``q1``.

``block_levinson`` restates the recursion of the kernel (csrc/sdr/bsseval.cuh) in NumPy, ``best_permutation`` is the
brute force over the ``S!`` assignments, ``signals`` is the recipe of the GPU tests. NumPy / SciPy on the CPU only.
"""
import functools
import itertools

import numpy as np
import scipy.linalg
import scipy.signal

from sdr_ref import lags, shift_matrix

EPS = 2.0**-52
FLOOR_DB = 10.0*np.log10(2.0**52)
KINDS = ('white', 'ar2', 'corr')
NOISE_DB = (0.0, 40.0)
TAPS = np.array([0.9, 0.35, -0.2, 0.1])          # the 4-tap filtering of its target that every estimate carries
CORR_TAPS = np.array([0.5, 0.3, -0.2])           # s_1 of the correlated pair is this filtering of s_0 plus 0.1 w
LEAK = 0.3                                       # weight of every other reference in an estimate
# the pivot rule of the kernel: a pivot d of a J x J factorisation counts as not positive unless d > 2^-40 a_ii
PIVOT_TOL = 2.0**-40
# the loading of the loaded cases: it reaches the library as a C float, and its fp32 value is what enters R
LOAD = float(np.float32(1e-3))


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def signals(kind, J, S, T, noise_db, seed=0):
    """``(references (J, T), estimates (S, T))``, float64 holding fp32-representable values. The references are white,
    AR(2) ``1/(1 - 1.8 z^-1 + 0.9 z^-2)``, or white with ``s_1 = fir(CORR_TAPS) s_0 + 0.1 w``; estimate ``e`` is the
    4-tap filtering of reference ``e`` plus ``LEAK`` times every other reference plus white noise ``noise_db`` below
    the filtered target."""
    rng = np.random.default_rng([seed, KINDS.index(kind), J, S, T, int(noise_db)])
    w = rng.standard_normal((J, T + 200))
    if kind == 'ar2':
        w = scipy.signal.lfilter([1.0], [1.0, -1.8, 0.9], w, axis=-1)
    elif kind == 'corr':
        w[1] = scipy.signal.lfilter(CORR_TAPS, [1.0], w[0]) + 0.1*w[1]
    s = w[:, 200:]
    s = _f32(s/np.maximum(np.sqrt(np.mean(s**2, axis=-1, keepdims=True)), 1e-30)*0.1)
    x = np.zeros((S, T))
    for e in range(S):
        f = np.convolve(s[e], TAPS)[:T]
        n = rng.standard_normal(T)
        n *= np.linalg.norm(f)/max(np.linalg.norm(n), 1e-30)*10.0**(-noise_db/20.0)
        x[e] = f + LEAK*(s.sum(axis=0) - s[e]) + n
    return s, _f32(x)


def lowpass_pair(T, seed=0):
    """``(references (2, T), estimates (2, T))`` with two independent 6th-order Butterworth low-pass references
    (0.25 of Nyquist): the stop band makes ``G`` ill-conditioned, the more the longer ``T`` and ``L``, so this pair is
    only ever scored with a loading."""
    rng = np.random.default_rng([seed, 99, T])
    w = scipy.signal.lfilter(*scipy.signal.butter(6, 0.25), rng.standard_normal((2, T + 200)), axis=-1)[:, 200:]
    s = _f32(w/np.sqrt(np.mean(w**2, axis=-1, keepdims=True))*0.1)
    x = np.stack([np.convolve(s[e], TAPS)[:T] + LEAK*s[1 - e] + 0.01*0.1*rng.standard_normal(T) for e in range(2)])
    return s, _f32(x)


def _db(num, den, E):
    return 10.0*np.log10(max(num, EPS*E)/max(den, EPS*E))


def _project(A, x_pad, load):
    """Energy captured by the least-squares projection of ``x_pad`` on the columns of ``A``; with the loading
    ``load`` (one value per column: the squared extra rows) it is ``x_pad^T A c`` of the loaded problem."""
    if load is None:
        c = np.linalg.lstsq(A, x_pad, rcond=None)[0]
        p = A @ c
        return float(np.dot(p, p)), p
    n = A.shape[1]
    Al = np.concatenate([A, np.diag(np.sqrt(load))])
    c = np.linalg.lstsq(Al, np.concatenate([x_pad, np.zeros(n)]), rcond=None)[0]
    p = A @ c
    return float(np.dot(x_pad, p)), p


def tables_lstsq(s, x, L, load_diag=0.0):
    """Formulation (a). ``s``: (J, T), ``x``: (S, T). Returns ``(sdr (S, J), sir (S, J), sar (S,))`` in dB. Unloaded,
    every ratio is one of energies of explicit residual vectors; loaded, of the ``q`` of the loaded problems."""
    s, x = np.asarray(s, dtype=np.float64), np.asarray(x, dtype=np.float64)
    J, T = s.shape
    S = x.shape[0]
    mats = [shift_matrix(s[j], L) for j in range(J)]
    # column (m, j) -> m*J + j, the ordering of the block system
    A = np.stack(mats, axis=2).reshape(T + L - 1, L*J)
    r0 = np.array([np.dot(s[j], s[j]) for j in range(J)])
    sdr, sir, sar = np.full((S, J), np.nan), np.full((S, J), np.nan), np.full(S, np.nan)
    for e in range(S):
        x_pad = np.concatenate([x[e], np.zeros(L - 1)])
        E = float(np.dot(x[e], x[e]))
        if load_diag:
            qJ, p_all = _project(A, x_pad, np.tile(load_diag*r0, L))
            sar[e] = _db(qJ, E - qJ, E)
        else:
            qJ, p_all = _project(A, x_pad, None)
            res = x_pad - p_all
            sar[e] = _db(qJ, float(np.dot(res, res)), E)
        for j in range(J):
            if load_diag:
                q1, _ = _project(mats[j], x_pad, np.full(L, load_diag*r0[j]))
                sdr[e, j], sir[e, j] = _db(q1, E - q1, E), _db(q1, qJ - q1, E)
            else:
                q1, p1 = _project(mats[j], x_pad, None)
                d, i = x_pad - p1, p_all - p1
                sdr[e, j], sir[e, j] = _db(q1, float(np.dot(d, d)), E), _db(q1, float(np.dot(i, i)), E)
    return sdr, sir, sar


def block_lags(s, x, L):
    """``R (L, J, J)`` with ``R[l][i][j] = r_ij[l]`` for ``l >= 0`` (``R(-l) = R(l)^T``) and ``d (S, L, J)`` with
    ``d[e][k][j] = b_je[k]``."""
    J, S = len(s), len(x)
    R, d = np.zeros((L, J, J)), np.zeros((S, L, J))
    for i in range(J):
        for j in range(J):
            R[:, i, j] = lags(s[i], s[j], L)[1]
    for e in range(S):
        for j in range(J):
            d[e, :, j] = lags(s[j], x[e], L)[1]
    return R, d


def gram(R, load_diag=0.0):
    """The ``J L x J L`` block-Toeplitz matrix ``G[(k, i), (m, j)] = R(k - m)[i][j]`` with the loading on its
    diagonal."""
    L, J, _ = R.shape
    G = np.zeros((L, J, L, J))
    for k in range(L):
        for m in range(L):
            G[k, :, m, :] = R[k - m] if k >= m else R[m - k].T
    G = G.reshape(L*J, L*J)
    return G + load_diag*np.diag(np.tile(np.diag(R[0]), L))


def _tables_from_q(q1, qJ, E):
    S, J = q1.shape
    sdr, sir, sar = np.full((S, J), np.nan), np.full((S, J), np.nan), np.full(S, np.nan)
    for e in range(S):
        sar[e] = _db(qJ[e], E[e] - qJ[e], E[e])
        for j in range(J):
            sdr[e, j], sir[e, j] = _db(q1[e, j], E[e] - q1[e, j], E[e]), _db(q1[e, j], qJ[e] - q1[e, j], E[e])
    return sdr, sir, sar


def tables_gram(s, x, L, load_diag=0.0, solver='dense', with_cond=True):
    """Formulation (b), or with ``solver='levinson'`` the NumPy restatement of the kernel's recursion for ``qJ``.
    Returns ``(sdr, sir, sar, cond(G))``; the condition number only for the dense solver and ``with_cond``."""
    s, x = np.asarray(s, dtype=np.float64), np.asarray(x, dtype=np.float64)
    J, S = len(s), len(x)
    R, d = block_lags(s, x, L)
    E = np.array([np.dot(x[e], x[e]) for e in range(S)])
    q1 = np.zeros((S, J))
    for j in range(J):
        Rj = scipy.linalg.toeplitz(R[:, j, j]) + load_diag*R[0, j, j]*np.eye(L)
        for e in range(S):
            q1[e, j] = np.dot(d[e, :, j], scipy.linalg.solve(Rj, d[e, :, j], assume_a='pos'))
    if solver == 'levinson':
        qJ, ok = block_levinson(R, d, load_diag)
        assert ok
        cond = float('nan')
    else:
        G = gram(R, load_diag)
        rhs = d.reshape(S, L*J).T
        qJ = np.einsum('ke,ke->e', rhs, scipy.linalg.solve(G, rhs, assume_a='pos'))
        cond = float(np.linalg.cond(G)) if with_cond else float('nan')
    return (*_tables_from_q(q1, qJ, E), cond)


def _ldl(A):
    """``(L, 1/d, ok)`` of ``A = L diag(d) L^T`` from the lower triangle, with the kernel's pivot rule."""
    J = len(A)
    Lf, dinv = np.eye(J), np.zeros(J)
    for i in range(J):
        v = A[i, i] - sum(Lf[i, k]*Lf[i, k]/dinv[k] for k in range(i))
        if not v > PIVOT_TOL*A[i, i]:
            return Lf, dinv, False
        dinv[i] = 1.0/v
        for r in range(i + 1, J):
            Lf[r, i] = (A[r, i] - sum(Lf[r, k]*Lf[i, k]/dinv[k] for k in range(i)))*dinv[i]
    return Lf, dinv, True


def _ldl_solve(Lf, dinv, rhs):
    y = scipy.linalg.solve_triangular(Lf, rhs, lower=True, unit_diagonal=True)
    return scipy.linalg.solve_triangular(Lf.T, y*dinv[:, None], lower=False, unit_diagonal=True)


def block_levinson(R, d, load_diag=0.0):
    """The Whittle-Wiggins-Robinson recursion as the kernel runs it. ``R``: (L, J, J), ``d``: (S, L, J). Returns
    ``(qJ (S,), ok)``; ``ok`` is False where a pivot is not positive."""
    L, J, _ = R.shape
    S = len(d)
    R = R.copy()
    R[0] = R[0] + load_diag*np.diag(np.diag(R[0]))
    F, B, C = np.zeros((L, J, J)), np.zeros((L, J, J)), np.zeros((L, J, S))
    F[0] = B[0] = np.eye(J)
    Ef, Eb = R[0].copy(), R[0].copy()
    fb, ib, ok = _ldl(Eb)
    if not ok:
        return np.full(S, np.nan), False
    ff, if_ = fb, ib
    # one step of iterative refinement: an estimate that is a reference times a power of two gets C[0] exactly
    d0 = d[:, 0, :].T
    C[0] = _ldl_solve(fb, ib, d0)
    C[0] += _ldl_solve(fb, ib, d0 - R[0] @ C[0])
    q = np.einsum('je,je->e', d0, C[0])
    for n in range(L - 1):
        # lane m holds F[m], C[m] and reads B[m - 1]: Df over m <= n, Db over 1 <= m <= n + 1
        Df = sum(R[n + 1 - m] @ F[m] for m in range(n + 1))
        Db = sum(R[m].T @ B[m - 1] for m in range(1, n + 2))
        eps = d[:, n + 1, :].T - sum(R[n + 1 - m] @ C[m] for m in range(n + 1))
        Kf, Kb = _ldl_solve(fb, ib, Df), _ldl_solve(ff, if_, Db)
        Ef, Eb = Ef - Db @ Kf, Eb - Df @ Kb
        ff, if_, ok_f = _ldl(Ef)
        fb, ib, ok_b = _ldl(Eb)
        if not (ok_f and ok_b):
            return np.full(S, np.nan), False
        g = _ldl_solve(fb, ib, eps)
        Bs = np.concatenate([np.zeros((1, J, J)), B[:n + 1]])            # [0, B]
        Fn = F[:n + 2] - Bs @ Kf
        Bn = Bs - F[:n + 2] @ Kb
        F[:n + 2], B[:n + 2] = Fn, Bn
        C[:n + 2] += Bn @ g
        q = q + np.einsum('je,je->e', eps, g)          # d'^T C' - d^T C = eps^T Eb'^-1 eps
    assert np.allclose(q, np.einsum('ekj,kje->e', d, C), rtol=1e-9)
    return q, True


def best_permutation(sir, S):
    """The bijection ``p`` of the ``S`` estimates onto the first ``S`` references with the largest
    ``sum_e sir[e][p(e)]``, the lexicographically smallest among equals; the identity where the table holds a NaN."""
    if np.isnan(sir).any():
        return tuple(range(S))
    best, best_sum = None, -np.inf
    for p in itertools.permutations(range(S)):
        total = 0.0
        for e in range(S):
            total += sir[e][p[e]]
        if total > best_sum:
            best, best_sum = p, total
    return best


# the (J, S, T, L) cases of tests/test_gpu_bsseval.py (CHUNK as in sdr_ref) and the (kind, noise dB) rows of each
CHUNK = 2048
CASES = ((2, 1, 3000, 512), (2, 2, 700, 512), (2, 2, 300, 512), (2, 1, 3000, 1), (3, 3, 3000, 33), (4, 2, 1500, 64),
         (2, 2, CHUNK - 1, 64), (2, 2, CHUNK, 64), (2, 2, CHUNK + 1, 64), (4, 4, 2500, 512))
VARIANTS = tuple((kind, db) for kind in KINDS for db in NOISE_DB)


def case_load(case):
    """``load_diag`` of a case. With ``T + L - 1 < J L`` the shifted references are linearly dependent and the joint
    system is singular, so the ``T < L`` case runs loaded, against the references with the same loading."""
    J, S, T, L = case
    return LOAD if T + L - 1 < J*L else 0.0


def case_rows(case):
    """The (kind, noise dB) rows of a case: all six, but two at the largest state, whose least-squares reference
    costs seconds per row."""
    return (('ar2', 40.0), ('corr', 0.0)) if case == (4, 4, 2500, 512) else VARIANTS


@functools.lru_cache(maxsize=None)
def reference(case, kind, db):
    """``(s, x, (sdr, sir, sar) of (a))`` of one row, computed once per process and shared read-only."""
    J, S, T, L = case
    s, x = signals(kind, J, S, T, db)
    out = tables_lstsq(s, x, L, case_load(case))
    for a in (s, x, *out):
        a.setflags(write=False)
    return s, x, out


# The reference spread: the largest |(a) - (b)| in dB over every table entry of every row of CASES
# (tests/test_bsseval_host.py prints each; 3.88e-10 dB at (2, 2, 700, 512), AR(2), 40 dB, cond(G) 6.9e6). The GPU's
# tables are held to 8 times it against (a). The NumPy restatement of the recursion lies within 1.05e-9 dB of (a).
REF_SPREAD = 3.9e-10
FORWARD_BOUND = 8*REF_SPREAD
COND_LIMIT = 1e7
