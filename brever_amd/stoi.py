"""STOI / ESTOI on the HIP path: the forward that the metric (``metrics.py``) and the training criteria
(``criterion.py``: ``StoiLoss`` / ``EstoiLoss``) share, and the criteria's backward.

The forward is five launches of ``libbrever_hip.so`` (``csrc/stoi.hip``) on the whole padded batch: polyphase
resampling to 10 kHz, silent-frame removal, a 512-point DFT of the 256-sample Hann frames as one exact-fp32 product,
one-third octave band magnitudes, segment correlations. The backward runs in ``libbrever_stoi_loss.so``
(include/brever_stoi_loss.h; csrc/stoi_loss/stoi_loss.hip) and goes the same way back:

    segment tiles' gradients                                     brv_sl_segment_backward
    their sum per (band, frame), through the band magnitude      brv_sl_bands_backward
    frame gradient = spectrum gradient x basis^T                 brv_gemm_f32, trans_b = 1
    frames folded onto the compacted signal                      brv_sl_fold_frames
    back to the frames that were kept                            brv_sl_compact_backward
    adjoint of the resampler (not at 10 kHz)                     brv_sl_resample_backward

Only the estimate gets a gradient; frame selection and everything computed from the target are constants. Every
stage is a gather in a fixed order, so a gradient is bitwise repeatable. ``lengths`` stays on the device; nothing
here synchronises. There is no CPU fallback: without the libraries or a ROCm device the calls raise.
"""
import math

import numpy as np
import torch

from . import hip

FS, NFFT, FRAME, BANDS, MINFREQ, SEGMENT = 10000, 512, 256, 15, 150, 30
HOP = FRAME//2
DYN_RANGE = 40.0
CLIP = 10.0**(15.0/20.0)
# brv_gemm_f32 splits a reduction over workgroups that add with atomics only from 16 chunks of 32 on; the frame
# gradient reduces over the 2 x 212 spectrum columns, 14 chunks, so the plain call keeps a fixed order
_GEMM_SPLIT_FROM = 16*32


# the brv_sl_* entry points of include/brever_stoi_loss.h
_LIB = hip.Library('brever_stoi_loss.h', 'libbrever_stoi_loss.so', 'BRV_STOI_LOSS_LIB_PATH',
                   'The STOI / ESTOI criteria have no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES, lib, call = _LIB.path, _LIB.header_path, _LIB.signatures, _LIB.lib, _LIB.call


_cache = {}


def constants(device, fs):
    """Band edges, the windowed DFT basis and, off 10 kHz, the padded polyphase filter, on ``device``."""
    key = (str(device), fs)
    if key in _cache:
        return _cache[key]
    # one-third octave band edges on the 512-point DFT grid (Taal et al. 2011)
    f = np.linspace(0, FS, NFFT + 1)[:NFFT//2 + 1]
    k = np.arange(BANDS, dtype=float)
    lo = MINFREQ*2.0**((2*k - 1)/6)
    hi = MINFREQ*2.0**((2*k + 1)/6)
    edges = np.array([[int(np.argmin((f - a)**2)), int(np.argmin((f - b)**2))]
                      for a, b in zip(lo, hi)], dtype=np.int32)
    bin0, bin1 = int(edges[:, 0].min()), int(edges[:, 1].max())
    m = np.arange(FRAME)
    window = np.hanning(FRAME + 2)[1:-1]
    ang = 2*np.pi*np.outer(m, np.arange(bin0, bin1))/NFFT
    basis = np.empty((FRAME, 2*(bin1 - bin0)), dtype=np.float64)
    basis[:, 0::2] = window[:, None]*np.cos(ang)
    basis[:, 1::2] = -window[:, None]*np.sin(ang)
    out = {'edges': torch.from_numpy(edges).to(device), 'bin0': bin0,
           'basis': torch.from_numpy(basis).float().to(device)}
    if fs != FS:
        # Octave-style Kaiser polyphase filter of pystoi's resample_oct, then padded and scaled
        # the way scipy.signal.resample_poly applies a given window
        g = math.gcd(FS, fs)
        up, down = FS//g, fs//g
        cutoff = 1.0/(2*max(up, down))
        L = int(np.ceil((60.0 - 8)/(28.714*cutoff/10)))
        t = np.arange(-L, L + 1)
        h = np.kaiser(2*L + 1, 0.1102*(60.0 - 8.7))*2*up*cutoff*np.sinc(2*cutoff*t)
        h = h/np.sum(h)*up
        half = (len(h) - 1)//2
        n_pre_pad = down - half % down
        out.update(up=up, down=down, n_pre_remove=(half + n_pre_pad)//down,
                   hpad=torch.from_numpy(np.concatenate([np.zeros(n_pre_pad), h])).float().to(device))
    _cache[key] = out
    return out


def forward(x, y, fs, extended, lengths):
    """``x``: estimate, ``y``: target, ``(R, L)`` contiguous fp32 on the GPU; ``lengths``: ``(R,)`` int64 on the
    GPU. Returns ``(value, saved)``: the ``(R,)`` fp32 STOI / ESTOI of every row and what the backward needs."""
    R, L = x.shape
    dev = x.device
    c = constants(dev, int(fs))
    st = hip.stream()
    sig = torch.stack([y, x]).reshape(2*R, L)                  # clean rows first
    saved = {'fs': int(fs), 'extended': bool(extended), 'L': L, 'lengths_in': lengths}
    if fs != FS:
        n10 = -(-L*c['up']//c['down'])
        res = torch.empty(2*R, n10, dtype=torch.float32, device=dev)
        len2 = torch.cat([lengths, lengths])
        hip.call('brv_resample_poly', sig, c['hpad'], res, len2, 2*R, L, n10, c['up'], c['down'], c['hpad'].numel(),
                 c['n_pre_remove'], st)
        sig, L = res, n10
        lengths = -(-lengths*c['up']//c['down'])
    nf_max = max(int(hip.lib().brv_stoi_frames(L)), 1)
    out_stride = FRAME + nf_max*HOP
    comp = torch.empty(2*R, out_stride, dtype=torch.float32, device=dev)
    geom = torch.empty(R, 4, dtype=torch.int32, device=dev)
    energy = torch.empty(R, nf_max, dtype=torch.float32, device=dev)
    kept = torch.empty(R, nf_max, dtype=torch.int32, device=dev)
    hip.call('brv_stoi_compact', sig[:R], sig[R:], lengths, R, L, comp[:R], comp[R:], out_stride, geom, energy, kept,
             nf_max, DYN_RANGE, st)
    ncols = c['basis'].shape[1]
    spec = torch.empty(2*R, nf_max, ncols, dtype=torch.float32, device=dev)
    # frames are rows of the compacted signals 128 samples apart: one product for all items
    hip.call('brv_gemm_f32', comp, c['basis'], spec, 2*R, nf_max, ncols, FRAME, HOP, ncols, ncols,
             out_stride, 0, nf_max*ncols, 0, 0, 1, 0, 0, None, 0, st)
    tob = torch.empty(2*R, BANDS, nf_max, dtype=torch.float32, device=dev)
    hip.call('brv_stoi_bands', spec, c['edges'], tob, 2*R, nf_max, ncols, c['bin0'], st)
    partial = torch.empty(R, max(nf_max - SEGMENT + 1, 1), dtype=torch.float32, device=dev)
    out = torch.empty(R, dtype=torch.float32, device=dev)
    hip.call('brv_stoi_correlate', tob[:R], tob[R:], geom, partial, out, R, nf_max, int(bool(extended)), CLIP, st)
    saved.update(kept=kept, geom=geom, spec=spec[R:], tob=tob, lengths10=lengths, L10=L, nf_max=nf_max,
                 out_stride=out_stride)
    return out, saved


def backward(saved, grad_rows):
    """Gradient ``(R, L)`` fp32 of ``sum(grad_rows * -value)`` with respect to the estimate, from what ``forward``
    saved; ``grad_rows``: ``(R,)`` contiguous fp32. Zero at and beyond every row's length."""
    spec, tob, geom, kept = saved['spec'], saved['tob'], saved['geom'], saved['kept']
    R, nf_max, ncols = spec.shape
    dev = spec.device
    c = constants(dev, saved['fs'])
    st = hip.stream()
    if ncols >= _GEMM_SPLIT_FROM:
        raise RuntimeError(f'the frame gradient reduces over {ncols} columns: brv_gemm_f32 would split it')
    f32 = dict(dtype=torch.float32, device=dev)
    seg = torch.empty(R, max(nf_max - SEGMENT + 1, 1), BANDS, SEGMENT, **f32)
    call('brv_sl_segment_backward', tob[:R], tob[R:], geom, grad_rows, seg, R, nf_max, int(saved['extended']),
         CLIP, st)
    dband = torch.empty(R, BANDS, nf_max, **f32)
    dspec = torch.empty(R, nf_max, ncols, **f32)
    call('brv_sl_bands_backward', seg, tob[R:], spec, c['edges'], geom, dband, dspec, R, nf_max, ncols, c['bin0'], st)
    dframes = torch.empty(R, nf_max, FRAME, **f32)
    hip.call('brv_gemm_f32', dspec, c['basis'], dframes, R, nf_max, FRAME, ncols, ncols, ncols, FRAME,
             nf_max*ncols, 0, nf_max*FRAME, 0, 1, 1, 0, 0, None, 0, st)
    dcomp = torch.empty(R, saved['out_stride'], **f32)
    call('brv_sl_fold_frames', dframes, geom, dcomp, R, nf_max, saved['out_stride'], st)
    d10 = torch.empty(R, saved['L10'], **f32)
    call('brv_sl_compact_backward', dcomp, kept, geom, saved['lengths10'], d10, R, nf_max, saved['out_stride'],
         saved['L10'], st)
    if saved['fs'] == FS:
        return d10
    dx = torch.empty(R, saved['L'], **f32)
    call('brv_sl_resample_backward', d10, c['hpad'], saved['lengths_in'], dx, R, saved['L'], saved['L10'], c['up'],
         c['down'], c['hpad'].numel(), c['n_pre_remove'], st)
    return dx
