"""Evaluation metrics (reference brever/metrics.py:16-150): the same registry keys and call
signatures -- ``metric(x, y, ..., lengths=None)`` with ``x`` the processed signal and ``y`` the
clean target, batched ``(B, L)`` or single ``(L,)``.

* ``snr`` / ``sisnr``: minus the HIP criteria;
* ``stoi`` / ``estoi``: the reference calls the ``pystoi`` / ``batch_pystoi`` wheels (absent from
  this image, not under the reference tree). Here the published algorithm runs as HIP kernels
  (``csrc/stoi.hip``: polyphase resampling to 10 kHz, silent-frame removal, one-third octave band
  magnitudes through an exact-fp32 MFMA DFT product, segment correlations) for the whole padded
  batch at once. Checked against ``oracle/stoi.py``; parity with the wheels themselves is
  **unpinned**. Results come back as NumPy arrays / floats like the reference's;
* ``pesq``: ITU-T P.862 lives in the third-party ``pesq`` C extension. The key is registered so
  that reference configs resolve; calling it uses the wheel when it is importable and raises a
  clear ``ImportError`` otherwise (``metric_available('pesq')`` tells which).
"""
import math

import numpy as np
import torch

from . import hip
from .criterion import CriterionRegistry
from .registry import Registry

MetricRegistry = Registry('metric')


def metric_available(name):
    """False for registered metrics whose third-party backend is missing (``pesq``)."""
    if name == 'pesq':
        try:
            import pesq  # noqa: F401
        except ImportError:
            return False
    return name in MetricRegistry.keys()


# ---- STOI / ESTOI ------------------------------------------------------------------------------
_STOI_FS, _STOI_NFFT, _STOI_FRAME, _STOI_BANDS, _STOI_MINFREQ = 10000, 512, 256, 15, 150
_stoi_cache = {}


def _stoi_constants(device, fs):
    key = (str(device), fs)
    if key in _stoi_cache:
        return _stoi_cache[key]
    # one-third octave band edges on the 512-point DFT grid (Taal et al. 2011)
    f = np.linspace(0, _STOI_FS, _STOI_NFFT + 1)[:_STOI_NFFT//2 + 1]
    k = np.arange(_STOI_BANDS, dtype=float)
    lo = _STOI_MINFREQ*2.0**((2*k - 1)/6)
    hi = _STOI_MINFREQ*2.0**((2*k + 1)/6)
    edges = np.array([[int(np.argmin((f - a)**2)), int(np.argmin((f - b)**2))]
                      for a, b in zip(lo, hi)], dtype=np.int32)
    bin0, bin1 = int(edges[:, 0].min()), int(edges[:, 1].max())
    m = np.arange(_STOI_FRAME)
    window = np.hanning(_STOI_FRAME + 2)[1:-1]
    ang = 2*np.pi*np.outer(m, np.arange(bin0, bin1))/_STOI_NFFT
    basis = np.empty((_STOI_FRAME, 2*(bin1 - bin0)), dtype=np.float64)
    basis[:, 0::2] = window[:, None]*np.cos(ang)
    basis[:, 1::2] = -window[:, None]*np.sin(ang)
    out = {'edges': torch.from_numpy(edges).to(device), 'bin0': bin0,
           'basis': torch.from_numpy(basis).float().to(device)}
    if fs != _STOI_FS:
        # Octave-style Kaiser polyphase filter of pystoi's resample_oct, then padded and scaled
        # the way scipy.signal.resample_poly applies a given window
        g = math.gcd(_STOI_FS, fs)
        up, down = _STOI_FS//g, fs//g
        cutoff = 1.0/(2*max(up, down))
        L = int(np.ceil((60.0 - 8)/(28.714*cutoff/10)))
        t = np.arange(-L, L + 1)
        h = np.kaiser(2*L + 1, 0.1102*(60.0 - 8.7))*2*up*cutoff*np.sinc(2*cutoff*t)
        h = h/np.sum(h)*up
        half = (len(h) - 1)//2
        n_pre_pad = down - half % down
        out.update(up=up, down=down, n_pre_remove=(half + n_pre_pad)//down,
                   hpad=torch.from_numpy(np.concatenate([np.zeros(n_pre_pad), h])).float().to(device))
    _stoi_cache[key] = out
    return out


def _stoi_hip(x, y, fs, extended, lengths):
    """x: processed, y: clean, (B, L) float tensors on the GPU; lengths: (B,) or None."""
    lib = hip.lib()
    x = x.detach().float().contiguous()
    y = y.detach().float().contiguous()
    hip.require_device(x, y)
    B, L = x.shape
    dev = x.device
    if lengths is None:
        lengths = torch.full((B,), L, dtype=torch.int64, device=dev)
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).contiguous()
    c = _stoi_constants(dev, int(fs))
    st = hip.stream()
    sig = torch.stack([y, x]).reshape(2*B, L)                  # clean rows first
    if fs != _STOI_FS:
        n10 = -(-L*c['up']//c['down'])
        res = torch.empty(2*B, n10, dtype=torch.float32, device=dev)
        len2 = torch.cat([lengths, lengths])
        hip.call('brv_resample_poly', sig, c['hpad'], res, len2, 2*B, L, n10, c['up'], c['down'], c['hpad'].numel(),
                 c['n_pre_remove'], st)
        sig, L = res, n10
        lengths = -(-lengths*c['up']//c['down'])
    nf_max = max(int(lib.brv_stoi_frames(L)), 1)
    out_stride = _STOI_FRAME + nf_max*(_STOI_FRAME//2)
    comp = torch.empty(2*B, out_stride, dtype=torch.float32, device=dev)
    geom = torch.empty(B, 4, dtype=torch.int32, device=dev)
    energy = torch.empty(B, nf_max, dtype=torch.float32, device=dev)
    kept = torch.empty(B, nf_max, dtype=torch.int32, device=dev)
    hip.call('brv_stoi_compact', sig[:B], sig[B:], lengths, B, L, comp[:B], comp[B:], out_stride, geom, energy, kept,
             nf_max, 40.0, st)
    ncols = c['basis'].shape[1]
    spec = torch.empty(2*B, nf_max, ncols, dtype=torch.float32, device=dev)
    # frames are rows of the compacted signals 128 samples apart: one product for all items
    hip.call('brv_gemm_f32', comp, c['basis'], spec, 2*B, nf_max, ncols, _STOI_FRAME, _STOI_FRAME//2, ncols, ncols,
             out_stride, 0, nf_max*ncols, 0, 0, 1, 0, 0, None, 0, st)
    tob = torch.empty(2*B, _STOI_BANDS, nf_max, dtype=torch.float32, device=dev)
    hip.call('brv_stoi_bands', spec, c['edges'], tob, 2*B, nf_max, ncols, c['bin0'], st)
    partial = torch.empty(B, max(nf_max - 29, 1), dtype=torch.float32, device=dev)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    hip.call('brv_stoi_correlate', tob[:B], tob[B:], geom, partial, out, B, nf_max, int(bool(extended)),
             10.0**(15.0/20.0), st)
    return out.double().cpu().numpy()


def _as_gpu(t):
    t = torch.as_tensor(t)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('stoi / estoi run as HIP kernels: a ROCm device is required '
                               '(there is no CPU fallback)')
        t = t.cuda()
    return t


def _stoi(x, y, fs, extended, batched, lengths):
    x, y = _as_gpu(x), _as_gpu(y)
    if x.shape != y.shape:
        raise ValueError(f'inputs must have same shape, got {x.shape} and {y.shape}')
    if x.ndim == 1:
        if lengths is not None and not batched:
            raise ValueError('Non-batched stoi does not support lengths '
                             'argument for 1D inputs.')
        return float(_stoi_hip(x[None], y[None], fs, extended,
                               None if lengths is None else torch.as_tensor(lengths).reshape(1))[0])
    if x.ndim != 2:
        raise ValueError(f'input must be 1 or 2 dimensional, got {x.ndim}')
    if batched:
        return _stoi_hip(x, y, fs, extended, lengths)
    if lengths is None:
        lengths = [x.shape[-1]]*x.shape[0]
    return np.array([_stoi_hip(xi[None, :n], yi[None, :n], fs, extended, None)[0]
                     for xi, yi, n in zip(x, y, [int(n) for n in lengths])])


@MetricRegistry.register('stoi')
def stoi(x, y, fs=16000, batched=True, lengths=None):
    return _stoi(x, y, fs, False, batched, lengths)


@MetricRegistry.register('estoi')
def estoi(x, y, fs=16000, batched=True, lengths=None):
    return _stoi(x, y, fs, True, batched, lengths)


@MetricRegistry.register('pesq')
def pesq(x, y, fs=16000, mode='wb', normalized=False, batched=True, lengths=None):
    """ITU-T P.862 through the third-party ``pesq`` wheel (reference metrics.py:48-95)."""
    try:
        from pesq import pesq as pesq_pesq
    except ImportError as e:
        raise ImportError(
            "the 'pesq' metric needs the third-party `pesq` package (ITU-T P.862 C code), "
            'which is not installed; remove pesq from val_metrics / --metrics or install it'
        ) from e
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)  # noqa: E731
    x, y = to_np(x), to_np(y)
    if x.ndim == 1:
        out = pesq_pesq(fs, y, x, mode=mode)
    else:
        if lengths is None:
            lengths = [x.shape[-1]]*x.shape[0]
        out = np.array([pesq_pesq(fs, yi[:int(n)], xi[:int(n)], mode=mode)
                        for xi, yi, n in zip(x, y, lengths)])
    if normalized:
        if mode not in ('nb', 'wb'):
            raise ValueError(f"mode must be 'nb' or 'wb', got '{mode}'")
        top = 4.548638319075995 if mode == 'nb' else 4.643888749336258
        out = (out - 1.0)/(top - 1.0)
    return out


def _check_input(x, y, lengths):
    """Add batch / source dims, default and validate ``lengths``
    (brever/metrics.py:126-150)."""
    if x.shape != y.shape:
        raise ValueError('inputs must have same shape, got '
                         f'{x.shape} and {y.shape}')
    unbatched = x.ndim == 1
    if unbatched:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    if x.ndim != 2:
        raise ValueError(f'input must be 1 or 2 dimensional, got {x.ndim}')
    x, y = x.unsqueeze(1), y.unsqueeze(1)
    if lengths is None:
        lengths = torch.full((x.shape[0],), x.shape[-1], device=x.device)
    else:
        if len(lengths) != x.shape[0]:
            raise ValueError('lengths must have same length as batch size, '
                             f'got {len(lengths)} and {x.shape[0]}')
        if bool((torch.as_tensor(lengths) > x.shape[-1]).any()):
            raise ValueError('lengths items must be smaller than input '
                             f'length, got lengths={lengths} and '
                             f'input.shape={x.shape}')
    return x, y, lengths, unbatched


def _negated(name):
    def metric(x, y, lengths=None):
        x, y, lengths, unbatched = _check_input(x, y, lengths)
        with torch.no_grad():
            value = -CriterionRegistry.get(name)(x, y, lengths)
        return value.item() if unbatched else value
    metric.__name__ = name
    return metric


snr = MetricRegistry.register('snr')(_negated('snr'))
sisnr = MetricRegistry.register('sisnr')(_negated('sisnr'))
