"""Evaluation metrics (reference brever/metrics.py:16-150): the same registry keys and call
signatures -- ``metric(x, y, ..., lengths=None)`` with ``x`` the processed signal and ``y`` the
clean target, batched ``(B, L)`` or single ``(L,)``.

* ``snr`` / ``sisnr``: minus the HIP criteria;
* ``sdr`` (not in the reference): the BSS-eval signal-to-distortion ratio with a 512-tap allowed distortion filter,
  in fp64 on the HIP path (``sdr.py``, ``csrc/sdr/sdr.hip``); the call shape of ``snr`` plus ``filter_length`` and
  ``load_diag``;
* ``sir`` / ``sar`` (not in the reference): the other two of the BSS-eval triple, the signal-to-interference and the
  signal-to-artifacts ratio (``bsseval.py``, ``csrc/sdr/bsseval.cuh``). They need a second reference, ``noise``: for
  a mixture ``foreground + background`` it is ``mixture - target``, which ``score`` below passes. The *input* column
  of ``sar`` sits at or near its floor of ``10 log10(2^52)`` dB by construction: the mixture lies in the span of its
  own two components;
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
import inspect

import numpy as np
import torch

from . import bsseval as bss_hip
from . import hip
from . import sdr as sdr_hip
from . import stoi as stoi_hip
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
def _stoi_hip(x, y, fs, extended, lengths):
    """x: processed, y: clean, (B, L) float tensors on the GPU; lengths: (B,) or None. The launches are those of
    the ``stoi`` / ``estoi`` criteria (``stoi.forward``)."""
    x = x.detach().float().contiguous()
    y = y.detach().float().contiguous()
    hip.require_device(x, y)
    B, L = x.shape
    dev = x.device
    if lengths is None:
        lengths = torch.full((B,), L, dtype=torch.int64, device=dev)
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).contiguous()
    out, _ = stoi_hip.forward(x, y, fs, extended, lengths)
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


@MetricRegistry.register('sdr')
def sdr(x, y, lengths=None, filter_length=512, load_diag=0.0):
    """BSS-eval signal-to-distortion ratio in dB with an allowed distortion filter of ``filter_length`` taps
    (``sdr.forward``): a ``(B,)`` fp64 tensor on the inputs' device, or a float for a single row. NaN for a
    degenerate row (a target or an estimate that is zero inside the length, a solver pivot that is not
    positive)."""
    filter_length, load_diag = sdr_hip.check_options(filter_length, load_diag)
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    hip.require_device(x, y)
    x, y, lengths, unbatched = _check_input(x, y, lengths)
    B, W = x.shape[0], x.shape[-1]
    lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int64).contiguous()
    value, _ = sdr_hip.forward(x.detach().reshape(B, W).float().contiguous(),
                               y.detach().reshape(B, W).float().contiguous(), lengths, filter_length, load_diag)
    return value.item() if unbatched else value


def _bss(which, x, y, lengths, noise, filter_length, load_diag):
    """``sir`` / ``sar`` of the estimate ``x`` against the references ``(y, noise ...)`` (``bsseval.bss_eval`` with
    one estimate, whose target is ``y``)."""
    filter_length, load_diag = sdr_hip.check_options(filter_length, load_diag)
    if noise is None:
        raise ValueError(f"the '{which}' metric needs a second reference: pass noise= (for a mixture of a target "
                         f'and a background, mixture - target; metrics.score does that), one (B, L) signal or up to '
                         f'{bss_hip.MAX_REFERENCES - 1} as (B, K, L)')
    x, y, noise = torch.as_tensor(x), torch.as_tensor(y), torch.as_tensor(noise)
    hip.require_device(x, y, noise)
    x, y, lengths, unbatched = _check_input(x, y, lengths)
    B, W = x.shape[0], x.shape[-1]
    if unbatched and noise.ndim == 1:
        noise = noise[None]
    if noise.ndim == 2:
        noise = noise[:, None]
    if noise.ndim != 3 or (noise.shape[0], noise.shape[-1]) != (B, W) or \
            not 1 <= noise.shape[1] <= bss_hip.MAX_REFERENCES - 1:
        raise ValueError(f'noise must be (B, L) or (B, K, L) with K <= {bss_hip.MAX_REFERENCES - 1} and match the '
                         f'inputs {tuple(x.shape)}, got {tuple(noise.shape)}')
    out = bss_hip.bss_eval(x.reshape(B, 1, W), torch.cat([y.reshape(B, 1, W).to(noise.dtype), noise], dim=1), lengths,
                           filter_length, load_diag, permute=False)
    value = getattr(out, which)[:, 0]
    return value.item() if unbatched else value


@MetricRegistry.register('sir')
def sir(x, y, lengths=None, noise=None, filter_length=512, load_diag=0.0):
    """BSS-eval signal-to-interference ratio in dB: of the part of ``x`` that lies in the span of the references
    ``(y, noise)``, each through ``filter_length`` taps, how much is ``y``'s. ``noise``: the other references,
    ``(B, L)`` or ``(B, K, L)`` with ``K <= 3`` (``(L,)`` for a single row). A ``(B,)`` fp64 tensor on the inputs'
    device, or a float for a single row; NaN for a degenerate one."""
    return _bss('sir', x, y, lengths, noise, filter_length, load_diag)


@MetricRegistry.register('sar')
def sar(x, y, lengths=None, noise=None, filter_length=512, load_diag=0.0):
    """BSS-eval signal-to-artifacts ratio in dB: the part of ``x`` in the span of the references ``(y, noise)``
    against the part outside it. Arguments and result as ``sir``. Scoring a mixture against its own components gives
    the floor, ``10 log10(2^52)`` dB or close to it."""
    return _bss('sar', x, y, lengths, noise, filter_length, load_diag)


def takes_noise(name):
    """True for a registered metric whose signature has a ``noise`` parameter (``sir``, ``sar``)."""
    return 'noise' in inspect.signature(MetricRegistry.get(name)).parameters


def score(name, x, target, lengths, mixture=None):
    """The registered metric ``name`` of ``x`` against ``target``. A metric whose signature has a ``noise`` parameter
    (``sir``, ``sar``) gets ``noise = mixture - target``, the second component of a mixture
    ``foreground + background``; every other metric is called as ``metric(x, target, lengths=lengths)``."""
    fn = MetricRegistry.get(name)
    if not takes_noise(name):
        return fn(x, target, lengths=lengths)
    if mixture is None:
        raise ValueError(f"the '{name}' metric needs the mixture: its second reference is mixture - target")
    return fn(x, target, lengths=lengths, noise=torch.as_tensor(mixture) - torch.as_tensor(target))
