"""BSS-eval signal-to-distortion ratio on the HIP path: the forward that the metric (``metrics.py``: ``sdr``) and the
training criterion (``criterion.py``: ``SdrLoss``) share, and the criterion's backward.

Both run in ``libbrever_sdr.so`` (include/brever_sdr.h; csrc/sdr/sdr.hip). Per row the ``filter_length`` correlation
lags of the reference with itself and with the estimate are accumulated in fp64, the symmetric Toeplitz system for the
allowed distortion filter ``h`` is solved by the Levinson recursion, and ``SDR = 10 log10(q / (E - q))`` with
``q = b^T h`` and ``E`` the estimate's energy. The backward is one FIR pass of the reference through
``h`` fused with the closed-form gradient.

Only the estimate gets a gradient. Every reduction has a fixed order, so values and gradients are bitwise repeatable
and a row gives the same bits alone as in a batch. ``lengths`` stays on the device; nothing here synchronises. There
is no CPU fallback: without the library or a ROCm device the calls raise.
"""
import torch

from . import hip

# the brv_sdr_* entry points of include/brever_sdr.h
_LIB = hip.Library('brever_sdr.h', 'libbrever_sdr.so', 'BRV_SDR_LIB_PATH',
                   'The sdr metric and criterion have no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, last_error = _LIB.lib, _LIB.call, _LIB.last_error
MAX_FILTER_LENGTH = _LIB.constants['BRV_SDR_MAX_FILTER_LENGTH']
# bits of the per-row flags word
NO_REFERENCE, NO_ESTIMATE, BAD_PIVOT, NUMERATOR_FLOOR, DENOMINATOR_FLOOR = (
    _LIB.constants['BRV_SDR_FLAG_' + name] for name in (
        'NO_REFERENCE', 'NO_ESTIMATE', 'BAD_PIVOT', 'NUMERATOR_FLOOR', 'DENOMINATOR_FLOOR'))
DEGENERATE = NO_REFERENCE | NO_ESTIMATE | BAD_PIVOT


def check_options(filter_length, load_diag):
    """``(filter_length, load_diag)`` as ``(int, float)``; ``ValueError`` for what the kernels do not take. The
    loading reaches the library as a C float: ``R`` carries ``float32(load_diag) r[0]`` on its diagonal."""
    if isinstance(filter_length, bool) or int(filter_length) != filter_length or \
            not 1 <= filter_length <= MAX_FILTER_LENGTH:
        raise ValueError(f'filter_length must be an integer in [1, {MAX_FILTER_LENGTH}], got {filter_length}')
    if not float(load_diag) >= 0.0:
        raise ValueError(f'load_diag must be non-negative, got {load_diag}')
    return int(filter_length), float(load_diag)


def forward(x, y, lengths, filter_length=512, load_diag=0.0):
    """``x``: estimate, ``y``: reference, ``(R, W)`` contiguous fp32 on the GPU; ``lengths``: ``(R,)`` int64 on the
    GPU. Returns ``(sdr, saved)``: the ``(R,)`` fp64 SDR in dB of every row (NaN for a degenerate one) and what the
    backward needs."""
    filter_length, load_diag = check_options(filter_length, load_diag)
    hip.require_device(x, y, lengths)
    R, W = x.shape
    dev = x.device
    nbytes = lib().brv_sdr_workspace_bytes(R, W, filter_length)
    if nbytes < 0:
        raise RuntimeError(f'brv_sdr_workspace_bytes: {last_error()}')
    f64 = dict(dtype=torch.float64, device=dev)
    ws = torch.empty(nbytes//8, **f64)
    value, q, e = torch.empty(R, **f64), torch.empty(R, **f64), torch.empty(R, **f64)
    h = torch.empty(R, filter_length, **f64)
    flags = torch.empty(R, dtype=torch.int32, device=dev)
    call('brv_sdr_forward', x, y, lengths, R, W, filter_length, load_diag, ws, value, h, q, e, flags, hip.stream())
    return value, dict(x=x, y=y, lengths=lengths, h=h, q=q, e=e, flags=flags, filter_length=filter_length)


def backward(saved, grad_rows):
    """Gradient ``(R, W)`` fp32 of ``sum(grad_rows * -sdr)`` with respect to the estimate, from what ``forward``
    saved; ``grad_rows``: ``(R,)`` contiguous fp64. Zero at and beyond every row's length and on degenerate rows."""
    x = saved['x']
    R, W = x.shape
    dx = torch.empty_like(x)
    call('brv_sdr_backward', x, saved['y'], saved['lengths'], saved['h'], saved['q'], saved['e'], saved['flags'],
         grad_rows, R, W, saved['filter_length'], dx, hip.stream())
    return dx
