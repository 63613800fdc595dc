"""The BSS-eval triple SDR / SIR / SAR on the HIP path: every estimate projected on each reference alone and on the
span of all references, each through an allowed distortion filter of ``filter_length`` taps.

It runs in ``libbrever_sdr.so`` through its second header (include/sdr/brever_bsseval.h; csrc/sdr/bsseval.cuh): the
lag and Levinson kernels of ``sdr.py`` give the single-reference projections, so ``sdr_table[b, e, j]`` has the bits
of ``sdr.forward`` on the row ``(x_e, s_j)``, and one workgroup per item runs the block Levinson recursion for the
joint projection. The metrics ``sir`` and ``sar`` of ``metrics.py`` call it with ``references = (target, noise ...)``.

Everything is fp64 from fp32 signals, every reduction has a fixed order, so the values are bitwise repeatable and an
item gives the same bits alone as in a batch. ``lengths`` stays on the device; nothing here synchronises. There is no
CPU fallback and no gradient: SIR and SAR are metrics, not criteria.
"""
from collections import namedtuple

import torch

from . import hip
from . import sdr as sdr_hip

# the brv_bss_* entry points of include/sdr/brever_bsseval.h, on the library of sdr.py
_LIB = hip.Library('sdr/brever_bsseval.h', 'libbrever_sdr.so', 'BRV_SDR_LIB_PATH',
                   'The sir and sar metrics have no CPU fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, query, last_error = _LIB.lib, _LIB.call, _LIB.query, _LIB.last_error
MIN_REFERENCES, MAX_REFERENCES = _LIB.constants['BRV_BSS_MIN_REFERENCES'], _LIB.constants['BRV_BSS_MAX_REFERENCES']
# bits of BssEval.item_flags (NO_REFERENCE, BAD_PIVOT) and BssEval.estimate_flags (the others)
(NO_REFERENCE, BAD_PIVOT, NO_ESTIMATE, SAR_NUMERATOR_FLOOR, SAR_DENOMINATOR_FLOOR, SIR_NUMERATOR_FLOOR,
 SIR_DENOMINATOR_FLOOR) = (_LIB.constants['BRV_BSS_FLAG_' + name] for name in (
     'NO_REFERENCE', 'BAD_PIVOT', 'NO_ESTIMATE', 'SAR_NUMERATOR_FLOOR', 'SAR_DENOMINATOR_FLOOR',
     'SIR_NUMERATOR_FLOOR', 'SIR_DENOMINATOR_FLOOR'))

BssEval = namedtuple('BssEval', 'sdr sir sar perm sdr_table sir_table item_flags estimate_flags')


def bss_eval(estimates, references, lengths=None, filter_length=512, load_diag=0.0, permute=True):
    """``estimates``: ``(B, S, W)``, ``references``: ``(B, J, W)`` on the GPU, ``2 <= J <= 4``, ``1 <= S <= J``; the
    targets are the first ``S`` references, further references are interferers only. ``lengths``: ``(B,)`` or None.

    Returns a ``BssEval`` of device tensors: ``sdr``, ``sir``, ``sar`` ``(B, S)`` fp64 in dB under the assignment
    ``perm`` ``(B, S)`` int64 of estimates to references (the one with the largest summed SIR, or the identity with
    ``permute=False``), the full ``sdr_table`` and ``sir_table`` ``(B, S, J)``, and the flag words ``item_flags``
    ``(B,)`` / ``estimate_flags`` ``(B, S)`` int32. NaN marks a degenerate item (a silent reference, a pivot of the
    block recursion that is not positive) or estimate (zero inside the length)."""
    filter_length, load_diag = sdr_hip.check_options(filter_length, load_diag)
    estimates, references = torch.as_tensor(estimates), torch.as_tensor(references)
    if estimates.ndim != 3 or references.ndim != 3:
        raise ValueError('estimates and references must be (batch, sources, samples), got '
                         f'{tuple(estimates.shape)} and {tuple(references.shape)}')
    (B, S, W), (Br, J, Wr) = estimates.shape, references.shape
    if (B, W) != (Br, Wr):
        raise ValueError('estimates and references must agree in batch size and length, got '
                         f'{tuple(estimates.shape)} and {tuple(references.shape)}')
    if not MIN_REFERENCES <= J <= MAX_REFERENCES or not 1 <= S <= J:
        raise ValueError(f'needs {MIN_REFERENCES} to {MAX_REFERENCES} references and 1 to that many estimates, got '
                         f'{J} references and {S} estimates')
    hip.require_device(estimates, references)
    dev = estimates.device
    if lengths is None:
        lengths = torch.full((B,), W, dtype=torch.int64, device=dev)
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f'lengths must have one entry per batch item, got {tuple(lengths.shape)} for {B} items')
    x = estimates.detach().float().contiguous()
    s = references.detach().float().contiguous()
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    ws = torch.empty(query('brv_bss_workspace_bytes', B, S, J, W, filter_length)//8, **f64)
    out = BssEval(torch.empty(B, S, **f64), torch.empty(B, S, **f64), torch.empty(B, S, **f64),
                  torch.empty(B, S, dtype=torch.int64, device=dev), torch.empty(B, S, J, **f64),
                  torch.empty(B, S, J, **f64), torch.empty(B, **i32), torch.empty(B, S, **i32))
    call('brv_bss_eval', x, s, lengths, B, S, J, W, filter_length, load_diag, int(bool(permute)), ws, out.sdr,
         out.sir, out.sar, out.perm, out.sdr_table, out.sir_table, out.item_flags, out.estimate_flags, hip.stream())
    return out
