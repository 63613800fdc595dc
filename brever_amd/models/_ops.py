"""Host-side building blocks the HIP-path models share: the ``use_amp`` flag, the matrix-product dispatcher and the
thin wrappers (column matrices, row / column sums, element-wise helpers) around ``libbrever_hip.so``, plus the two
autograd nodes more than one model runs (``LinearFunction``, ``LSTMFunction``). Model files import from here, never
from one another's private names."""
import contextlib
import os

import torch
import torch.nn as nn

from .. import hip


class _ParamOnly(nn.Module):
    def forward(self, *args, **kwargs):
        raise RuntimeError('this module only stores parameters; the compute runs in '
                           'libbrever_hip.so')


# use_amp of the training / enhancement forward passes: bf16-operand matrix products, fp32 accumulation. ONE flag for
# every model; autograd nodes read it in ``forward`` and keep what they read for ``backward``.
AMP = {'on': False}


@contextlib.contextmanager
def amp(use_amp):
    AMP['on'] = bool(use_amp)
    try:
        yield
    finally:
        AMP['on'] = False


def empty(*shape, like):
    return torch.empty(*shape, dtype=torch.float32, device=like.device)


_SMALL_SCRATCH = {}
# NOTE: the two narrow-layer paths of ``gemm`` are taken BEFORE ``lowp`` is looked at, so under use_amp the
# layers with K, N <= 64 (and their weight gradients) run in full fp32 while every other product rounds its operands
# to bf16: closer to the fp32 oracle than the bf16 emulation assumes, never further (the use_amp tolerances of
# tests/test_gpu.py are upper bounds on the distance from the fp32 reference). The cut-over is a size rule of the
# library (`brv_linear_small_supported`), so results change at that size by bf16-rounding level, not more.


def gemm(a, b, d, batch, M, N, K, lda, ldb, ldd, a_bs=0, b_bs=0, d_bs=0, trans_a=0, trans_b=0,
         kbatch=1, a_kbs=0, b_kbs=0, bias=None, mode=0, lowp=False, small=False, workspace=True):
    """Batched d = op(a) @ op(b) (+ bias); ``mode`` 1 adds to d, 2 reads ``bias`` per output column. fp32 tensors:
    the exact-fp32 MFMA (``hip.gemm_f32``; ``workspace=False``: plain ``brv_gemm_f32``, never its workspace form) or,
    with ``lowp`` (``use_amp``), ``brv_gemm_bf16`` -- operands rounded to bf16 inside the kernel, fp32 accumulation.
    A bf16 ``a``, ``b`` or ``d`` tensor selects ``brv_gemm_bf16_mixed``. ``small``: narrow fp32 products go to
    ``brv_linear_small`` / ``brv_linear_small_wgrad`` where the library takes them (TF-GridNet only)."""
    half = torch.bfloat16
    flags = int(b.dtype == half) | int(d.dtype == half) << 1 | int(a.dtype == half) << 2
    if small and not flags and batch == 1 and kbatch == 1 and not trans_a and (bias is None or mode == 2) \
            and lda % 4 == 0 and ldd % 4 == 0 and (a.data_ptr() | d.data_ptr()) % 16 == 0 \
            and hip.lib().brv_linear_small_supported(M, N, K):
        # narrow layers (K, N <= 64 over ~2.6e5 rows): one thread per row in fp32 instead of a 128 x 128 MFMA tile
        hip.call('brv_linear_small', a, b, bias, d, M, N, K, lda, ldb, ldd, trans_b, int(mode == 1), hip.stream())
        return
    if small and not flags and batch == 1 and kbatch == 1 and trans_a and not trans_b and bias is None and mode == 0 \
            and lda % 4 == 0 and ldb % 4 == 0 and (a.data_ptr() | b.data_ptr()) % 16 == 0 \
            and hip.lib().brv_linear_small_wgrad_supported(K, M, N):
        # their weight gradients: (rows x M)^T (rows x N) over ~2.6e5 rows, slices added in a fixed order
        # (one scratch buffer per device and stream, not an allocation per call: up to 48 calls per step -- ADVICE r4;
        # the launches of a stream run in order, so consecutive products may share it)
        nbytes = hip.lib().brv_linear_small_wgrad_scratch_bytes(M, N)
        key = (d.device.index, torch.cuda.current_stream(d.device).cuda_stream)
        scratch = _SMALL_SCRATCH.get(key)
        if scratch is None or scratch.numel() < nbytes:
            scratch = _SMALL_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=d.device)
        hip.call('brv_linear_small_wgrad', a, b, d, scratch, K, M, N, lda, ldb, ldd, hip.stream())
        return
    args = (a, b, d, batch, M, N, K, lda, ldb, ldd, a_bs, b_bs, d_bs, trans_a, trans_b, kbatch, a_kbs, b_kbs, bias,
            mode)
    if flags:
        assert lowp       # (bf16 tensors exist under use_amp only)
        hip.call('brv_gemm_bf16_mixed', *args, flags, hip.stream())
    elif lowp:
        hip.call('brv_gemm_bf16', *args, hip.stream())
    elif workspace:
        hip.gemm_f32(*args)
    else:
        hip.call('brv_gemm_f32', *args, hip.stream())


def gemm_conv(a, img, d, batch, M, N, K, lda, ldd, a_bs, img_bs, d_bs, mode, image, geom, grid,
              trans_b=0, kbatch=1, a_kbs=0, img_kbs=0, bias=None):
    """``gemm(lowp=True)`` whose B operand is the column matrix of ``img`` -- never written out
    (``brv_gemm_bf16_conv``): ``image`` = (C, H, W) of ``img``, ``grid`` = the pixel grid of the
    columns; mode 1 = im2col, mode 2 = the gather form of col2im."""
    (kh, kw), (sh, sw), (ph, pw) = geom
    hip.call('brv_gemm_bf16_conv', a, img, d, batch, M, N, K, lda, ldd, a_bs, img_bs, d_bs, 0, trans_b, kbatch, a_kbs,
             img_kbs, bias, 0, mode, image[0], image[1], image[2], kh, kw, sh, sw, ph, pw, grid[0], grid[1],
             hip.stream())


def im2col(x, geom, grid, lowp=False):
    """x (B, C, H, W) -> (B, C*kh*kw, pixels of ``grid``); ``lowp``: the column matrix in bf16 (half the bytes of
    the largest tensor of the layer)."""
    (kh, kw), (sh, sw), (ph, pw) = geom
    B, C, H, W = x.shape
    col = torch.empty(B, C*kh*kw, grid[0]*grid[1], dtype=torch.bfloat16 if lowp else torch.float32,
                      device=x.device)
    hip.call('brv_im2col_bf16' if lowp else 'brv_im2col', x, col, B, C, H, W, kh, kw, sh, sw, ph, pw,
             grid[0], grid[1], hip.stream())
    return col


def col2im(col, bias, C, image, geom, grid):
    """The adjoint: columns over ``grid`` scattered onto (B, C, *image), plus a per-channel ``bias``."""
    (kh, kw), (sh, sw), (ph, pw) = geom
    B = col.shape[0]
    y = torch.empty(B, C, image[0], image[1], dtype=torch.float32, device=col.device)
    hip.call('brv_col2im_bf16' if col.dtype == torch.bfloat16 else 'brv_col2im', col, bias, y, B, C,
             image[0], image[1], kh, kw, sh, sw, ph, pw, grid[0], grid[1], hip.stream())
    return y


def row_sum(x, batch, rows, cols):
    """x (batch, rows, cols) -> (rows,): summed over the batch and the columns."""
    out = torch.empty(rows, dtype=torch.float32, device=x.device)
    hip.call('brv_row_sum', x, out, batch, rows, cols, hip.stream())
    return out


def column_sums(x, rows, cols, batch=1):
    """(batch, rows, cols) -> (batch, cols). fp32 tensors: ``brv_col_sum`` (fixed order, 16-byte loads: 17 us for
    258 516 x 32 -- also under ``use_amp``, where round 3 used a ones-vector product with split atomics); bf16
    tensors: ``brv_col_sum_bf16`` or, off its layout, a ones-vector product on the bf16 MFMA."""
    out = torch.empty(batch, cols, dtype=torch.float32, device=x.device)
    name = 'brv_col_sum' if x.dtype == torch.float32 else \
        'brv_col_sum_bf16' if x.dtype == torch.bfloat16 and cols % 8 == 0 and x.data_ptr() % 16 == 0 else None
    if name:
        scratch = torch.empty(hip.lib().brv_col_sum_scratch_bytes(batch, cols), dtype=torch.uint8, device=x.device)
        hip.call(name, x, out, scratch, batch, rows, cols, hip.stream())
        return out
    ones = torch.ones(rows, dtype=torch.float32, device=x.device)
    gemm(ones, x, out, batch, 1, cols, rows, rows, cols, cols, 0, rows*cols, cols, lowp=True)
    return out


def axpby_raw(a, alpha, b, beta):
    """alpha*a + beta*b (``b`` may be None), no autograd."""
    out = torch.empty_like(a)
    hip.call('brv_axpby', a, float(alpha), b, float(beta), out, a.numel(), hip.stream())
    return out


def combine(a, b, sign):
    """a + sign*b, no autograd."""
    out = torch.empty_like(a)
    hip.call('brv_combine', a, b, out, a.numel(), float(sign), hip.stream())
    return out


class LinearFunction(torch.autograd.Function):
    """y[b] (O, T) = W (O, I) @ x[b] (I, T) + bias[:, None]: nn.Linear on the feature axis of a (B, features, frames)
    tensor without the two transposes of the reference (ffnn.py:167-171; LSTMBlock.linear_r / linear_i,
    dccrn.py:293-311). ``lowp`` False: plain ``brv_gemm_f32``; True (``use_amp``): the three products on bf16-rounded
    operands, fp32 accumulation -- what torch.autocast makes of nn.Linear (oracle/dccrn.py: _LSTMBlock._linear)."""

    @staticmethod
    def forward(ctx, x, weight, bias, lowp):
        B, I, T = x.shape
        O = weight.shape[0]
        x = x.contiguous()
        y = torch.empty(B, O, T, dtype=torch.float32, device=x.device)
        gemm(weight, x, y, B, O, T, I, I, T, T, 0, I*T, O*T, bias=bias, lowp=lowp, workspace=False)
        ctx.save_for_backward(x, weight)
        ctx.lowp = lowp
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        B, I, T = x.shape
        O = weight.shape[0]
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)                       # W^T (I, O) @ dy[b] (O, T)
            gemm(weight, dy, dx, B, I, T, O, I, T, T, 0, O*T, I*T, trans_a=1, lowp=ctx.lowp, workspace=False)
        dw = torch.empty_like(weight)                      # sum_b dy[b] (O, T) @ x[b]^T (T, I)
        gemm(dy, x, dw, 1, O, I, T, T, T, I, trans_b=1, kbatch=B, a_kbs=O*T, b_kbs=I*T, lowp=ctx.lowp,
             workspace=False)
        return dx, dw, row_sum(dy, B, O, T), None


def lstm_interleave(w, H):
    """Rows gate*H + unit -> 4*unit + gate (the gate layout of brv_lstm_tile_*)."""
    G = w.shape[0]
    return w.view(G, 4, H, *w.shape[2:]).transpose(1, 2).reshape(w.shape).contiguous()


def lstm_deinterleave(w, H):
    G = w.shape[0]
    return w.view(G, H, 4, *w.shape[2:]).transpose(1, 2).reshape(w.shape).contiguous()


# BRV_LSTM_MV=0: the fp32 recurrence kernels under use_amp too (round 4)
_LSTM_MV = os.environ.get('BRV_LSTM_MV', '1') != '0'


class LSTMFunction(torch.autograd.Function):
    """G independent single-layer unidirectional nn.LSTMs (batch_first, zero initial state) in
    one set of launches: x (G, B, T, I) -> hidden states (G, B, T, H), parameters stacked on a
    leading group axis (w_ih (G, 4H, I), w_hh (G, 4H, H), b_ih / b_hh (G, 4H)). The input
    projections and their gradients are batched matrix products over G; the recurrence runs
    all G*B chains concurrently, one workgroup each."""

    TILE_MIN_CHAINS = 256       # below this the one-chain-per-workgroup kernels have more parallelism
    # use_amp: the tile kernels multiply on the bf16 MFMA (a step of 16 chains = 16 instructions per wave); DCCRN's 64
    # long chains then run as 4 workgroups
    TILE_MIN_CHAINS_LOWP = int(os.environ.get('BRV_LSTM_TILE_MIN_LOWP', '256'))

    _interleave = staticmethod(lstm_interleave)
    _deinterleave = staticmethod(lstm_deinterleave)

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh):
        lib = hip.lib()
        x, w_ih, w_hh = x.contiguous(), w_ih.contiguous(), w_hh.contiguous()
        G, B, T, I = x.shape
        # x of shape (1, B, T, I) with several weight sets: ONE input shared by all groups (batch stride 0 in the
        # products; its gradient is the sum over the groups) -- DCCRN's complex LSTM feeds [real; imag] to both modules
        shared = ctx.shared = G == 1 and w_hh.shape[0] > 1
        if shared:
            G = w_hh.shape[0]
        H = w_hh.shape[-1]
        lowp = ctx.lowp = AMP['on']
        # many short chains (TF-GridNet): 16 chains per workgroup on the exact-fp32 MFMA, gates
        # interleaved; few long chains (DCCRN): one workgroup per chain
        tiled = ctx.tiled = bool(lib.brv_lstm_tile_supported(H)) and \
            G*B >= (LSTMFunction.TILE_MIN_CHAINS_LOWP if lowp else LSTMFunction.TILE_MIN_CHAINS)
        if tiled:
            w_ih = lstm_interleave(w_ih, H)
        gates = torch.empty(G, B, T, 4*H, dtype=torch.float32, device=x.device)
        gemm(x, w_ih, gates, G, B*T, 4*H, I, I, I, 4*H, 0 if shared else B*T*I, 4*H*I, B*T*4*H, trans_b=1,
             lowp=lowp)
        bias = combine(b_ih.detach().contiguous(), b_hh.detach().contiguous(), 1.0)
        y = torch.empty(G, B, T, H, dtype=torch.float32, device=x.device)
        act = torch.empty(G, B, T, 4*H, dtype=torch.float32, device=x.device)
        cs = torch.empty(G, B, T, H, dtype=torch.float32, device=x.device)
        # use_amp, few long chains: the step's matrix-vector product on the bf16 MFMA (csrc/dccrn.hip lstm_*_mv_kernel)
        mv = ctx.mv = bool(lowp and not tiled and _LSTM_MV and lib.brv_lstm_recurrent_bf16_supported(H))
        name = 'brv_lstm_tile_forward' if tiled else \
            'brv_lstm_recurrent_forward_bf16' if mv else 'brv_lstm_recurrent_forward'
        extra = (0, H, B*T*H, int(lowp)) if tiled else ()   # no reversed group, (G, B, T, H) output
        hip.call(name, gates, w_hh, bias, y, act, cs, G*B, T, H, G, *extra, hip.stream())
        ctx.save_for_backward(x, w_ih, w_hh, y, act, cs)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_ih, w_hh, y, act, cs = ctx.saved_tensors          # w_ih interleaved when tiled
        G, B, T, I = x.shape
        shared = ctx.shared
        if shared:
            G = w_hh.shape[0]
        H = w_hh.shape[-1]
        lowp = ctx.lowp
        dy = dy.contiguous()
        dg = torch.empty(G, B, T, 4*H, dtype=torch.float32, device=x.device)
        name = 'brv_lstm_tile_backward' if ctx.tiled else \
            'brv_lstm_recurrent_backward_bf16' if ctx.mv else 'brv_lstm_recurrent_backward'
        extra = (0, H, B*T*H, int(lowp)) if ctx.tiled else ()
        hip.call(name, act, cs, w_hh, dy, dg, G*B, T, H, G, *extra, hip.stream())
        BT = B*T
        dx = torch.empty_like(x)                                   # dg (BT, 4H) @ W_ih (4H, I)
        if shared:                                                 # (summed over the groups: they are the k-batches)
            gemm(dg, w_ih, dx, 1, BT, I, 4*H, 4*H, I, I, kbatch=G, a_kbs=BT*4*H, b_kbs=4*H*I, lowp=lowp)
        else:
            gemm(dg, w_ih, dx, G, BT, I, 4*H, 4*H, I, I, BT*4*H, 4*H*I, BT*I, lowp=lowp)
        dw_ih = torch.empty_like(w_ih)                             # dg^T (4H, BT) @ x (BT, I)
        gemm(dg, x, dw_ih, G, 4*H, I, BT, 4*H, I, I, BT*4*H, 0 if shared else BT*I, 4*H*I, trans_a=1, lowp=lowp)
        # recurrent weight gradient: the gate gradients of frames 1.. against the hidden states of frames 0..T-2 of the
        # same chain, through shifted views (round 5: a zero-filled shifted copy of y was built per call -- a 16 MB fill
        # and a 16 MB copy in front of every product; the chains are the k-batches of the product instead)
        dw_hh = torch.zeros_like(w_hh) if T == 1 else torch.empty_like(w_hh)
        if T > 1:
            # (one launch: the groups are the batch, the chains of a group the k-batches)
            gemm(dg.view(-1)[4*H:], y, dw_hh, G, 4*H, H, T - 1, 4*H, H, H, B*T*4*H, B*T*H, 4*H*H, trans_a=1,
                 kbatch=B, a_kbs=T*4*H, b_kbs=T*H, lowp=lowp)
        # bias gradients: column sums of dg (BT, 4H) per group, in a fixed order (no transposed copy)
        db = column_sums(dg, BT, 4*H, batch=G)
        if ctx.tiled:
            dw_ih, dw_hh, db = (lstm_deinterleave(t, H) for t in (dw_ih, dw_hh, db))
        return dx, dw_ih, dw_hh, db, db.clone()
