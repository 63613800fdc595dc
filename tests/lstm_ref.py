"""A float64 restatement of what the LSTM recurrence entry points of include/brever_hip.h define (brv_lstm_recurrent_*,
brv_lstm_recurrent_*_bf16, brv_lstm_tile_*): the reference of tests/test_gpu_lstm.py, itself held to torch.nn.LSTM by
tests/test_lstm_ref_host.py. Plain torch on the CPU; nothing of brever_amd is imported.

Layouts. The chains are ``groups`` consecutive sets of B/groups chains, each set with its own ``w_hh[g]`` (4H, H) and
``bias[g]`` (4H). Every tensor here has torch's gate order on its last axis (row gate*H + unit, gates i, f, g, o);
``interleave`` / ``deinterleave`` convert to and from the order of brv_lstm_tile_* (column 4*unit + gate). Bit g of
``reverse_mask`` makes group g walk the frames backwards: recurrence step t is then frame T-1-t. ``gates_in``, ``y``,
``dy`` and ``dgates`` are indexed by FRAME, the saved ``act`` / ``cs`` by recurrence STEP -- exactly what
csrc/lstm_tile.hip does.

Rounding. ``round_operands`` rounds to bf16 (nearest even) only what the bf16 kernels round: h and W_hh in the
recurrent product, the gate gradients and W_hh in its adjoint. ``io16`` is the storage format of lowp == 2: the saved
activations and the gate gradients are bf16 tensors (the unrounded values still drive the recurrence that produced
them; the rounded gate gradients feed the adjoint product, as in the kernels, which round once for both uses).

``dtype`` / ``fast`` restate the same arithmetic in float32 with the kernels' own forms of the gate non-linearities
(1/(1 + exp(-x)), 2/(1 + exp(-2x)) - 1): the distance of that restatement from the float64 one is the yardstick for
what float32 arithmetic alone may cost (never the kernels' own output)."""
import torch

F64 = torch.float64


def round_bf16(t):
    """The value a kernel sees after rounding to bf16 (nearest even: common.cuh f2bf / pack2), in t's own dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()/(b.norm() + 1e-30))


def interleave(x):
    """Last axis gate*H + unit -> 4*unit + gate."""
    H = x.shape[-1]//4
    return x.reshape(*x.shape[:-1], 4, H).transpose(-1, -2).reshape(x.shape).contiguous()


def deinterleave(x):
    """Last axis 4*unit + gate -> gate*H + unit."""
    H = x.shape[-1]//4
    return x.reshape(*x.shape[:-1], H, 4).transpose(-1, -2).reshape(x.shape).contiguous()


def y_index(B, T, H, groups, ld, group_offset):
    """(B, T, H) int64: where element (chain, frame, unit) of y / dy lives in the flat buffer,
    g*group_offset + (c*T + t)*ld + u with chain = g*(B/groups) + c."""
    per = B//groups
    chain = torch.arange(B)
    g, c = chain//per, chain % per
    return ((g*group_offset)[:, None, None] + ((c*T)[:, None, None] + torch.arange(T)[None, :, None])*ld
            + torch.arange(H)[None, None, :])


def place_y(y, groups, ld, group_offset, fill=0.0):
    """y (B, T, H) -> the flat buffer of that layout (``fill`` wherever no element lives)."""
    B, T, H = y.shape
    idx = y_index(B, T, H, groups, ld, group_offset)
    buf = torch.full((int(idx.max()) + 1,), fill, dtype=y.dtype)
    buf[idx.reshape(-1)] = y.reshape(-1)
    return buf


def _sigmoid(x, fast):
    return 1.0/(1.0 + torch.exp(-x)) if fast else torch.sigmoid(x)


def _tanh(x, fast):
    return 2.0/(1.0 + torch.exp(-2.0*x)) - 1.0 if fast else torch.tanh(x)


def _frames(T, reverse):
    return list(range(T - 1, -1, -1)) if reverse else list(range(T))


def forward(gates_in, w_hh, bias, groups=1, reverse_mask=0, round_operands=False, io16=False, dtype=F64, fast=False):
    """gates_in (B, T, 4H) by frame, w_hh (groups, 4H, H), bias (groups, 4H) or None -> y (B, T, H) by frame,
    act (B, T, 4H) and cs (B, T, H) by recurrence step. Zero initial state. ``io16``: act comes back rounded to bf16
    (the caller makes gates_in bf16-representable)."""
    gates_in, w_hh = gates_in.to(dtype), w_hh.to(dtype)
    B, T, H4 = gates_in.shape
    H = H4//4
    assert B % groups == 0 and w_hh.shape == (groups, H4, H)
    per = B//groups
    y = torch.zeros(B, T, H, dtype=dtype)
    act = torch.zeros(B, T, H4, dtype=dtype)
    cs = torch.zeros(B, T, H, dtype=dtype)
    for g in range(groups):
        sl = slice(g*per, (g + 1)*per)
        w = round_bf16(w_hh[g]) if round_operands else w_hh[g]
        b = bias[g].to(dtype) if bias is not None else torch.zeros(H4, dtype=dtype)
        h = torch.zeros(per, H, dtype=dtype)
        c = torch.zeros(per, H, dtype=dtype)
        for t, frame in enumerate(_frames(T, (reverse_mask >> g) & 1)):
            hq = round_bf16(h) if round_operands else h
            pre = gates_in[sl, frame] + b + hq @ w.t()
            i, f, gg, o = pre.chunk(4, dim=-1)
            i, f, gg, o = _sigmoid(i, fast), _sigmoid(f, fast), _tanh(gg, fast), _sigmoid(o, fast)
            c = f*c + i*gg
            h = o*_tanh(c, fast)
            y[sl, frame] = h
            cs[sl, t] = c
            act[sl, t] = torch.cat([i, f, gg, o], dim=-1)
    return y, (round_bf16(act) if io16 else act), cs


def backward(act, cs, w_hh, dy, groups=1, reverse_mask=0, round_operands=False, io16=False, dtype=F64, fast=False):
    """act (B, T, 4H), cs (B, T, H) by recurrence step, dy (B, T, H) by frame -> the gradient with respect to the gate
    pre-activations, dgates (B, T, 4H) by frame. ``io16``: returns (dgates, dgates rounded to bf16) and feeds the
    rounded copy to the adjoint product."""
    act, cs, w_hh, dy = act.to(dtype), cs.to(dtype), w_hh.to(dtype), dy.to(dtype)
    B, T, H4 = act.shape
    H = H4//4
    assert B % groups == 0 and w_hh.shape == (groups, H4, H)
    per = B//groups
    dgates = torch.zeros(B, T, H4, dtype=dtype)
    for g in range(groups):
        sl = slice(g*per, (g + 1)*per)
        w = round_bf16(w_hh[g]) if round_operands else w_hh[g]
        frames = _frames(T, (reverse_mask >> g) & 1)
        dh = torch.zeros(per, H, dtype=dtype)
        dc = torch.zeros(per, H, dtype=dtype)
        for t in range(T - 1, -1, -1):
            i, f, gg, o = act[sl, t].chunk(4, dim=-1)
            c = cs[sl, t]
            cp = cs[sl, t - 1] if t > 0 else torch.zeros(per, H, dtype=dtype)
            tc = _tanh(c, fast)
            dht = dh + dy[sl, frames[t]]
            dct = dc + dht*o*(1 - tc*tc)
            d = torch.cat([dct*gg*i*(1 - i), dct*cp*f*(1 - f), dct*i*(1 - gg*gg), dht*tc*o*(1 - o)], dim=-1)
            dgates[sl, frames[t]] = d
            dc = dct*f
            dh = (round_bf16(d) if round_operands or io16 else d) @ w
    return (dgates, round_bf16(dgates)) if io16 else dgates
