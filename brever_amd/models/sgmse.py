"""SGMSE+ (score-based generative speech enhancement) on the HIP path -- inference.

Same constructor signature, registry keys (``sgmsep``, ``sgmsepm``), module tree / state-dict
names and seeded initialisation as the reference (brever/models/sgmse/sgmse.py:23-213,
net.py:12-477, preconditioning.py:5-58, sdes.py:11-81, solvers.py:8-77). ``enhance`` runs the
reverse SDE (predictor-corrector or EDM/Heun sampler) with every network evaluation -- 3x3 /
1x1 convolutions, group norms, SiLU, FIR resampling, self-attention, noise embedding -- and
every state update in ``libbrever_hip.so`` (``enhance(x, use_amp=True)`` puts the convolutions
on the fp16 MFMA with folded group norms, ``hip_autocast``); torch draws the Gaussian noise, concatenates skip
tensors and holds the parameters.

Built: every SDE, both solvers (``pc``, ``edm``), all three preconditionings and every
encoder / decoder / block type of ``DiffusionUNet``; training (``loss``) runs the differentiable
network of ``sgmse_train.py``.
"""
import math
import os

import torch
import torch.nn as nn

from .. import hip
from ..modules.resampling import Resample
from ..modules.stft import STFT
from ..registry import Registry
from ._ops import amp
from .base import BreverBaseModel, ModelRegistry

SDERegistry = Registry('sde')
SolverRegistry = Registry('solver')


# ------------------------------------------------------------------------------------------
# HIP primitives (inference: plain functions on contiguous fp32 tensors)
# ------------------------------------------------------------------------------------------
_STATE = {'amp': False, 'graph': False, 'pver': None}
_GN_SCRATCH = {}
# Parameters of these models are also written through raw pointers (FlatAdam's fused clip + Adam launch) and through
# ``param.data`` (EMA), neither of which moves ``Tensor._version``: every derived copy of a weight (packed fp16
# convolution weights, the stacked q / k / v and embedding matrices, captured HIP graphs) is keyed on this counter
# too. ``SGMSEp.mark_params_changed`` -- called by FlatAdam.step, EMA and the trainer's checkpoint loads -- bumps it.
_PARAM_EPOCH = [0]
_CONV_SPLIT = os.environ.get('BRV_CONV_SPLIT', '1') != '0'


class hip_autocast:
    """``use_amp`` of the HIP path: inside the block the 1x1 / 3x3 convolutions run on the fp16
    MFMA with fp32 accumulation and the group norms feeding them are folded into their load
    path (the reference autocasts to fp16, sgmse.py:190-193). Networks with 'standard' / 'skip'
    encoders and decoders keep channels-last fp16 activations between the layers
    (``brv_conv_nhwc_forward`` and the ``brv_nhwc_*`` kernels, ``DiffusionUNet._forward_nhwc``);
    the others fp32 NCHW activations (``brv_conv2d_mfma_forward``). Outside the block every
    kernel is fp32."""

    def __init__(self, enabled):
        self.enabled = bool(enabled)

    def __enter__(self):
        self.prev = _STATE['amp']
        _STATE['amp'] = self.enabled

    def __exit__(self, *exc):
        _STATE['amp'] = self.prev


def _packed_weight(mod):
    w = mod.weight
    key = (w.data_ptr(), w._version, _PARAM_EPOCH[0])
    if getattr(mod, '_brv_wp_key', None) != key:
        Cout, Cin, k, _ = w.shape
        n = hip.lib().brv_conv2d_packed_size(Cout, Cin, k)
        wp = torch.empty(n, dtype=torch.float16, device=w.device)
        hip.call('brv_conv2d_pack_f16', w.detach().contiguous(), wp, Cout, Cin, k, hip.stream())
        mod._brv_wp, mod._brv_wp_key = wp, key
    return mod._brv_wp


def _conv(x, mod, fold=None, silu=False, res=None, out_scale=1.0):
    """out_scale*(conv(act(fold(x))) + bias + res); ``fold`` = (scale, shift) per (item, channel)
    from ``_gn_fold`` (a GroupNorm reduced to an affine map), applied on the load path of the
    MFMA kernel under ``hip_autocast`` and by ``brv_affine_act`` otherwise."""
    x = x.contiguous()
    B, Cin, H, W = x.shape
    Cout = mod.out_channels
    (kh, kw), (sh, sw), (ph, pw) = mod.kernel_size, mod.stride, mod.padding
    # (the MFMA kernel addresses its input with 32-bit byte offsets: very long spectrograms take
    # the fp32 matrix-product path below instead)
    fits = (-(-Cin//32)*32 + 1)*H*W*4 < (1 << 32)
    if _STATE['amp'] and fits and kh == kw and kh in (1, 3) and (sh, sw) == (1, 1) \
            and ph == pw == kh//2:
        y = torch.empty(B, Cout, H, W, dtype=torch.float32, device=x.device)
        sc, sf = fold if fold is not None else (None, None)
        hip.call('brv_conv2d_mfma_forward', x, _packed_weight(mod), mod.bias,
                 res.contiguous() if res is not None else None, sc, sf, int(silu), y, B, Cin, H, W, Cout, kh, Cin*H*W,
                 Cout*H*W, float(out_scale), hip.stream())
        return y
    if fold is not None:
        x = _affine_act(x, fold, silu)
    Ho, Wo = (H + 2*ph - kh)//sh + 1, (W + 2*pw - kw)//sw + 1
    y = torch.empty(B, Cout, Ho, Wo, dtype=torch.float32, device=x.device)
    K = Cin*kh*kw
    if Cout >= 16 and K >= 16:
        # fp32 path: column matrix + one exact-fp32 MFMA product per item (a 1x1 convolution
        # is the product on the image itself)
        if (kh, kw, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0):
            col = x
        else:
            col = torch.empty(B, K, Ho*Wo, dtype=torch.float32, device=x.device)
            hip.call('brv_im2col', x, col, B, Cin, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo, hip.stream())
        hip.call('brv_gemm_f32', mod.weight, col, y, B, Cout, Ho*Wo, K, K, Ho*Wo, Ho*Wo, 0, K*Ho*Wo, Cout*Ho*Wo, 0, 0,
                 1, 0, 0, mod.bias, 0, hip.stream())
    else:
        hip.call('brv_conv2d_forward', x, mod.weight, mod.bias, y, B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, Cin*H*W,
                 Cout*Ho*Wo, 0, 1.0, hip.stream())
    if res is not None or out_scale != 1.0:
        y = _axpby(y, out_scale, res, out_scale)
    return y


def _gn_fold(x, mod, add=None, adm=None):
    """GroupNorm(x + add[:, :, None, None]) [then (1 + adm[0])*. + adm[1]] as a per-(item,
    channel) affine map of x: returns (scale, shift), each (B, C)."""
    x = x.contiguous()
    B, C, H, W = x.shape
    lib = hip.lib()
    need = lib.brv_groupnorm_scratch_bytes(B, mod.num_groups)
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    scratch = _GN_SCRATCH.get(key)
    if scratch is None or scratch.numel() < need:        # zero once; the kernels leave it zero
        scratch = _GN_SCRATCH[key] = torch.zeros(max(need, 1 << 16), dtype=torch.uint8,
                                                 device=x.device)
    scale = torch.empty(B, C, dtype=torch.float32, device=x.device)
    shift = torch.empty_like(scale)
    a0, a1 = (adm[0].contiguous(), adm[1].contiguous()) if adm is not None else (None, None)
    hip.call('brv_groupnorm_fold', x, add.contiguous() if add is not None else None, mod.weight, mod.bias, a0, a1,
             scratch, scale, shift, None, None, B, C, H*W, mod.num_groups, float(mod.eps), hip.stream())
    return scale, shift


def _affine_act(x, fold, silu=False):
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    hip.call('brv_affine_act', x, fold[0], fold[1], y, B, C, H*W, int(silu), hip.stream())
    return y


def _group_norm(x, mod, add=None, silu=False):
    return _affine_act(x, _gn_fold(x, mod, add), silu)


def _silu(x):
    x = x.contiguous()
    y = torch.empty_like(x)
    hip.call('brv_silu', x, y, x.numel(), hip.stream())
    return y


def _linear(x, mod):
    """(N, in) -> (N, out): W (out, in) @ x^T (+ bias per row), returned transposed back."""
    x = x.contiguous()
    N, K = x.shape
    O = mod.out_features
    d = torch.empty(O, N, dtype=torch.float32, device=x.device)
    hip.call('brv_gemm_f32', mod.weight, x, d, 1, O, N, K, K, K, N, 0, 0, 0, 0, 1, 1, 0, 0, mod.bias, 0, hip.stream())
    return d.t().contiguous()


def _axpby(a, alpha, b=None, beta=0.0):
    a = a.contiguous()
    out = torch.empty_like(a)
    ar = torch.view_as_real(a) if a.is_complex() else a
    orr = torch.view_as_real(out) if a.is_complex() else out
    br = None
    if b is not None:
        b = b.contiguous()
        if a.is_complex() and not b.is_complex():
            b = torch.complex(b, torch.zeros_like(b))        # real noise added to a complex state
        br = torch.view_as_real(b) if b.is_complex() else b
    hip.call('brv_axpby', ar, float(alpha), br, float(beta), orr, ar.numel(), hip.stream())
    return out


# ------------------------------------------------------------------------------------------
# use_amp, second form: channels-last fp16 activations between the layers (the tensors the
# reference's fp16 autocast holds there too). ``_Act`` = (B, H, W, Cs) fp16 with C valid channels
# (Cs = C rounded up to 8, the rest zeros), optionally followed by a second one along the
# channels (a U-Net skip connection: never copied together, the consumers read both).
# ------------------------------------------------------------------------------------------
class _Act:
    __slots__ = ('t', 'C', 'second', 'sums')

    def __init__(self, t, C, second=None):
        self.t, self.C, self.second, self.sums = t, C, second, None

    @property
    def Cs(self):
        return self.t.shape[3]

    @property
    def channels(self):
        return self.C + (self.second.C if self.second is not None else 0)

    @property
    def hw(self):
        return self.t.shape[1], self.t.shape[2]


def _h_new(B, H, W, C, device):
    return _Act(torch.empty(B, H, W, -(-C//8)*8, dtype=torch.float16, device=device), C)


def _h_from_nchw(x):
    x = x.contiguous()
    B, C, H, W = x.shape
    a = _h_new(B, H, W, C, x.device)
    hip.call('brv_nchw_to_nhwc_f16', x, a.t, B, C, a.Cs, H*W, hip.stream())
    return a


def _h_to_nchw(a):
    if a.second is not None:
        return torch.cat([_h_to_nchw(_Act(a.t, a.C)), _h_to_nchw(a.second)], dim=1)
    B, H, W, Cs = a.t.shape
    y = torch.empty(B, a.C, H, W, dtype=torch.float32, device=a.t.device)
    hip.call('brv_nhwc_f16_to_nchw', a.t, y, B, a.C, Cs, H*W, hip.stream())
    return y


def _h_single(a):
    """One tensor holding all the channels of ``a`` (a copy only if ``a`` is a concatenation)."""
    if a.second is None:
        return a
    parts = [a.t[..., :a.C], a.second.t[..., :a.second.C]]
    C = a.channels
    pad = -(-C//8)*8 - C
    if pad:
        parts.append(torch.zeros(*a.t.shape[:3], pad, dtype=torch.float16, device=a.t.device))
    return _Act(torch.cat(parts, dim=3).contiguous(), C)


_ZERO_POOL = {'buf': None, 'off': 0}


def _zeros_f64(n, device):
    """n zeroed doubles out of a pooled arena (one fill per ~100 requests instead of one each)."""
    pool = _ZERO_POOL
    if pool['buf'] is None or pool['buf'].device != device or pool['off'] + n > pool['buf'].numel():
        pool['buf'] = torch.zeros(max(1 << 18, 4*n), dtype=torch.float64, device=device)
        pool['off'] = 0
    out = pool['buf'][pool['off']:pool['off'] + n]
    pool['off'] += n
    return out


def _h_sums(a):
    """Per-channel (sum, sum of squares) over the pixels, (B, C, 2) fp64; kept with the tensor: a
    skip connection's are computed once, where the encoder normalises it."""
    if a.sums is None:
        B, H, W, Cs = a.t.shape
        a.sums = _zeros_f64(B*a.C*2, a.t.device).view(B, a.C, 2)
        hip.call('brv_nhwc_chan_stats', a.t, a.sums, B, a.C, Cs, H*W, 0, a.C, hip.stream())
    return a.sums


def _h_gn_fold(a, mod, add=None, adm=None):
    """GroupNorm(a + add[:, :, None, None]) [then (1 + adm[0])*. + adm[1]] as a per-(item,
    channel) affine map: (scale, shift), each (B, C)."""
    sums = _h_sums(a)
    if a.second is not None:
        sums = torch.cat([sums, _h_sums(a.second)], dim=1).contiguous()
    B, (H, W), C = a.t.shape[0], a.hw, a.channels
    scale = torch.empty(B, C, dtype=torch.float32, device=a.t.device)
    shift = torch.empty_like(scale)
    a0, a1 = (adm[0].contiguous(), adm[1].contiguous()) if adm is not None else (None, None)
    hip.call('brv_groupnorm_fold_chan', sums, add.contiguous() if add is not None else None, mod.weight, mod.bias, a0,
             a1, scale, shift, B, C, H*W, mod.num_groups, float(mod.eps), hip.stream())
    return scale, shift


def _h_packed3(mod):
    w = mod.weight
    key = (w.data_ptr(), w._version, _PARAM_EPOCH[0])
    if getattr(mod, '_brv_hp_key', None) != key:
        Cout, Cin, k, _ = w.shape
        n = hip.lib().brv_conv_nhwc_packed_size(Cout, Cin, k)
        wp = torch.empty(n, dtype=torch.float16, device=w.device)
        hip.call('brv_conv_nhwc_pack', w.detach().contiguous(), wp, Cout, Cin, k, hip.stream())
        mod._brv_hp, mod._brv_hp_key = wp, key
    return mod._brv_hp


def _h_conv3(a, mod, fold=None, silu=False, res=None, out_scale=1.0, norm=None, add=None, adm=None):
    """out_scale*(conv3x3(act(a)) + bias + res) on the fp16 MFMA. act = the folded GroupNorm ``fold`` =
    (scale, shift) [+ SiLU], or -- ``norm`` = the GroupNorm module, ``add`` its embedding term,
    ``adm`` its modulation -- the same fold left to the convolution (``brv_conv_nhwc_forward_gn``:
    computed in the kernel's prologue from the per-channel sums, no launch in between)."""
    if a.second is not None and a.C % 32:
        a = _h_single(a)
    B, (H, W) = a.t.shape[0], a.hw
    y = _h_new(B, H, W, mod.out_channels, a.t.device)
    y.sums = _zeros_f64(B*mod.out_channels*2, a.t.device).view(B, mod.out_channels, 2)
    if res is not None:
        res = _h_single(res)
    b = a.second
    common = (a.t, a.C, a.Cs, b.t if b is not None else None, b.C if b is not None else 0,
              b.Cs if b is not None else 0, _h_packed3(mod), mod.bias,
              res.t if res is not None else None, res.Cs if res is not None else 0)
    # scratch of the launches that split their reduction over workgroups (the inner U-Net levels: csrc/conv_nhwc_splitk.cuh);
    # BRV_CONV_SPLIT=0: the pixel-parallel kernel for every launch (rounds 2 - 5)
    nsplit = hip.lib().brv_conv_nhwc_split_ws_bytes(B, H, W, a.C, b.C if b is not None else 0, mod.out_channels) \
        if _CONV_SPLIT else 0
    split_ws = torch.empty(nsplit, dtype=torch.uint8, device=a.t.device) if nsplit > 0 else None
    tail = (int(silu), y.t, y.Cs, B, H, W, mod.out_channels, 3, float(out_scale), y.sums, split_ws, nsplit,
            hip.stream())
    if norm is not None:
        ws = torch.empty(2*B*a.channels, dtype=torch.float32, device=a.t.device)
        a0, a1 = (adm[0].contiguous(), adm[1].contiguous()) if adm is not None else (None, None)
        hip.call('brv_conv_nhwc_forward_gn_ws', *common, _h_sums(a), _h_sums(b) if b is not None else None,
                 add.contiguous() if add is not None else None, norm.weight, norm.bias, a0, a1, norm.num_groups,
                 float(norm.eps), ws, *tail)
        return y
    sc, sf = fold if fold is not None else (None, None)
    hip.call('brv_conv_nhwc_forward_ws', *common, sc, sf, *tail)
    return y


def _h_conv1(a, mod, out_scale=1.0):
    """1x1 convolution of [a | a.second] (UNetBlock.skip_conv)."""
    w = mod.weight
    b = a.second
    C2 = b.C if b is not None else 0
    key = (w.data_ptr(), w._version, _PARAM_EPOCH[0], a.C, C2)
    if getattr(mod, '_brv_h1_key', None) != key:
        n = hip.lib().brv_nhwc_conv1x1_packed_size(mod.out_channels, a.C, C2)
        wp = torch.empty(n, dtype=torch.float16, device=w.device)
        hip.call('brv_nhwc_conv1x1_pack', w.detach().contiguous(), wp, mod.out_channels, a.C, C2, hip.stream())
        mod._brv_h1, mod._brv_h1_key = wp, key
    B, (H, W) = a.t.shape[0], a.hw
    y = _h_new(B, H, W, mod.out_channels, a.t.device)
    hip.call('brv_nhwc_conv1x1_forward', a.t, a.C, a.Cs, b.t if b is not None else None, C2,
             b.Cs if b is not None else 0, mod._brv_h1, mod.bias, y.t, y.Cs, B*H*W, mod.out_channels, float(out_scale),
             hip.stream())
    return y


def _h_affine_act(a, fold, silu=False):
    a = _h_single(a)
    B, H, W, Cs = a.t.shape
    y = _Act(torch.empty_like(a.t), a.C)
    hip.call('brv_nhwc_affine_act', a.t, fold[0], fold[1], y.t, B, a.C, Cs, H*W, int(silu), hip.stream())
    return y


def _h_resample(a, resampler, up_or_down):
    a = _h_single(a)
    B, H, W, Cs = a.t.shape
    K = resampler.kernel.shape[-1]
    padding, (Ho, Wo), up = resampler.plan((H, W), up_or_down)
    y = _Act(torch.empty(B, Ho, Wo, Cs, dtype=torch.float16, device=a.t.device), a.C)
    hip.call('brv_nhwc_fir_resample2d', a.t, resampler.kernel.float().contiguous(), y.t, B, Cs, H, W, Ho, Wo, K,
             padding[0], padding[1], int(up), 4.0 if up else 1.0, hip.stream())
    return y


def _h_resample_pair(a, fold, resampler, up_or_down, silu=True):
    """(resample(a), resample(act(scale*a + shift))) in one launch (the two inputs of a resampling
    UNetBlock); FIR kernels longer than 4 taps take the separate kernels."""
    a = _h_single(a)
    B, H, W, Cs = a.t.shape
    K = resampler.kernel.shape[-1]
    if K > 4:
        return (_h_resample(a, resampler, up_or_down),
                _h_resample(_h_affine_act(a, fold, silu=silu), resampler, up_or_down))
    padding, (Ho, Wo), up = resampler.plan((H, W), up_or_down)
    y = _Act(torch.empty(B, Ho, Wo, Cs, dtype=torch.float16, device=a.t.device), a.C)
    h = _Act(torch.empty_like(y.t), a.C)
    hip.call('brv_nhwc_fir_resample2d_dual', a.t, fold[0], fold[1], int(silu), resampler.kernel.float().contiguous(),
             y.t, h.t, B, a.C, Cs, H, W, Ho, Wo, K, padding[0], padding[1], int(up), 4.0 if up else 1.0, hip.stream())
    return y, h


def _h_small_conv(a, mod, fold=None, silu=False, y_in=None):
    """3x3 convolution to <= 8 channels, (B, Cout, H, W) fp32 = [y_in +] conv(act(a)) + bias."""
    a = _h_single(a)
    B, H, W, Cs = a.t.shape
    w = mod.weight
    key = (w.data_ptr(), w._version, _PARAM_EPOCH[0])
    if getattr(mod, '_brv_hs_key', None) != key:
        w16 = torch.empty(9*w.shape[0]*w.shape[1], dtype=torch.float16, device=w.device)
        hip.call('brv_nhwc_conv3x3_small_pack', w.detach().contiguous(), w16, w.shape[0], w.shape[1], hip.stream())
        mod._brv_hs, mod._brv_hs_key = w16, key
    y = torch.empty(B, mod.out_channels, H, W, dtype=torch.float32, device=a.t.device)
    sc, sf = fold if fold is not None else (None, None)
    hip.call('brv_nhwc_conv3x3_small', a.t, mod._brv_hs, mod.bias, sc, sf, int(silu),
             y_in.contiguous() if y_in is not None else None, y, B, a.C, Cs, H, W, mod.out_channels, hip.stream())
    return y


def _h_add_pointwise(a, aux, mod, out_scale=1.0):
    """out_scale*(a + conv1x1(aux)), aux (B, K <= 8, H, W) fp32 (AuxiliaryDown)."""
    a = _h_single(a)
    B, H, W, Cs = a.t.shape
    y = _Act(torch.empty_like(a.t), a.C)
    hip.call('brv_nhwc_add_pointwise', a.t, aux.contiguous(), mod.weight, mod.bias, y.t, B, a.C, Cs, mod.in_channels,
             H*W, float(out_scale), hip.stream())
    return y


# ------------------------------------------------------------------------------------------
# U-Net (parameter containers in the reference's construction order + HIP forward)
# ------------------------------------------------------------------------------------------
class GroupNorm(nn.GroupNorm):
    def __init__(self, num_channels, num_groups=32, min_channels_per_group=4, eps=1e-6):
        super().__init__(num_groups=min(num_groups, num_channels//min_channels_per_group),
                         num_channels=num_channels, eps=eps)


class GaussianFourierProjection(nn.Module):
    def __init__(self, embedding_size, scale=16.0):
        super().__init__()
        self.register_buffer('b', torch.randn(embedding_size//2)*scale)

    def forward(self, x):
        x = x.float().contiguous()
        out = torch.empty(x.numel(), 2*self.b.numel(), dtype=torch.float32, device=x.device)
        hip.call('brv_fourier_features', x, self.b, out, x.numel(), self.b.numel(), hip.stream())
        return out


class NoiseEmbedding(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.fourier_proj = GaussianFourierProjection(in_channels)
        self.linear_1 = nn.Linear(in_channels, out_channels)
        self.linear_2 = nn.Linear(out_channels, out_channels)

    def forward(self, x):
        x = self.fourier_proj(x.reshape(-1))
        x = _silu(_linear(x, self.linear_1))
        return _silu(_linear(x, self.linear_2))


class AttentionBlock(nn.Module):
    def __init__(self, num_channels):
        super().__init__()
        self.norm = GroupNorm(num_channels)
        self.conv_query = nn.Conv2d(num_channels, num_channels, 1)
        self.conv_key = nn.Conv2d(num_channels, num_channels, 1)
        self.conv_value = nn.Conv2d(num_channels, num_channels, 1)
        self.conv_out = nn.Conv2d(num_channels, num_channels, 1)

    def forward(self, x, out_scale=1.0):
        N, C, H, W = x.shape
        L = H*W
        fold = _gn_fold(x, self.norm)
        # query, key and value as ONE 1x1 convolution to 3 C channels (three launches of a few-thousand-pixel product
        # before: launch-bound, 35 us each); the products below read their thirds in place (item stride 3 C L)
        qkv = _conv(x, self._qkv_module(), fold=fold)
        q, k, v = qkv[:, :C], qkv[:, C:2*C], qkv[:, 2*C:]
        # weights (L, L) = q^T (L, C) @ k (C, L) / sqrt(C), softmax over the last dim
        w = torch.empty(N, L, L, dtype=torch.float32, device=x.device)
        # (hip.gemm_f32: with scratch for an ordered reduction split -- a 512 x 512 x 256 product is 8 tiles of the big
        # kernel, 77 us on 8 workgroups without it)
        hip.gemm_f32(q, k, w, N, L, L, C, L, L, L, 3*C*L, 3*C*L, L*L, 1, 0, 1, 0, 0, None, 0)
        w = _axpby(w, 1.0/C**0.5)
        p = torch.empty_like(w)
        hip.call('brv_softmax_rows', w, p, N*L, L, hip.stream())
        # attention^T (C, L) = v (C, L) @ weights^T (L, L)
        a = torch.empty(N, C, L, dtype=torch.float32, device=x.device)
        hip.gemm_f32(v, p, a, N, C, L, L, L, L, L, 3*C*L, L*L, C*L, 0, 1, 1, 0, 0, None, 0)
        return _conv(a.view(N, C, H, W), self.conv_out, res=x, out_scale=out_scale)

    def _qkv_module(self):
        """conv_query / conv_key / conv_value stacked along the output channels (rebuilt when a weight changes)."""
        mods = (self.conv_query, self.conv_key, self.conv_value)
        key = tuple((t.data_ptr(), t._version) for m in mods for t in (m.weight, m.bias)) + (_PARAM_EPOCH[0],)
        if getattr(self, '_qkv_key', None) != key:
            import types
            self._qkv = types.SimpleNamespace(
                weight=torch.cat([m.weight.detach() for m in mods]).contiguous(),
                bias=torch.cat([m.bias.detach() for m in mods]).contiguous(),
                out_channels=3*self.conv_query.out_channels, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0))
            self._qkv_key = key
        return self._qkv

    def forward_h(self, x, out_scale=1.0):
        # (self-attention sits at the 16-row resolution and in the bottleneck only: a few thousand
        # pixels, run on the fp32 layout)
        return _h_from_nchw(self.forward(_h_to_nchw(x), out_scale=out_scale))


class UNetBlock(nn.Module):
    def __init__(self, in_channels, out_channels, emb_channels, block_type, skip_scale, dropout,
                 attention=False, resampler=None, up_or_down='none'):
        super().__init__()
        self.skip_scale = skip_scale
        self.norm_1 = GroupNorm(in_channels)
        self.conv_1 = nn.Conv2d(in_channels, out_channels, 3, 1, 1)
        self.linear = nn.Linear(emb_channels, out_channels*(2 if block_type == 'adm' else 1))
        self.norm_2 = GroupNorm(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv_2 = nn.Conv2d(out_channels, out_channels, 3, 1, 1)
        if in_channels != out_channels or (block_type == 'ncsn' and resampler is not None):
            self.skip_conv = nn.Conv2d(in_channels, out_channels, 1)
        else:
            self.skip_conv = None
        self.resampler = resampler
        self.up_or_down = up_or_down
        self.attn = AttentionBlock(out_channels) if attention else None
        self.block_type = block_type
        self._e = None            # this block's slice of DiffusionUNet._block_embeddings

    def forward(self, x, emb):
        if self.resampler is not None:
            h = self.resampler(_group_norm(x, self.norm_1, silu=True), self.up_or_down)
            x = self.resampler(x, self.up_or_down)
            h = _conv(h, self.conv_1)
        else:
            h = _conv(x, self.conv_1, fold=_gn_fold(x, self.norm_1), silu=True)
        e = self._e if self._e is not None else _linear(emb, self.linear)   # (N, out or 2*out)
        if e.shape[0] != h.shape[0]:
            e = e.expand(h.shape[0], -1).contiguous()
        if self.block_type == 'adm':                          # silu((scale + 1)*norm(h) + shift)
            fold = _gn_fold(h, self.norm_2, adm=e.chunk(2, dim=1))
        else:                                                 # silu(norm(h + emb))
            fold = _gn_fold(h, self.norm_2, add=e)
        if self.skip_conv is not None:
            x = _conv(x, self.skip_conv)
        # dropout: identity at inference; x = skip_scale*(x + conv_2(...))
        x = _conv(h, self.conv_2, fold=fold, silu=True, res=x, out_scale=self.skip_scale)
        if self.attn is not None:
            x = self.attn(x, out_scale=self.skip_scale)
        return x

    def forward_h(self, x, emb):
        """``forward`` on channels-last fp16 activations (``_Act``)."""
        if self.resampler is not None:
            x, h = _h_resample_pair(x, _h_gn_fold(x, self.norm_1), self.resampler, self.up_or_down)
            h = _h_conv3(h, self.conv_1)
        else:
            h = _h_conv3(x, self.conv_1, norm=self.norm_1, silu=True)
        e = self._e if self._e is not None else _linear(emb, self.linear)
        if e.shape[0] != h.t.shape[0]:
            e = e.expand(h.t.shape[0], -1).contiguous()
        if self.skip_conv is not None:
            x = _h_conv1(x, self.skip_conv)
        if self.block_type == 'adm':
            x = _h_conv3(h, self.conv_2, norm=self.norm_2, adm=e.chunk(2, dim=1), silu=True, res=x,
                         out_scale=self.skip_scale)
        else:
            x = _h_conv3(h, self.conv_2, norm=self.norm_2, add=e, silu=True, res=x,
                         out_scale=self.skip_scale)
        if self.attn is not None:
            x = self.attn.forward_h(x, out_scale=self.skip_scale)
        return x


class EncoderBlock(nn.Module):
    def __init__(self, in_channels, out_channels, emb_channels, block_type, num_blocks,
                 skip_scale, dropout, attention, resampler):
        super().__init__()
        self.unet_blocks = nn.ModuleList([
            UNetBlock(in_channels if i == 0 else out_channels, out_channels, emb_channels,
                      block_type, skip_scale, dropout,
                      attention=False if i == num_blocks else attention,
                      resampler=resampler if i == num_blocks else None, up_or_down='down')
            for i in range(num_blocks if resampler is None else num_blocks + 1)])

    def forward(self, x, emb, skips):
        for i, blk in enumerate(self.unet_blocks):
            x = blk(x, emb)
            if i != len(self.unet_blocks) - 1:
                skips.append(x)
        return x, skips

    def forward_h(self, x, emb, skips):
        for i, blk in enumerate(self.unet_blocks):
            x = blk.forward_h(x, emb)
            if i != len(self.unet_blocks) - 1:
                skips.append(x)
        return x, skips


class DecoderBlock(nn.Module):
    def __init__(self, in_channels, out_channels, emb_channels, block_type, num_blocks,
                 skip_scale, dropout, attention, resampler, skip_channels):
        super().__init__()
        self.unet_blocks = nn.ModuleList([
            UNetBlock(in_channels if i == -1 else skip_channels.pop()
                      + (in_channels if i == 0 else out_channels),
                      in_channels if i == -1 else out_channels, emb_channels, block_type,
                      skip_scale, dropout,
                      attention=attention and (block_type == 'adm' or i == num_blocks - 1),
                      resampler=resampler if i == -1 else None, up_or_down='up')
            for i in range(0 if resampler is None else -1, num_blocks)])

    def forward(self, x, emb, skips):
        for blk in self.unet_blocks:
            if blk.resampler is None:
                x = torch.cat([x, skips.pop()], dim=1)
            x = blk(x, emb)
        return x

    def forward_h(self, x, emb, skips):
        for blk in self.unet_blocks:
            if blk.resampler is None:
                x = _h_single(x)
                cat = _Act(x.t, x.C, second=skips.pop())    # torch.cat([x, skip], dim=1), never copied
                cat.sums = x.sums                           # (sums describe the first part only)
                x = cat
            x = blk.forward_h(x, emb)
        return x


class AuxiliaryDown(nn.Module):
    def __init__(self, in_channels, out_channels, resampler, type_, skip_scale):
        super().__init__()
        self.resampler = resampler
        self.type_ = type_
        self.conv = nn.Conv2d(in_channels, out_channels, 1) if type_ == 'skip' \
            else nn.Conv2d(in_channels, out_channels, 3, 1, 1)
        self.skip_scale = skip_scale

    def forward(self, x, aux):
        aux = self.resampler(aux, 'down')
        x = _axpby(x, 1.0, _conv(aux, self.conv), 1.0)
        if self.type_ == 'residual':
            aux = x = _axpby(x, self.skip_scale)
        return x, aux

    def forward_h(self, x, aux):
        """type 'skip': the trunk ``x`` channels-last fp16, the side branch ``aux`` (B, 4, H, W) fp32."""
        aux = self.resampler(aux, 'down')
        return _h_add_pointwise(x, aux, self.conv), aux


class AuxiliaryUp(nn.Module):
    def __init__(self, in_channels, out_channels, resampler, type_):
        super().__init__()
        self.resampler = resampler
        self.type_ = type_
        self.conv = nn.Conv2d(in_channels, out_channels, 3, 1, 1)
        if type_ == 'skip' or resampler is None:
            self.norm = GroupNorm(in_channels)

    def forward(self, x, aux):
        if self.resampler is not None:
            aux = self.resampler(aux, 'up')
        if self.type_ == 'skip' or self.resampler is None:
            h = _conv(x, self.conv, fold=_gn_fold(x, self.norm), silu=True)
            aux = h if aux is None else _axpby(aux, 1.0, h, 1.0)
        else:
            x = aux = _axpby(x, 1.0, _conv(aux, self.conv), 1.0)
        return x, aux

    def forward_h(self, x, aux):
        if self.resampler is not None:
            aux = self.resampler(aux, 'up')
        aux = _h_small_conv(x, self.conv, fold=_h_gn_fold(x, self.norm), silu=True, y_in=aux)
        return x, aux


class _OutputConv(nn.Sequential):
    def forward(self, x):
        return _conv(x, self[1], fold=_gn_fold(x, self[0]))


class DiffusionUNet(nn.Module):
    def __init__(self, num_freqs, base_channels, channel_mult, num_blocks_per_res,
                 noise_channel_mult, emb_channel_mult, fir_kernel, attn_resolutions,
                 attn_bottleneck, encoder_type, decoder_type, block_type, skip_scale, dropout,
                 aux_out_channels, in_channels=4, out_channels=2):
        super().__init__()
        assert encoder_type in ['standard', 'residual', 'skip']
        assert decoder_type in ['standard', 'residual', 'skip']
        assert block_type in ['ncsn', 'adm']
        self._blocks, self._emb_key = None, None
        self._emb_gidx = {}             # (N, batch) -> index tensor; lives as long as any graph that captured it
        self._graphs = {}
        self.resampler = Resample(fir_kernel, buffer_padding=True)
        emb_channels = base_channels*emb_channel_mult
        self.emb = NoiseEmbedding(base_channels*noise_channel_mult, emb_channels)
        self.input_conv = nn.Conv2d(in_channels, base_channels, 3, 1, 1)
        num_res = len(channel_mult)
        channels = [base_channels*m for m in channel_mult]
        common = dict(emb_channels=emb_channels, block_type=block_type, skip_scale=skip_scale,
                      dropout=dropout)
        self.encoder = nn.ModuleList(
            EncoderBlock(base_channels if i == 0 else channels[i - 1], channels[i],
                         num_blocks=num_blocks_per_res, attention=num_freqs >> i in attn_resolutions,
                         resampler=None if i == num_res - 1 else self.resampler, **common)
            for i in range(num_res))
        if encoder_type != 'standard':
            self.aux_downs = nn.ModuleList(
                None if i == num_res - 1 else AuxiliaryDown(
                    in_channels if encoder_type == 'skip' or i == 0 else channels[i - 1],
                    channels[i], self.resampler, encoder_type, skip_scale)
                for i in range(num_res))
        else:
            self.aux_downs = [None]*num_res
        skip_channels = [base_channels] + [channels[i] for i in range(num_res)
                                           for _ in self.encoder[i].unet_blocks]
        self.bottleneck_block_1 = UNetBlock(channels[-1], channels[-1], attention=attn_bottleneck,
                                            **common)
        self.bottleneck_block_2 = UNetBlock(channels[-1], channels[-1], **common)
        self.decoder = nn.ModuleList(
            DecoderBlock(channels[i] if i == num_res - 1 else channels[i + 1], channels[i],
                         num_blocks=num_blocks_per_res + 1,
                         attention=num_freqs >> i in attn_resolutions,
                         resampler=None if i == num_res - 1 else self.resampler,
                         skip_channels=skip_channels, **common)
            for i in reversed(range(num_res)))
        if decoder_type != 'standard':
            self.aux_ups = nn.ModuleList(
                AuxiliaryUp(channels[i] if decoder_type == 'skip' or i == num_res - 1
                            else channels[i + 1],
                            aux_out_channels if decoder_type == 'skip' else channels[i],
                            None if i == num_res - 1 else self.resampler, decoder_type)
                for i in reversed(range(num_res)))
        else:
            self.aux_ups = [None]*num_res
        if decoder_type != 'skip':
            self.output_conv = _OutputConv(GroupNorm(channels[0]),
                                           nn.Conv2d(channels[0], out_channels, 3, 1, 1))
        else:
            self.output_conv = nn.Conv2d(aux_out_channels, out_channels, 1)

    def _block_embeddings(self, emb, batch=None):
        """``linear(emb)`` of every U-Net block in ONE matrix product per network evaluation
        (they depend on the noise level only); each block reads its slice."""
        if self._blocks is None:
            self._blocks = [m for m in self.modules() if isinstance(m, UNetBlock)]
        key = tuple((b.linear.weight.data_ptr(), b.linear.weight._version, b.linear.bias._version)
                    for b in self._blocks) + (_PARAM_EPOCH[0],)
        if self._emb_key != key:
            self._emb_w = torch.cat([b.linear.weight.detach() for b in self._blocks]).contiguous()
            self._emb_b = torch.cat([b.linear.bias.detach() for b in self._blocks]).contiguous()
            self._emb_key = key
        N, K = emb.shape
        O = self._emb_w.shape[0]
        d = torch.empty(O, N, dtype=torch.float32, device=emb.device)
        hip.call('brv_gemm_f32', self._emb_w, emb.contiguous(), d, 1, O, N, K, K, K, N, 0, 0, 0, 0, 1, 1, 0, 0,
                 self._emb_b, 0, hip.stream())
        gidx = self._emb_gidx.get((N, batch)) if batch is not None else None
        if gidx is None and batch is not None and batch % N == 0 and not torch.cuda.is_current_stream_capturing():
            # source index of every element of the blocks' (batch, out_features) slices laid out back to back: built on
            # the host once per (noise-level batch, input batch) -- in the eager warm-up evaluation, never inside a
            # HIP-graph capture. The index depends on the block widths only (fixed at construction), and a captured
            # graph bakes the tensor's address in: entries are never replaced, only dropped together with the graphs.
            parts, o = [], 0
            rows = (torch.arange(batch) % N).view(batch, 1)
            for b in self._blocks:
                n = b.linear.out_features
                parts.append(((o + torch.arange(n).view(1, n))*N + rows).reshape(-1))
                o += n
            if len(self._emb_gidx) >= 8:
                self._emb_gidx.clear()
                self._graphs.clear()
            gidx = self._emb_gidx[(N, batch)] = torch.cat(parts).to(emb.device)
        if gidx is not None:
            # ONE gather for all blocks: transposed, expanded to the input batch, contiguous per block (a transpose-copy
            # and an expand-copy per block before: 74 launches of an evaluation)
            e_all = d.view(-1).index_select(0, gidx)
            o = 0
            for b in self._blocks:
                n = b.linear.out_features
                b._e = e_all[o:o + batch*n].view(batch, n)
                o += batch*n
            return
        o = 0
        for b in self._blocks:
            n = b.linear.out_features
            b._e = d[o:o + n].t().contiguous()
            o += n

    def forward(self, x, sigma):
        """One network evaluation. Inside ``SGMSEp.enhance`` the ~800 kernel launches of an
        evaluation are captured once per input shape into a HIP graph and replayed (the
        Python-side launch cost, not the GPU, bounds an eager evaluation)."""
        sigma = torch.as_tensor(sigma, dtype=torch.float32).to(x.device).reshape(-1)
        if not _STATE['graph']:
            return self._forward_impl(x, sigma)
        key = (tuple(x.shape), tuple(sigma.shape), _STATE['amp'], _STATE['pver'])
        entry = self._graphs.get(key)
        if entry is None:
            import gc
            sx, ss = x.clone(), sigma.clone()
            # Old graphs (this model's previous shape, other models that became garbage) are released HERE, with the
            # device idle, and the cyclic collector stays off until the capture has ended: a collection that ran inside
            # the warm-up pass -- finalisers of captured graphs and of their memory pools beside a busy side stream --
            # aborted the process once in three runs of the GPU test suite (round 6)
            self._graphs.clear()                          # one shape at a time: bound the memory
            torch.cuda.synchronize(x.device)
            gc.collect()
            was_enabled = gc.isenabled()
            gc.disable()
            try:
                side = torch.cuda.Stream(device=x.device)
                side.wait_stream(torch.cuda.current_stream(x.device))
                with torch.cuda.stream(side):             # warm-up: packs weights, fills caches
                    self._forward_impl(sx, ss)
                torch.cuda.current_stream(x.device).wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = self._forward_impl(sx, ss)
            finally:
                if was_enabled:
                    gc.enable()
            entry = self._graphs[key] = (graph, sx, ss, out)
        graph, sx, ss, out = entry
        sx.copy_(x)
        ss.copy_(sigma)
        graph.replay()
        return out

    def _nhwc_ok(self):
        """The channels-last fp16 form covers the 'standard' / 'skip' encoders and decoders whose
        convolutions have the channel counts its kernels take; anything else runs the fp32-layout
        form of ``use_amp``."""
        ok = getattr(self, '_nhwc_ok_cache', None)
        if ok is None:
            ok = os.environ.get('BRV_SGMSE_NCHW', '0') != '1'
            for m in self.modules():
                if isinstance(m, (AuxiliaryDown, AuxiliaryUp)) and m.type_ != 'skip':
                    ok = False
                if isinstance(m, AuxiliaryDown) and (m.conv.kernel_size != (1, 1) or m.conv.in_channels > 8):
                    ok = False
                if isinstance(m, AuxiliaryUp) and m.conv.out_channels > 8:
                    ok = False
                if isinstance(m, UNetBlock):
                    for conv in (m.conv_1, m.conv_2):
                        if conv.out_channels % 4 or conv.in_channels % 32:
                            ok = False
            if self.input_conv.out_channels % 4 or self.input_conv.in_channels > 8:
                ok = False
            if isinstance(self.output_conv, nn.Conv2d):
                ok = ok and self.output_conv.kernel_size == (1, 1)
            else:
                ok = ok and self.output_conv[1].out_channels <= 8
            self._nhwc_ok_cache = ok
        return ok

    def _forward_nhwc(self, x, sigma):
        _ZERO_POOL['buf'] = None       # the arena is cleared inside this evaluation (and its HIP graph)
        emb = self.emb(sigma)
        self._block_embeddings(emb, x.shape[0])
        aux = x
        x = _h_conv3(_h_from_nchw(x), self.input_conv)
        skips = [x]
        for enc, aux_block in zip(self.encoder, self.aux_downs):
            x, skips = enc.forward_h(x, emb, skips)
            if aux_block is not None:
                x, aux = aux_block.forward_h(x, aux)
            skips.append(x)
        x = self.bottleneck_block_1.forward_h(x, emb)
        x = self.bottleneck_block_2.forward_h(x, emb)
        aux = None
        for dec, aux_block in zip(self.decoder, self.aux_ups):
            x = dec.forward_h(x, emb, skips)
            if aux_block is not None:
                x, aux = aux_block.forward_h(x, aux)
        if isinstance(self.output_conv, nn.Conv2d):
            return _conv(aux, self.output_conv)
        return _h_small_conv(x, self.output_conv[1], fold=_h_gn_fold(x, self.output_conv[0]))

    def _forward_impl(self, x, sigma):
        if _STATE['amp'] and self._nhwc_ok():
            return self._forward_nhwc(x, sigma)
        emb = self.emb(sigma)
        self._block_embeddings(emb, x.shape[0])
        aux = x
        x = _conv(x, self.input_conv)
        skips = [x]
        for enc, aux_block in zip(self.encoder, self.aux_downs):
            x, skips = enc(x, emb, skips)
            if aux_block is not None:
                x, aux = aux_block(x, aux)
            skips.append(x)
        x = self.bottleneck_block_1(x, emb)
        x = self.bottleneck_block_2(x, emb)
        aux = None
        for dec, aux_block in zip(self.decoder, self.aux_ups):
            x = dec(x, emb, skips)
            if aux_block is not None:
                x, aux = aux_block(x, aux)
        if aux is None:
            aux = x
        if isinstance(self.output_conv, nn.Conv2d):
            return _conv(aux, self.output_conv)
        return self.output_conv(aux)


# ------------------------------------------------------------------------------------------
# SDEs, preconditioning, solvers (scalars on the host, tensors through brv_axpby)
# ------------------------------------------------------------------------------------------
class _SDE:
    """Scalar schedules on the host (0-d / 1-d CPU tensors); the drift is
    ``drift_coef(t)*(y - x)`` for every SDE of the reference (sdes.py:11-251)."""

    def f(self, x, y, t):
        c = float(self.drift_coef(t))
        return _axpby(y, c, x, -c)


class _OUVE(_SDE):
    def __init__(self, stiffness, sigma_min, sigma_max, **kwargs):
        self.stiffness = stiffness
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max
        self._sigma_p = sigma_max/sigma_min
        self._log_sigma_p = math.log(sigma_max/sigma_min)

    def s(self, t):
        return (-self.stiffness*t).exp()

    def drift_coef(self, t):
        return self.stiffness


@SDERegistry.register('richter-ouve')
class RichterOUVESDE(_OUVE):
    def sigma(self, t):
        return self.sigma_min*(((self._sigma_p**t/self.s(t))**2 - 1)
                               / (1 + self.stiffness/self._log_sigma_p))**0.5

    def g(self, t):
        return self.sigma_min*self._sigma_p**t*(2*self._log_sigma_p)**0.5

    def sigma_inv(self, sigma):
        return 0.5*(1 + (1 + self.stiffness/self._log_sigma_p)*(sigma/self.sigma_min)**2).log() \
            / (self.stiffness + self._log_sigma_p)


@SDERegistry.register('brever-ouve')
class BreverOUVESDE(_OUVE):
    def sigma(self, t):
        return self.sigma_min*(self._sigma_p**(2*t) - 1)**0.5

    def g(self, t):
        return self.s(t)*self.sigma_min*self._sigma_p**t*(2*self._log_sigma_p)**0.5

    def sigma_inv(self, sigma):
        return 0.5*((sigma/self.sigma_min)**2 + 1).log()/self._log_sigma_p


class _VP(_SDE):
    def s(self, t):
        return (-self.stiffness*t).exp()/(1 + self.sigma(t)**2)**0.5

    def drift_coef(self, t):
        return self.stiffness + 0.5*self.beta(t)

    def g(self, t):
        return (-self.stiffness*t).exp()*self.beta(t)**0.5


@SDERegistry.register('brever-ouvp')
class BreverOUVPSDE(_VP):
    def __init__(self, stiffness, beta_min, beta_max, **kwargs):
        self.stiffness = stiffness
        self.beta_min = beta_min
        self._beta_d = beta_max - beta_min

    def beta(self, t):
        return self.beta_min + self._beta_d*t

    def sigma(self, t):
        return ((0.5*self._beta_d*t**2 + self.beta_min*t).exp() - 1)**0.5

    def sigma_inv(self, sigma):
        return ((self.beta_min**2 + 2*self._beta_d*(sigma**2 + 1).log())**0.5
                - self.beta_min)/self._beta_d


@SDERegistry.register('brever-oucosine')
class BreverOUCosineSDE(_VP):
    def __init__(self, stiffness, lambda_min, lambda_max, shift, beta_clamp, **kwargs):
        self.stiffness = stiffness
        self.shift = shift
        self.t_min = self._lambda_inv(lambda_min + shift)
        self.t_max = self._lambda_inv(lambda_max + shift)
        self.t_d = self.t_min - self.t_max
        self.beta_clamp = beta_clamp

    def _lambda_inv(self, lam):
        if isinstance(lam, torch.Tensor):
            return 2/math.pi*((self.shift - lam)/2).exp().atan()
        return 2/math.pi*math.atan(math.exp((self.shift - lam)/2))

    def _angle(self, t):
        return math.pi*(self.t_max + self.t_d*t)/2

    def beta(self, t):
        a = self._angle(t)
        return (math.pi*self.t_d/a.cos()**2*a.tan()
                / (math.exp(self.shift) + a.tan()**2)).clamp(max=self.beta_clamp)

    def sigma(self, t):
        lam = -2*self._angle(t).tan().log() + self.shift
        return (-lam/2).exp()

    def sigma_inv(self, sigma):
        return (self._lambda_inv(-2*sigma.log()) - self.t_max)/self.t_d


class _BridgeSDE(_SDE):
    t_max = 0.999

    def __init__(self, scaling=0.1, **kwargs):
        self.scaling = scaling

    def s(self, t):
        return 1 - t*self.t_max

    def drift_coef(self, t):
        return 1/(1 - t*self.t_max)


@SDERegistry.register('bbed')
class BBEDSDE(_BridgeSDE):
    def __init__(self, scaling=0.1, k=10.0, **kwargs):
        super().__init__(scaling)
        self.k = k

    def g(self, t):
        return self.scaling*self.k**(t*self.t_max)

    def sigma(self, t):
        from scipy.special import expi
        t = t*self.t_max
        k2, logk2 = self.k**2, 2*math.log(self.k)
        ei = torch.as_tensor(expi(((t - 1)*logk2).numpy()))
        return self.scaling*(k2*logk2*(ei - float(expi(-logk2))) - k2**t/(t - 1) - 1)**0.5


@SDERegistry.register('bbcd')
class BBCD(_BridgeSDE):
    def g(self, t):
        return self.scaling

    def sigma(self, t):
        t = t*self.t_max
        return self.scaling*(t/(1 - t))**0.5

    def sigma_inv(self, sigma):
        return sigma**2/(self.scaling**2 + sigma**2)/self.t_max


@SDERegistry.register('bbls')
class BBLS(_BridgeSDE):
    def g(self, t):
        t = t*self.t_max
        return self.scaling*(1 - t)*(2*t)**0.5

    def sigma(self, t):
        return self.scaling*t*self.t_max

    def sigma_inv(self, sigma):
        return sigma/(self.scaling*self.t_max)


def _randn(model, shape, device, complex_):
    """Gaussian noise of the solvers (tests replace ``model._noise_source`` to replay)."""
    if model._noise_source is not None:
        return model._noise_source(shape, complex_).to(device)
    dtype = torch.complex64 if complex_ else torch.float32
    return torch.randn(shape, dtype=dtype, device=device)


class Preconditioning(nn.Module):
    def __init__(self, raw_net, sde, cskip, cout, cin, cshift, cnoise, weight, sigma_data):
        super().__init__()
        self.net = raw_net
        self.sde = sde
        table = {
            'richter': dict(
                cskip=lambda sigma: 1,
                cout=lambda sigma, scaling, t: -scaling*sigma**2/t,
                cin=lambda sigma, scaling: scaling,
                cshift=lambda cin, scaling: 1.0,                    # multiplies y
                cnoise=lambda sigma, t: t.log(),
                weight=lambda sigma: 1/sigma**2),
            'edm': dict(
                cskip=lambda sigma: sigma_data**2/(sigma**2 + sigma_data**2),
                cout=lambda sigma, scaling, t: sigma*sigma_data/(sigma**2 + sigma_data**2)**0.5,
                cin=lambda sigma, scaling: 1/(sigma**2 + sigma_data**2)**0.5,
                cshift=lambda cin, scaling: 0.0,
                cnoise=lambda sigma, t: sigma.log()/4,
                weight=lambda sigma: (sigma**2 + sigma_data**2)/(sigma*sigma_data)**2),
            'edm-scaled-shift': dict(cshift=lambda cin, scaling: cin/scaling),
        }
        for arg, val in (('cskip', cskip), ('cout', cout), ('cin', cin), ('cshift', cshift),
                         ('cnoise', cnoise), ('weight', weight)):
            if val not in table or arg not in table[val]:
                raise ValueError(f'Invalid preconditioning {arg}: {val}')
            setattr(self, arg, table[val][arg])

    def forward(self, x, y, sigma, t):
        """x, y complex (B, 1, F, T); sigma, t 0-d tensors (one noise level per call)."""
        scaling = self.sde.s(t)
        cskip, cout = self.cskip(sigma), self.cout(sigma, scaling, t)
        cin = self.cin(sigma, scaling)
        x_in = _axpby(x, float(cin), y, float(self.cshift(cin, scaling)))
        net_in = torch.cat([x_in.real, x_in.imag, y.real, y.imag], dim=1).contiguous()
        net_out = self.net(net_in, self.cnoise(sigma, t))
        net_out = torch.complex(net_out[:, 0], net_out[:, 1]).unsqueeze(1)
        return _axpby(x, float(cskip), net_out, float(cout))

    def forward_train(self, x, y, sigma, t):
        """The same denoiser with per-item noise levels (``sigma``, ``t`` of shape (B, 1, 1, 1) on
        the device) and gradients with respect to the network parameters (the training
        objective, sgmse.py:163-176); the pre / post scaling are a few elementwise torch ops on
        (B, 1, F, T), the network is ``sgmse_train.unet``."""
        from . import sgmse_train
        scaling = self.sde.s(t)
        cskip, cout = self.cskip(sigma), self.cout(sigma, scaling, t)
        cin = self.cin(sigma, scaling)
        x_in = cin*x + self.cshift(cin, scaling)*y
        net_in = torch.cat([x_in.real, x_in.imag, y.real, y.imag], dim=1).float().contiguous()
        net_out = sgmse_train.unet(self.net, net_in, self.cnoise(sigma, t).float())
        net_out = torch.complex(net_out[:, 0], net_out[:, 1]).unsqueeze(1)
        return cskip*x + cout*net_out

    def score(self, x, y, sigma, t):
        d = self(x, y, sigma, t)
        c = 1.0/float(self.sde.s(t)*sigma**2)
        return _axpby(d, c, x, -c)


@SolverRegistry.register('pc')
class PCSolver:
    def __init__(self, num_steps, corrector_steps, corrector_snr, **kwargs):
        self.num_steps = num_steps
        self.corrector_steps = corrector_steps
        self.corrector_snr = corrector_snr

    def __call__(self, sde, y, model, owner):
        dt = -1/self.num_steps
        t = torch.arange(1, 0, dt)                             # host scalars, fp32 as the reference
        sigma = sde.sigma(t)
        one = torch.tensor(1)
        x = _axpby(y, 1.0, _randn(owner, y.shape, y.device, True), float(sde.s(one)*sde.sigma(one)))
        eps = 2*(self.corrector_snr*sde.s(t)*sigma)**2

        def score_at(i):
            x_tilde = _axpby(x, 1.0/float(sde.s(t[i])), y, -1.0/float(sde.s(t[i])))
            return model.score(x_tilde, y, sigma[i], t[i])
        for i in range(self.num_steps):
            for _ in range(self.corrector_steps):
                x = _axpby(x, 1.0, score_at(i), float(eps[i]))
                x = _axpby(x, 1.0, _randn(owner, x.shape, x.device, True), float((2*eps[i])**0.5))
            score = score_at(i)
            g = float(sde.g(t[i]))
            drift = sde.f(x, y, t[i])
            if i < self.num_steps - 1:                         # reverse_step (sdes.py:17-19)
                step = _axpby(drift, dt, score, -g*g*dt)
                x = _axpby(x, 1.0, step, 1.0)
                x = _axpby(x, 1.0, _randn(owner, x.shape, x.device, False), g*(-dt)**0.5)
            else:                                              # probability flow, no noise
                step = _axpby(drift, dt, score, -0.5*g*g*dt)
                x = _axpby(x, 1.0, step, 1.0)
            hook = getattr(owner, '_step_hook', None)          # tests: the state after every reverse step
            if hook is not None:
                hook(i, x)
        return x, self.num_steps*(self.corrector_steps + 1)


@SolverRegistry.register('edm')
class EDMSolver:
    def __init__(self, num_steps, schurn, smin, smax, snoise, **kwargs):
        self.num_steps = num_steps
        self.schurn = schurn
        self.smin = smin
        self.smax = smax
        self.snoise = snoise
        self._gamma = min(schurn/num_steps, 2**0.5 - 1)

    def __call__(self, sde, y, model, owner):
        t = torch.linspace(1, 0, self.num_steps + 1)
        sigma = sde.sigma(t)
        one = torch.tensor(1)
        x = _axpby(y, 1.0, _randn(owner, y.shape, y.device, True), float(sde.s(one)*sde.sigma(one)))

        def flow(xc, tc, sc):
            x_tilde = _axpby(xc, 1.0/float(sde.s(tc)), y, -1.0/float(sde.s(tc)))
            score = model.score(x_tilde, y, sc, tc)
            return _axpby(sde.f(xc, y, tc), 1.0, score, -0.5*float(sde.g(tc))**2)
        for i in range(self.num_steps):
            eps = _randn(owner, x.shape, x.device, True)
            gamma = self._gamma if self.smin <= sigma[i] <= self.smax else 0
            sigma_hat = sigma[i]*(1 + gamma)
            t_hat = sde.sigma_inv(sigma_hat)
            r = float(sde.s(t_hat)/sde.s(t[i]))
            x_hat = _axpby(x, r, y, 1.0 - r)
            x_hat = _axpby(x_hat, 1.0, eps, self.snoise*float(
                sde.s(t_hat)*(sigma_hat**2 - sigma[i]**2)**0.5))
            d_hat = flow(x_hat, t_hat, sigma_hat)
            h = float(t[i + 1] - t_hat)
            x = _axpby(x_hat, 1.0, d_hat, h)
            if i < self.num_steps - 1:
                d_next = flow(x, t[i + 1], sigma[i + 1])
                x = _axpby(x_hat, 1.0, _axpby(d_hat, 1.0, d_next, 1.0), 0.5*h)
        return x, 2*self.num_steps


# ------------------------------------------------------------------------------------------
@ModelRegistry.register('sgmsep')
class SGMSEp(BreverBaseModel):
    _fused_adam = True       # clip + Adam as brv_clip_adam_step2 on one flat buffer (models/base.py)

    def mark_params_changed(self):
        """Parameters were written without touching ``Tensor._version`` (FlatAdam's raw-pointer launch, EMA's
        ``param.data.copy_``): every cached copy derived from a weight and every captured graph is stale."""
        _PARAM_EPOCH[0] += 1

    def __init__(
        self,
        stft_frame_length: int = 512,
        stft_hop_length: int = 128,
        stft_window: str = 'hann',
        stft_compression_factor: float = 0.5,
        stft_scale_factor: float = 0.15,
        stft_discard_nyquist: bool = True,
        sde_name: str = 'richter-ouve',
        sde_stiffness: float = 1.5,
        sde_ve_sigma_min: float = 0.05,
        sde_ve_sigma_max: float = 0.5,
        sde_vp_beta_min: float = 0.01,
        sde_vp_beta_max: float = 1.0,
        sde_cosine_lambda_min: float = -12.0,
        sde_cosine_lambda_max: float = float('inf'),
        sde_cosine_shift: float = 3.0,
        sde_cosine_beta_clamp: float = 10.0,
        sde_bb_scaling: float = 0.1,
        sde_bb_k: float = 10.0,
        solver_name: str = 'pc',
        solver_num_steps: int = 16,
        solver_edm_schurn: float = float('inf'),
        solver_edm_smin: float = 0.0,
        solver_edm_smax: float = float('inf'),
        solver_edm_snoise: float = 1.0,
        solver_pc_corrector_steps: int = 1,
        solver_pc_corrector_snr: float = 0.5,
        net_base_channels: int = 128,
        net_channel_mult: list[int] = [1, 1, 2, 2, 2, 2, 2],
        net_num_blocks_per_res: int = 2,
        net_noise_channel_mult: int = 2,
        net_emb_channel_mult: int = 4,
        net_fir_kernel: list[int] = [1, 3, 3, 1],
        net_attn_resolutions: list[int] = [16],
        net_attn_bottleneck: bool = True,
        net_encoder_type: str = 'skip',
        net_decoder_type: str = 'skip',
        net_block_type: str = 'ncsn',
        net_skip_scale: float = 0.5 ** 0.5,
        net_dropout: float = 0.0,
        net_aux_out_channels: int = 4,
        preconditioning_cskip: str = 'richter',
        preconditioning_cout: str = 'richter',
        preconditioning_cin: str = 'richter',
        preconditioning_cnoise: str = 'richter',
        preconditioning_cshift: str = 'richter',
        preconditioning_weight: str = 'richter',
        preconditioning_sigma_data: float = 0.1,
        t_eps: float = 0.01,
        criterion: str = 'mse',
        optimizer: str = 'Adam',
        learning_rate: float = 0.0001,
    ):
        super().__init__(criterion=criterion)
        self.stft = STFT(frame_length=stft_frame_length, hop_length=stft_hop_length,
                         window=stft_window, compression_factor=stft_compression_factor,
                         scale_factor=stft_scale_factor, normalized=False)
        self.stft_discard_nyquist = stft_discard_nyquist
        self.sde = SDERegistry.get(sde_name)(
            stiffness=sde_stiffness, sigma_min=sde_ve_sigma_min, sigma_max=sde_ve_sigma_max,
            beta_min=sde_vp_beta_min, beta_max=sde_vp_beta_max, lambda_min=sde_cosine_lambda_min,
            lambda_max=sde_cosine_lambda_max, shift=sde_cosine_shift,
            beta_clamp=sde_cosine_beta_clamp, scaling=sde_bb_scaling, k=sde_bb_k)
        self.solver = SolverRegistry.get(solver_name)(
            num_steps=solver_num_steps, schurn=solver_edm_schurn, smin=solver_edm_smin,
            smax=solver_edm_smax, snoise=solver_edm_snoise,
            corrector_steps=solver_pc_corrector_steps, corrector_snr=solver_pc_corrector_snr)
        raw_net = DiffusionUNet(
            num_freqs=stft_frame_length//2, base_channels=net_base_channels,
            channel_mult=net_channel_mult, num_blocks_per_res=net_num_blocks_per_res,
            noise_channel_mult=net_noise_channel_mult, emb_channel_mult=net_emb_channel_mult,
            fir_kernel=net_fir_kernel, attn_resolutions=net_attn_resolutions,
            attn_bottleneck=net_attn_bottleneck, encoder_type=net_encoder_type,
            decoder_type=net_decoder_type, block_type=net_block_type, skip_scale=net_skip_scale,
            dropout=net_dropout, aux_out_channels=net_aux_out_channels)
        self.model = Preconditioning(
            raw_net=raw_net, sde=self.sde, cskip=preconditioning_cskip, cout=preconditioning_cout,
            cin=preconditioning_cin, cnoise=preconditioning_cnoise, cshift=preconditioning_cshift,
            weight=preconditioning_weight, sigma_data=preconditioning_sigma_data)
        self.t_eps = t_eps
        self._noise_source = None
        self.optimizer = self.init_optimizer(optimizer, lr=learning_rate)

    def transform(self, sources):
        assert sources.shape[0] == 2  # mixture, foreground
        home = sources.device
        dev = home if home.type == 'cuda' else next(self.parameters()).device
        if dev.type != 'cuda':
            if not torch.cuda.is_available():
                raise RuntimeError('the HIP path needs a ROCm device (no CPU fallback)')
            dev = torch.device('cuda', torch.cuda.current_device())
        sources = sources.to(dev).mean(axis=-2)
        sources = sources/sources[0].abs().max()
        sources = self.stft(sources)
        if self.stft_discard_nyquist:
            sources = sources[..., :-1, :]
        return sources.to(home)

    @torch.no_grad()
    def forward(self, x, y, sigma, t):
        """Denoiser D(x; y, sigma, t): one noise level for the whole batch (0-d ``sigma``, ``t``:
        the samplers' fast path), or one level per item (``sigma``, ``t`` of shape (B, 1, 1, 1), as
        the training objective and the reference's known-answer test use it)."""
        hip.require_device(x, y)
        sigma, t = torch.as_tensor(sigma).float(), torch.as_tensor(t).float()
        if sigma.numel() > 1 or t.numel() > 1:
            return self.model.forward_train(x.to(torch.complex64), y.to(torch.complex64),
                                            sigma.to(x.device), t.to(x.device))
        return self.model(x.to(torch.complex64), y.to(torch.complex64), sigma.cpu(), t.cpu())

    def _draw_t(self, n, device):
        return torch.rand(n, 1, 1, 1, device=device)*(1 - self.t_eps) + self.t_eps

    def _draw_noise(self, x_0):
        return torch.randn_like(x_0)

    def loss(self, batch, lengths, use_amp):
        """Denoising score matching objective (sgmse.py:163-176); ``use_amp`` runs the
        convolutions (forward, data and weight gradients) with bf16 operands and fp32
        accumulation, everything else stays fp32."""
        hip.require_device(batch)
        y, x_0 = batch[:, 0].unsqueeze(1), batch[:, 1].unsqueeze(1)     # noisy, clean
        t = self._draw_t(x_0.shape[0], y.device)
        sigma = self.sde.sigma(t)
        n = sigma*self._draw_noise(x_0)
        weight = self.model.weight(sigma)
        with amp(use_amp):
            d = self.model.forward_train(x_0 - y + n, y, sigma, t)
        return self.criterion(d, x_0 - y, lengths, weight=weight).mean()

    @torch.no_grad()
    def _enhance(self, x, use_amp):
        hip.require_device(x)
        length = x.shape[-1]
        x = x.mean(axis=-2, keepdims=True)                     # (B, 1, L)
        norm = x.abs().amax(axis=-1, keepdims=True)
        x = x/norm
        x = self.stft(x)
        if self.stft_discard_nyquist:
            x = x[..., :-1, :]
        net = self.model.net
        first = next(net.parameters())
        _STATE['pver'] = (first.data_ptr(), sum(p._version for p in net.parameters()), _PARAM_EPOCH[0])
        _STATE['graph'] = os.environ.get('BRV_NO_GRAPH', '0') != '1'
        try:
            with hip_autocast(use_amp):
                x, nfe = self.solver(self.sde, x.contiguous(), self.model, self)
        finally:
            _STATE['graph'] = False
        x = torch.nn.functional.pad(x, (0, 0, 0, 1))           # pad the Nyquist bin
        x = self.stft.backward(x)
        x = x*norm
        return x[..., :length].squeeze(1)


@ModelRegistry.register('sgmsepm')
class SGMSEpM(SGMSEp):
    _is_submodel = True

    def __init__(self, net_channel_mult: list[int] = [1, 2, 2, 2], net_num_blocks_per_res: int = 1,
                 net_attn_resolutions: list[int] = [], **kwargs):
        super().__init__(net_channel_mult=net_channel_mult,
                         net_num_blocks_per_res=net_num_blocks_per_res,
                         net_attn_resolutions=net_attn_resolutions, **kwargs)


def _edm_kwargs(defaults, kwargs):
    """Merged constructor arguments of the EDM sub-models. The reference declares
    ``sde_stiffness = 0.0`` on them but never forwards it to ``SGMSEp.__init__``
    (sgmse.py:243-264, 268-289, 293-338), so the effective stiffness is the parent's 1.5
    whatever the caller passes; reproduced here so that results are identical."""
    merged = {**defaults, **kwargs}
    merged.pop('sde_stiffness', None)
    return merged


_EDM_COSINE = dict(sde_name='brever-oucosine', sde_stiffness=0.0, solver_name='edm',
                   preconditioning_cskip='edm', preconditioning_cout='edm',
                   preconditioning_cin='edm', preconditioning_cnoise='edm',
                   preconditioning_cshift='edm', preconditioning_weight='edm')


@ModelRegistry.register('sgmsepheun')
class sgmsepheun(SGMSEp):
    _is_submodel = True
    _defaults = _EDM_COSINE          # read by config.model_defaults like a signature

    def __init__(self, **kwargs):
        super().__init__(**_edm_kwargs(sgmsepheun._defaults, kwargs))


@ModelRegistry.register('sgmsepmheun')
class sgmsepmheun(SGMSEpM):
    _is_submodel = True
    _defaults = _EDM_COSINE

    def __init__(self, **kwargs):
        super().__init__(**_edm_kwargs(sgmsepmheun._defaults, kwargs))


@ModelRegistry.register('idmse')
class IDMSE(SGMSEp):
    _is_submodel = True
    _defaults = dict(_EDM_COSINE, net_base_channels=64, net_channel_mult=[1, 2, 3, 4],
                     net_num_blocks_per_res=1, net_noise_channel_mult=1, net_emb_channel_mult=4,
                     net_fir_kernel=[1, 1], net_attn_resolutions=[], net_encoder_type='standard',
                     net_decoder_type='standard', net_block_type='adm')

    def __init__(self, **kwargs):
        super().__init__(**_edm_kwargs(IDMSE._defaults, kwargs))
