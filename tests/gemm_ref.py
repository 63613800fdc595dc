"""Float64 restatement of the general matrix products of include/brever_hip.h (brv_gemm_f32, brv_gemm_bf16,
brv_gemm_bf16_mixed, brv_gemm_bf16_conv, brv_matmul_f32), the yardstick of tests/test_gpu_gemm.py.

Plain torch on the CPU; nothing of brever_amd is imported. tests/test_gemm_ref_host.py holds ``column_matrix`` to
``F.unfold`` (mode 1) and to ``F.conv_transpose2d`` (mode 2)."""
import torch


def round_bf16(t):
    """The value a kernel sees after rounding an operand to bf16 (nearest even: common.cuh f2bf / pack2)."""
    return t.to(torch.bfloat16).double()


def product(a, b, ta, tb, bias=None, col_bias=False, d0=None):
    """``sum_kb op(a[z, kb]) @ op(b[z, kb]) (+ bias) (+ d0)`` in float64.

    ``a``, ``b``: (batch | 1, kbatch, rows, cols) AS STORED -- views of their extent inside storage with a padded
    leading dimension: a is (K, M) with ``ta`` else (M, K), b is (N, K) with ``tb`` else (K, N). ``bias``: (M,), or
    (N,) with ``col_bias``. ``d0``: (batch, M, N), the previous result of an accumulating call."""
    opa = a.double().transpose(-1, -2) if ta else a.double()
    opb = b.double().transpose(-1, -2) if tb else b.double()
    out = (opa @ opb).sum(1)
    if bias is not None:
        out = out + (bias.double()[None, None, :] if col_bias else bias.double()[None, :, None])
    if d0 is not None:
        out = out + d0.double()
    return out


def column_matrix(img, mode, kernel, stride, padding, grid):
    """The (C*kh*kw, Ho*Wo) column matrix of ``img`` (..., C, H, W) over the pixel grid ``grid`` = (Ho, Wo), by the
    index arithmetic of the header: row r = (c, i, j) of a kh x kw window, column = pixel (y, x);

      mode 1: img[c][y*sh - ph + i][x*sw - pw + j]
      mode 2: img[c][(y + ph - i)/sh][(x + pw - j)/sw]   where both numerators are >= 0 and divisible

    and zero outside the image. Leading axes of ``img`` are kept."""
    (kh, kw), (sh, sw), (ph, pw), (Ho, Wo) = kernel, stride, padding, grid
    C, H, W = img.shape[-3:]
    r = torch.arange(C*kh*kw)
    c, i, j = r//(kh*kw), (r % (kh*kw))//kw, r % kw
    pix = torch.arange(Ho*Wo)
    y, x = pix//Wo, pix % Wo
    if mode == 1:
        hi = y[None, :]*sh - ph + i[:, None]
        wi = x[None, :]*sw - pw + j[:, None]
        live = torch.ones_like(hi, dtype=torch.bool)
    elif mode == 2:
        hn = y[None, :] + ph - i[:, None]
        wn = x[None, :] + pw - j[:, None]
        live = (hn >= 0) & (wn >= 0) & (hn % sh == 0) & (wn % sw == 0)
        hi = torch.div(hn.clamp(min=0), sh, rounding_mode='floor')
        wi = torch.div(wn.clamp(min=0), sw, rounding_mode='floor')
    else:
        raise ValueError('mode is 1 or 2')
    live = live & (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
    flat = (c[:, None]*H + hi.clamp(0, H - 1))*W + wi.clamp(0, W - 1)
    out = img.reshape(*img.shape[:-3], C*H*W)[..., flat]
    return torch.where(live, out, torch.zeros((), dtype=img.dtype))


def conv_grid(size, kernel, stride, padding):
    """Output grid of the convolution (mode 1)."""
    return tuple((n + 2*p - k)//s + 1 for n, k, s, p in zip(size, kernel, stride, padding))


def tconv_grid(size, kernel, stride, padding, output_padding=(0, 0)):
    """Output grid of the transposed convolution (mode 2)."""
    return tuple((n - 1)*s - 2*p + k + op for n, k, s, p, op in zip(size, kernel, stride, padding, output_padding))
