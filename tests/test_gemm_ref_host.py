"""tests/gemm_ref.py against torch's own operators on the CPU: the reference of tests/test_gpu_gemm.py is held to
``F.unfold`` (mode 1, exact) and to float64 ``F.conv_transpose2d`` (mode 2), and ``product`` to einsum."""
import pytest
import torch
import torch.nn.functional as F

from gemm_ref import column_matrix, conv_grid, product, round_bf16, tconv_grid

#             kernel  stride  padding output_padding
GEOMETRIES = [((5, 2), (2, 1), (2, 0), (1, 0)),         # DCCRN
              ((3, 3), (1, 1), (1, 1), (0, 0)),         # 3 x 3 same
              ((7, 7), (3, 2), (3, 3), (2, 1)),
              ((2, 3), (2, 3), (0, 1), (0, 0))]
IDS = ['%dx%d_s%d%d_p%d%d_op%d%d' % (k + s + p + op) for k, s, p, op in GEOMETRIES]


@pytest.mark.parametrize('geom', GEOMETRIES, ids=IDS)
def test_mode_1_is_unfold(geom):
    k, s, p, _ = geom
    g = torch.Generator().manual_seed(1)
    for C, H, W in ((3, 16, 21), (2, 9, 10), (1, 7, 7)):
        img = torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
        grid = conv_grid((H, W), k, s, p)
        assert torch.equal(column_matrix(img, 1, k, s, p, grid), F.unfold(img, k, padding=p, stride=s))


@pytest.mark.parametrize('geom', GEOMETRIES, ids=IDS)
def test_mode_2_is_the_transposed_convolution(geom):
    k, s, p, op = geom
    g = torch.Generator().manual_seed(2)
    for C, H, W in ((3, 16, 21), (2, 9, 10), (1, 7, 7)):
        M = 4
        img = torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
        a = torch.randn(M, C*k[0]*k[1], generator=g, dtype=torch.float64)
        grid = tconv_grid((H, W), k, s, p, op)
        got = (a @ column_matrix(img, 2, k, s, p, grid)).reshape(2, M, *grid)
        want = F.conv_transpose2d(img, a.reshape(M, C, *k).transpose(0, 1), stride=s, padding=p, output_padding=op)
        assert float((got - want).abs().max()) <= 1e-13*float(want.abs().max())


def test_mode_2_without_output_padding_is_the_adjoint_of_mode_1():
    """<col1(x), g> == <x, fold(g)> and fold(g)[c] = sum over window rows of g gathered by mode 2 with the window
    unrotated: checked through the identity col2(g)-gather == F.fold of one-hot rows."""
    k, s, p = (5, 2), (2, 1), (2, 0)
    g = torch.Generator().manual_seed(3)
    C, H, W = 2, 10, 7
    Ho, Wo = conv_grid((H, W), k, s, p)
    col = torch.randn(C*k[0]*k[1], Ho*Wo, generator=g, dtype=torch.float64)
    want = F.fold(col[None], (H, W), k, padding=p, stride=s)[0]
    # fold as a gather: image pixel (h, w) of channel c sums col[(c, i, j)][(h + ph - i)/sh, (w + pw - j)/sw]
    khw = k[0]*k[1]
    got = torch.zeros(C, H, W, dtype=torch.float64)
    for c in range(C):
        rows = col[c*khw:(c + 1)*khw].reshape(khw, Ho, Wo)         # one "image" per window element
        cm = column_matrix(rows, 2, k, s, p, (H, W))               # (khw*khw, H*W): row (r, i, j)
        pick = torch.arange(khw)*khw + torch.arange(khw)           # row r = its own (i, j)
        got[c] = cm[pick].sum(0).reshape(H, W)
    assert float((got - want).abs().max()) <= 1e-13


def test_product_is_the_plain_sum_of_products():
    g = torch.Generator().manual_seed(4)
    batch, kbatch, M, N, K = 2, 3, 5, 7, 4
    for ta in (0, 1):
        for tb in (0, 1):
            a = torch.randn(batch, kbatch, *((K, M + 2) if ta else (M, K + 2)), generator=g)
            b = torch.randn(1, kbatch, *((N, K + 3) if tb else (K, N + 3)), generator=g)
            av, bv = a[..., :M] if ta else a[..., :K], b[..., :K] if tb else b[..., :N]
            bias, d0 = torch.randn(N, generator=g), torch.randn(batch, M, N, generator=g)
            want = torch.zeros(batch, M, N, dtype=torch.float64)
            for z in range(batch):
                for kb in range(kbatch):
                    for m in range(M):
                        for n in range(N):
                            for kk in range(K):
                                x = av[z, kb, kk, m] if ta else av[z, kb, m, kk]
                                y = bv[0, kb, n, kk] if tb else bv[0, kb, kk, n]
                                want[z, m, n] += float(x)*float(y)
            want += bias.double()[None, None, :] + d0.double()
            got = product(av, bv, ta, tb, bias, True, d0)
            assert float((got - want).abs().max()) <= 1e-13


def test_round_bf16_rounds_to_nearest_even():
    one = 1.0
    ulp = 2.0**-7                              # bf16 spacing in [1, 2)
    t = torch.tensor([one + ulp/2, one + 3*ulp/2, one + ulp/2 + 2.0**-20, one + ulp/4, -3.0, 0.0])
    want = torch.tensor([one, one + 2*ulp, one + ulp, one, -3.0, 0.0], dtype=torch.float64)
    assert torch.equal(round_bf16(t), want)
