"""The autograd nodes of brever_amd/models/_ops.py that more than one model runs, against float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.double()
    return float((a - b).norm()/b.norm())


@pytest.mark.parametrize('lowp', [False, True], ids=['fp32', 'lowp'])
def test_linear_function_matches_float64(lowp):
    """``LinearFunction`` on (B, I, T) = (2, 24, 19) -> O = 40: no extent is a multiple of 16, so the K and N tails of
    ``brv_gemm_f32`` (``lowp`` False) and ``brv_gemm_bf16`` (True) are hit in all three products. Output and the
    gradients with respect to input, weight and bias against the same products in float64; for ``lowp`` the operands
    of each product are rounded to bf16 first, as the kernel does (the bias and the bias gradient take no part in a
    product and stay fp32). rel-L2 <= 2e-6, the bound of the exact-fp32 product against float64 in
    test_gpu_shapes.py::test_gemm_f32_big_tiles_all_layouts; it holds for ``lowp`` unchanged because products of
    bf16 values are exact in fp32, which leaves the fp32 accumulation of at most 40 terms as the only error."""
    from brever_amd.models._ops import LinearFunction
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    dev = torch.device('cuda:0')
    B, I, O, T = 2, 24, 40, 19
    gen = torch.Generator().manual_seed(5)
    x, w, b, dy = (torch.randn(s, generator=gen) for s in ((B, I, T), (O, I), (O,), (B, O, T)))
    xd, wd, bd = (t.to(dev).requires_grad_() for t in (x, w, b))
    y = LinearFunction.apply(xd, wd, bd, lowp)
    dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), dy.to(dev))
    torch.cuda.synchronize()
    r = (lambda t: t.bfloat16().double()) if lowp else (lambda t: t.double())
    want = {'y': torch.einsum('oi,bit->bot', r(w), r(x)) + b.double()[None, :, None],
            'dx': torch.einsum('oi,bot->bit', r(w), r(dy)),
            'dw': torch.einsum('bot,bit->oi', r(dy), r(x)),
            'db': dy.double().sum((0, 2))}
    got = {'y': y, 'dx': dx, 'dw': dw, 'db': db}
    errs = {k: _rel(got[k], want[k]) for k in want}
    print('LinearFunction lowp=%s rel-L2 %s' % (lowp, errs))
    assert got['y'].dtype == got['dx'].dtype == torch.float32
    assert max(errs.values()) <= 2e-6, errs
