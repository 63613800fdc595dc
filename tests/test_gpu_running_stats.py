"""Running statistics along time and fixed-order row sums against float64.

The kernels here keep a sum over a long axis: the FFNN's cumulative normaliser (csrc/ffnn.hip), the causal
group / layer / instance norm with its prefix and suffix scans (csrc/norm.hip), the bias-gradient sums
brv_row_sum (csrc/ffnn.hip), and the per-frame feature / label kernels next to them. Every input is drawn from a
seeded torch.Generator on the CPU, every reference is a float64 CPU computation of the same fp32 inputs, and every
bound is formed from the reference alone: what a correct fp32 kernel may lose by rounding, doubled.

Each test prints its worst error as a fraction of its bound (pytest -s shows it).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0**-23           # spacing of fp32 at 1


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()/(b.norm() + 1e-30))


def _assert_within(got, ref, bound, what):
    """No NaN / Inf, and |got - ref| <= bound per element; prints the worst error / bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, f'{what}: {bad} of {got.numel()} outputs are NaN or Inf'
    ratio = ((got - ref).abs()/bound).max().item()
    print(f'{what}: worst error / bound = {ratio:.3f}')
    assert ratio <= 1.0, f'{what}: worst error is {ratio:.3g} x the bound'
    return ratio


# ---- (a) cumulative normaliser -----------------------------------------------------------------------------------

EPS_CUM = 1e-4           # CumulativeNormalizer's default
FLOOR = -18.420681       # log(1e-8): the log of an energy floor
FAMILIES = ('normal', 'logmel', 'logmel_narrow', 'floor', 'zero', 'first_only')


def _family_rows(family, shape, g):
    """fp32 rows of one family; `lead_in` needs more than 600 frames."""
    T = shape[-1]
    if family == 'normal':
        return torch.randn(shape, generator=g)
    if family == 'logmel':
        return -8 + 2*torch.randn(shape, generator=g)
    if family == 'logmel_narrow':
        return -8 + 0.05*torch.randn(shape, generator=g)
    if family == 'floor':
        return torch.full(shape, FLOOR)
    if family == 'zero':
        return torch.zeros(shape)
    if family == 'first_only':
        x = torch.zeros(shape)
        x[..., 0] = (1 + torch.rand(shape[:-1], generator=g))*(2*torch.randint(0, 2, shape[:-1], generator=g) - 1)
        return x
    assert family == 'lead_in' and T > 600
    x = -6 + 2*torch.randn(shape, generator=g)
    x[..., :600] = FLOOR
    return x


def _cumnorm_reference(x):
    """float64 value of the fp32 input and the per-element bound 2^-23 (|m| r + 3 |y|) + 1e-7: twice what a kernel
    loses that rounds the running mean, 1/sqrt(var + eps) and the result to fp32 once each."""
    from oracle.norm import cumulative_norm
    y, m, r = cumulative_norm(x.double(), EPS_CUM, parts=True)
    assert torch.isfinite(y).all()
    return y, ULP*(m.abs()*r + 3*y.abs()) + 1e-7


def _cumnorm_direct(x2d, dev):
    """brv_cumulative_norm on a (rows, T) matrix."""
    from brever_amd import hip
    xd = x2d.to(dev).contiguous()
    out = torch.full_like(xd, float('nan'))
    hip.check(hip.lib().brv_cumulative_norm(hip.ptr(xd), hip.ptr(out), xd.shape[0], xd.shape[1], EPS_CUM,
                                            hip.stream()), 'brv_cumulative_norm')
    return out


@pytest.mark.parametrize('T', [1, 2, 37, 255, 256, 257, 2000])
@pytest.mark.parametrize('family', FAMILIES)
def test_cumulative_normalizer_equals_float64(family, T):
    """CumulativeNormalizer on (1, 1, T), (1, 5, T) and (3, 384, T) rows of one family, and brv_cumulative_norm
    itself on 1 row and on 3*384 rows (one thread, and five workgroups of one thread per row): no NaN or Inf, and
    every element within 2^-23 (|m| r + 3 |y|) + 1e-7 of the float64 value. A kernel that keeps the sums in fp32
    returns NaN on the constant rows (var = q/n - mean^2 comes out below -eps) and misses the bound wherever the
    mean is several standard deviations from zero, which log-mel features are."""
    from brever_amd.models.ffnn import CumulativeNormalizer
    dev = _cuda()
    g = torch.Generator().manual_seed(1000*FAMILIES.index(family) + T)
    norm = CumulativeNormalizer().to(dev)
    assert norm.eps == EPS_CUM
    for B, R in ((1, 1), (1, 5), (3, 384)):
        x = _family_rows(family, (B, R, T), g)
        ref, bound = _cumnorm_reference(x)
        got = norm(x.to(dev))
        _assert_within(got, ref, bound, f'module {family} ({B}, {R}, {T})')
        if R != 5:
            direct = _cumnorm_direct(x.reshape(B*R, T), dev)
            assert torch.equal(direct.view_as(got), got)


def test_cumulative_normalizer_lead_in_and_mixed_rows():
    """T = 1000: 600 constant frames (a digitally silent lead-in) followed by N(-6, 2), where the variance leaves
    zero after 600 frames of exact cancellation; and one (3, 384, 1000) tensor whose neighbouring rows belong to
    different families, so that a row reading its neighbour's sums cannot pass."""
    from brever_amd.models.ffnn import CumulativeNormalizer
    dev = _cuda()
    g = torch.Generator().manual_seed(77)
    norm = CumulativeNormalizer().to(dev)
    for B, R in ((1, 1), (1, 5), (3, 384)):
        x = _family_rows('lead_in', (B, R, 1000), g)
        ref, bound = _cumnorm_reference(x)
        _assert_within(norm(x.to(dev)), ref, bound, f'module lead_in ({B}, {R}, 1000)')
    kinds = FAMILIES + ('lead_in',)
    x = torch.stack([_family_rows(kinds[i % len(kinds)], (1000,), g) for i in range(3*384)]).view(3, 384, 1000)
    ref, bound = _cumnorm_reference(x)
    _assert_within(norm(x.to(dev)), ref, bound, 'module mixed rows (3, 384, 1000)')
    _assert_within(_cumnorm_direct(x.view(-1, 1000), dev).view(3, 384, 1000), ref, bound, 'direct mixed rows')


# ---- (b) causal group / layer / instance norm --------------------------------------------------------------------

EPS_CGN = 1e-10          # the modules' default

# (shape, groups, time_dim, mean of the input)
CGN_CASES = [((2, 6, 5, T), 2, -1, 0.0) for T in (1, 2, 255, 256, 257, 511, 513, 1000)] + [
    ((2, 6, 5, 257), 2, -1, 3.0),       # offset input: E[x^2] - E[x]^2 cancels one digit, U and 2 x V cancel in dx
    ((2, 6, 5, 1000), 2, -1, 3.0),
    ((1, 4, 300), 4, -1, 0.0),          # instance norm, R = 1, no inner dimension: frame 0 has variance exactly 0
    ((1, 4, 300), 4, -1, 3.0),
    ((3, 6, 257), 1, -1, 0.0),          # layer norm
    ((2, 6, 300, 4), 3, 2, 0.0),        # frames on axis 2: transposed copy around the kernels
    ((70, 4, 3, 40), 4, -1, 0.0),       # B*G = 280 workgroups of the scans
]


def _cgn_id(case):
    shape, groups, time_dim, mean = case
    return 'x'.join(map(str, shape)) + f'_g{groups}_t{time_dim}_m{mean:g}'


def _gain_bias(C, g):
    return 1 + 0.3*torch.randn(C, generator=g), 0.2*torch.randn(C, generator=g)


def _cgn_module(C, groups, time_dim, gain, bias, dev):
    from brever_amd.modules import CausalGroupNorm
    norm = CausalGroupNorm(C, groups, time_dim=time_dim).to(dev)
    assert norm.eps == EPS_CGN
    with torch.no_grad():
        norm.gain.copy_(gain)
        norm.bias.copy_(bias)
    return norm


def _cgn_forward_bound(x64, gain, groups, time_dim):
    """2^-23 (|m| r + 3 |y|) |gain| + 1e-7 with the running mean m, r = 1/sqrt(var + eps) and the normalised value y
    before gain and bias, all float64, from the running moments written out here (the oracle is checked against
    them on the way)."""
    from oracle.norm import causal_group_norm
    B, C = x64.shape[:2]
    t_ax = range(x64.ndim)[time_dim]
    z = x64.movedim(t_ax, -1)
    moved = z.shape
    z = z.reshape(B, groups, -1, moved[-1])
    n = z.shape[2]*torch.arange(1, moved[-1] + 1, dtype=torch.float64)
    m = (z.sum(2).cumsum(-1)/n)[:, :, None]
    var = ((z*z).sum(2).cumsum(-1)/n)[:, :, None] - m*m
    r = 1/(var + EPS_CGN).sqrt()
    y = (z - m)*r
    per_channel = [1, C] + [1]*(x64.ndim - 2)
    back = lambda a: a.expand_as(z).reshape(moved).movedim(-1, t_ax)       # noqa: E731
    y0 = causal_group_norm(x64, torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), groups,
                           time_dim, EPS_CGN)
    assert (back(y) - y0).abs().max().item() <= 1e-9*(1 + y0.abs().max().item())
    return ULP*(back(m.abs()*r) + 3*y0.abs())*gain.double().abs().view(per_channel) + 1e-7


@pytest.mark.parametrize('case', CGN_CASES, ids=_cgn_id)
def test_causal_group_norm_equals_float64(case):
    """CausalGroupNorm (groups = 1: layer norm, groups = channels: instance norm) forward and backward against
    oracle.norm.causal_group_norm on the .double() input with torch autograd. blocked_scan gives each of 256
    threads ceil(T/256) consecutive frames: T = 255, 256 one frame per thread, 257 .. 511 two (the last segments
    empty, one straddling T), 513 and 1000 three and four; T > 256 also takes a second workgroup of the frame
    sums. Forward per element within 2^-23 (|m| r + 3 |y|) |gain| + 1e-7; dx, dgain, dbias 1e-4 rel-L2."""
    from oracle.norm import causal_group_norm
    dev = _cuda()
    shape, groups, time_dim, mean = case
    C = shape[1]
    g = torch.Generator().manual_seed(sum(shape)*7 + groups + int(mean))
    x = mean + torch.randn(shape, generator=g)
    gy = torch.randn(shape, generator=g)
    gain, bias = _gain_bias(C, g)

    x64 = x.double().requires_grad_(True)
    gain64, bias64 = gain.double().requires_grad_(True), bias.double().requires_grad_(True)
    ref = causal_group_norm(x64, gain64, bias64, groups, time_dim, EPS_CGN)
    (ref*gy.double()).sum().backward()

    norm = _cgn_module(C, groups, time_dim, gain, bias, dev)
    xg = x.to(dev).requires_grad_(True)
    y = norm(xg)
    (y*gy.to(dev)).sum().backward()

    tag = _cgn_id(case)
    _assert_within(y, ref.detach(), _cgn_forward_bound(x64.detach(), gain, groups, time_dim), f'forward {tag}')
    errs = {'dx': rel(xg.grad, x64.grad), 'dgain': rel(norm.gain.grad, gain64.grad),
            'dbias': rel(norm.bias.grad, bias64.grad)}
    print(f'gradients {tag}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()) + ' (bound 1e-4)')
    for k, v in errs.items():
        assert v <= 1e-4, (tag, k, v)


@functools.lru_cache(maxsize=None)
def _causality_setup():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 6, 3, 600, generator=g)
    gy = torch.randn(2, 6, 3, 600, generator=g)
    return (x, gy) + _gain_bias(6, g)


@pytest.mark.parametrize('i', [1, 255, 256, 257, 599])
def test_causal_group_norm_is_causal_across_scan_segments(i):
    """T = 600 (three frames per scan thread, three workgroups of the frame sums). NaN written into frame i of the
    input leaves every earlier output frame finite and bit-equal to the output of the clean input; NaN written
    into frame i of the upstream gradient leaves dx finite in every later frame (a frame's statistics feed itself
    and later frames only, so the suffix scan must carry nothing backwards past a segment). The NaN does reach
    every frame it should, which shows that it was in the kernels' input at all."""
    dev = _cuda()
    x, gy, gain, bias = _causality_setup()
    norm = _cgn_module(6, 2, -1, gain, bias, dev)
    with torch.no_grad():
        clean = norm(x.to(dev))
        assert torch.isfinite(clean).all()
        xn = x.clone()
        xn[..., i] = float('nan')
        yn = norm(xn.to(dev))
    assert torch.isfinite(yn[..., :i]).all()
    assert torch.equal(yn[..., :i], clean[..., :i])
    assert torch.isnan(yn[..., i:]).all()
    xg = x.to(dev).requires_grad_(True)
    gn = gy.clone()
    gn[..., i] = float('nan')
    (norm(xg)*gn.to(dev)).sum().backward()
    assert torch.isfinite(xg.grad[..., i + 1:]).all()
    assert torch.isnan(xg.grad[..., :i + 1]).all()


@pytest.mark.parametrize('value', [0.0, FLOOR])
def test_causal_group_norm_on_constant_input(value):
    """The whole (2, 6, 5, 1000) tensor constant: var is the rounding of an exact zero next to eps = 1e-10. All
    outputs finite and within 1e-5 of the bias, all gradients finite."""
    dev = _cuda()
    g = torch.Generator().manual_seed(5)
    gain, bias = _gain_bias(6, g)
    gy = torch.randn(2, 6, 5, 1000, generator=g)
    norm = _cgn_module(6, 2, -1, gain, bias, dev)
    xg = torch.full((2, 6, 5, 1000), value).to(dev).requires_grad_(True)
    y = norm(xg)
    (y*gy.to(dev)).sum().backward()
    assert torch.isfinite(y).all()
    off = (y.detach().cpu() - bias.view(1, 6, 1, 1)).abs().max().item()
    print(f'constant {value}: max |y - bias| = {off:.3g} (bound 1e-5)')
    assert off <= 1e-5
    for grad in (xg.grad, norm.gain.grad, norm.bias.grad):
        assert torch.isfinite(grad).all()


# ---- (c) brv_row_sum ---------------------------------------------------------------------------------------------

# (B, M, T, offset of the view in its buffer)
ROW_SUM_CASES = [
    (3, 7, 100, 0), (1, 1, 1, 0), (2, 5, 8196, 0), (1, 3, 16388, 0), (1, 2, 70000, 0), (2, 5, 8197, 0),
    (2, 5, 8196, 1), (1025, 2, 20, 0), (1, 300, 20000, 0),
]


@pytest.mark.parametrize('case', ROW_SUM_CASES, ids=lambda c: 'B%d_M%d_T%d_off%d' % c)
def test_row_sum_equals_float64_on_every_path(case):
    """out[m] = sum over (b, t) of x[b][m][t], the bias gradient of FFNN, DCCRN, TF-GridNet and SGMSE+. brv_row_sum
    takes slices = min(64, ceil(B T / 16384)) and then one of three paths:

    (3, 7, 100), (1, 1, 1)    B T <= 16384, slices = 1: one launch of row_sum_kernel, result written directly.
    (2, 5, 8196)              B T = 16392, slices = 2, T % 4 == 0, B <= 1024, aligned: row_sum4_kernel with
                              pieces = ceil(T / 16384) = 1, one workgroup per (row, item).
    (1, 3, 16388)             the same path with pieces = 2: 4097 float4 split 2049 + 2048.
    (1, 2, 70000)             ceil(T / 16384) = 5, capped at pieces = 4 of 4375 float4.
    (2, 5, 8197)              T % 4 = 1: row_sum_kernel over 2 slices of 8197 elements with fp64 partials, then
                              row_sum_final_kernel.
    (2, 5, 8196) at offset 1  the pointer is 4 bytes past a 16-byte boundary: sliced generic path as well.
    (1025, 2, 20)             B > 1024 (the grid's y extent of row_sum4 is B pieces): sliced generic, the slice
                              boundary at element 10250 falls inside item 512.
    (1, 300, 20000)           row_sum4 with 300 rows: row_sum_final_kernel runs two workgroups of 256 rows.

    Values N(0.3, 1). Every case is called twice and the two results are bit-equal (fixed order, no atomics);
    |got - ref| <= 2^-23 |ref| + 2^-23 sqrt(n) rms(x), n = B T: fp64 accumulation rounded to fp32 once, with the
    pairwise fp32 add of four neighbours inside row_sum4 (three roundings of 2^-24 |partial| per four elements,
    adding up like a random walk) allowed for."""
    from brever_amd import hip
    dev = _cuda()
    B, M, T, offset = case
    g = torch.Generator().manual_seed(B + 10*M + T + offset)
    x = 0.3 + torch.randn(B, M, T, generator=g)
    buf = torch.zeros(B*M*T + offset, device=dev)
    view = buf[offset:].view(B, M, T)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4*offset and view.is_contiguous()
    outs = []
    for _ in range(2):
        out = torch.full((M,), float('nan'), device=dev)
        hip.check(hip.lib().brv_row_sum(hip.ptr(view), hip.ptr(out), B, M, T, hip.stream()), 'brv_row_sum')
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    x64 = x.double()
    ref = x64.sum((0, 2))
    rms = (x64*x64).mean((0, 2)).sqrt()
    bound = ULP*ref.abs() + ULP*(B*T)**0.5*rms
    _assert_within(outs[0], ref, bound, 'row_sum B%d M%d T%d off%d' % case)


# ---- (d) per-frame feature and label kernels ---------------------------------------------------------------------

def _assert_ulps(got, ref, ulps, what):
    """|got - ref| <= ulps units in the last place of the fp32 reference."""
    got, ref = got.cpu(), ref.cpu()
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape, what
    assert torch.isfinite(got).all(), what
    spacing = torch.ldexp(torch.ones_like(ref, dtype=torch.float64), torch.frexp(ref)[1] - 24)
    spacing = torch.where(ref == 0, 2.0**-149, spacing.clamp_min(2.0**-149))
    worst = ((got.double() - ref.double()).abs()/spacing).max().item()
    assert worst <= ulps, f'{what}: {worst} ulp'


@pytest.mark.parametrize('T', [1, 2, 3, 50])
@pytest.mark.parametrize('B', [1, 3])
def test_frame_kernels_equal_their_restatements(B, T):
    """brv_stack_frames, brv_deltas, brv_static_norm, brv_irm, brv_col_normalize and brv_masked_mean_spec away from
    the golden's shape, against the same fp32 expression in torch on the CPU: 7 rows, B = 1 and 3 (the row index
    arithmetic), T = 1, 2, 3 (the t < 1 and t < 2 zeros of the deltas, the clamp to frame 0 of the stacking with
    stacks = 5 >= T) and 50. The copies (stacking, rows 0..M of the deltas) bit for bit, the arithmetic to 4 ulp."""
    from brever_amd import hip
    dev = _cuda()
    lib = hip.lib()
    M = 7
    g = torch.Generator().manual_seed(100*B + T)
    x = torch.randn(B, M, T, generator=g)
    xd = x.to(dev)

    for stacks in (0, 5):
        out = torch.full((B, (stacks + 1)*M, T), float('nan'), device=dev)
        hip.check(lib.brv_stack_frames(hip.ptr(xd), hip.ptr(out), B, M, T, stacks, hip.stream()), 'brv_stack_frames')
        frames = torch.arange(T)
        ref = torch.cat([x[..., (frames - k).clamp_min(0)] for k in range(stacks + 1)], 1)
        assert torch.equal(out.cpu(), ref), f'stack_frames stacks={stacks}'

    out = torch.full((B, 3*M, T), float('nan'), device=dev)
    hip.check(lib.brv_deltas(hip.ptr(xd), hip.ptr(out), B, M, T, hip.stream()), 'brv_deltas')
    d1, d2 = torch.zeros_like(x), torch.zeros_like(x)
    d1[..., 1:] = x[..., 1:] - x[..., :-1]
    d2[..., 2:] = x[..., 2:] - 2*x[..., 1:-1] + x[..., :-2]
    assert torch.equal(out[:, :M].cpu(), x)
    _assert_ulps(out[:, M:].cpu(), torch.cat([d1, d2], 1), 4, 'deltas')
    assert not out[:, M:, :1].any() and not out[:, 2*M:, :2].any()

    mean, std = torch.randn(M, 1, generator=g), 0.5 + torch.rand(M, 1, generator=g)
    out = torch.full_like(xd, float('nan'))
    mean_d, std_d = mean.to(dev), std.to(dev)           # named, so that both stay allocated until the launch
    hip.check(lib.brv_static_norm(hip.ptr(xd), hip.ptr(mean_d), hip.ptr(std_d), hip.ptr(out), B, M, T,
                                  hip.stream()), 'brv_static_norm')
    _assert_ulps(out, (x - mean)/std, 4, 'static_norm')

    fg, bg = torch.rand(B, M, T, generator=g)**4, torch.rand(B, M, T, generator=g)**4
    eps = 2.0**-52
    out = torch.full_like(xd, float('nan'))
    fg_d, bg_d = fg.to(dev), bg.to(dev)
    hip.check(lib.brv_irm(hip.ptr(fg_d), hip.ptr(bg_d), hip.ptr(out), B*M*T, eps, hip.stream()), 'brv_irm')
    _assert_ulps(out, 1/torch.sqrt(1 + bg/(fg + eps)), 4, 'irm')

    p = torch.rand(B, M, T, generator=g) + 0.01
    out = p.to(dev)
    hip.check(lib.brv_col_normalize(hip.ptr(out), B, M, T, 1e-7, hip.stream()), 'brv_col_normalize')
    total = torch.zeros(B, T)
    for m in range(M):                  # the kernel's order of the M additions
        total = total + p[:, m]
    _assert_ulps(out, p*(1/(total + 1e-7))[:, None], 4, 'col_normalize')

    C, bins = 2, 5
    spec = torch.randn(B, C, bins, T, 2, generator=g)
    mask = torch.rand(B, bins, T, generator=g)
    out = torch.full((B, bins, T, 2), float('nan'), device=dev)
    spec_d, mask_d = spec.to(dev), mask.to(dev)
    hip.check(lib.brv_masked_mean_spec(hip.ptr(spec_d), hip.ptr(mask_d), hip.ptr(out), B, C, bins*T, hip.stream()),
              'brv_masked_mean_spec')
    _assert_ulps(out, (spec[:, 0] + spec[:, 1])*(mask/C)[..., None], 4, 'masked_mean_spec')
