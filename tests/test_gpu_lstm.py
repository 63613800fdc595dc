"""Every LSTM recurrence kernel, called directly through its entry point and named by the variant it runs, against the
float64 restatement of tests/lstm_ref.py (itself held to nn.LSTM by tests/test_lstm_ref_host.py):

  brv_lstm_recurrent_forward / _backward         lstm_fwd/bwd_quad_kernel (H = 128), lstm_fwd/bwd_reg_kernel (H <= 128,
                                                 H % 16 == 0), lstm_recurrent_kernel / lstm_bwd_kernel (any other H)
  brv_lstm_recurrent_forward_bf16 / _backward_   lstm_fwd/bwd_mv_kernel
  brv_lstm_tile_forward / _backward              variant 0: lstm_tile_fwd/bwd_kernel, 1: lstm_tile_*_bf16_kernel<IO16>,
                                                 2: lstm_q4_*_kernel<IO16> -- every tile case first asserts that
                                                 brv_lstm_tile_variant names the variant the case is about

The backward kernels run on saved activations and cell states made by the REFERENCE, so the two directions fail
independently. Every forward variant is also run without saved activations (act == cs == NULL) and a second time:
both give bit-identical hidden states. Every output sits between two guard bands of a sentinel that must come back
untouched.

Tolerances (rel-L2):
  fp32 kernels against the unrounded reference: y, act, cs 1e-5, dgates 1e-4 (test_lstm_kernels_match_torch's).
  bf16-operand kernels, tensors stored as fp32, against the reference that rounds the same operands: 2e-4
    (test_lstm_bf16_matrix_pipe_recurrence_matches_rounded_operand_loop's).
  bf16-STORED tensors (act and dgates at lowp == 2), where one rounding flip is 2^-8 of an element:
    (a) against the reference before storage rounding: 2^-8 + 2e-4 (round to nearest costs at most 2^-8 per element);
    (b) at most 1 % of the elements differ in their bf16 bits from the rounded reference;
    (c) rel-L2 against the rounded reference: at most four times what the float32 restatement of the reference with
        the kernels' forms of sigmoid / tanh (lstm_ref ``dtype=float32, fast=True``) differs from the float64 one AT
        THE CASE'S OWN SHAPE (the kernels' exp / rcp are about 1 ulp each where libm is under 1), never below 2e-4.
        The yardstick is computed on the CPU with the case, never from the kernels' output. Over the cases of this
        file it is 0 .. 1.5e-4 (few elements: a single flip or none), so the bound is 2e-4 .. 5.9e-4; the largest
        distances the kernels themselves showed on an MI355X: lstm_q4_* act 2.9e-5 (yardstick of that case 3.5e-5),
        dgates 6.8e-5 (5.4e-5); lstm_tile_*_bf16 act 3.1e-5 (2.7e-5), dgates 2.8e-5 (3.1e-5); at most 0.1 % of the
        bf16 patterns differed (condition (b) allows 1 %).
"""
import functools

import pytest
import torch

import lstm_ref
from lstm_ref import rel

pytestmark = pytest.mark.gpu

H128 = 128
GUARD = 1024                    # elements of sentinel on either side of every output
SENTINEL = -4096.0              # exact in bf16; no LSTM quantity of these inputs comes near it
TOL_F32, TOL_F32_GRAD, TOL_BF16_OPERANDS = 1e-5, 1e-4, 2e-4
TOL_BF16_STORED = 2.0**-8 + TOL_BF16_OPERANDS
MAX_FLIPPED = 0.01


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda:0')


def _lib():
    from brever_amd import hip
    return hip


class _Checks:
    """Print every figure, then fail once with all that missed their bound."""

    def __init__(self, case):
        self.case, self.missed = case, []

    def hold(self, what, value, bound):
        print(f'{self.case}: {what} = {value:.3e} (bound {bound:.3e})')
        if not value <= bound:
            self.missed.append((what, value, bound))

    def true(self, what, ok):
        if not ok:
            print(f'{self.case}: {what} FAILED')
            self.missed.append((what,))

    def done(self):
        assert not self.missed, (self.case, self.missed)


@functools.lru_cache(maxsize=8)
def _inputs(B, T, H, groups, io16):
    """N(0, 1) gate inputs and output gradients, W_hh ~ N(0, 1/H), bias 0.1 N(0, 1): float32 values as the kernels
    get them (``io16``: gate inputs representable in bf16), torch's gate order."""
    gen = torch.Generator().manual_seed(1000003*B + 1009*T + 31*H + groups)
    gates = torch.randn(B, T, 4*H, generator=gen)
    if io16:
        gates = lstm_ref.round_bf16(gates)
    w_hh = torch.randn(groups, 4*H, H, generator=gen)/H**0.5
    bias = 0.1*torch.randn(groups, 4*H, generator=gen)
    dy = torch.randn(B, T, H, generator=gen)
    return gates, w_hh, bias, dy


@functools.lru_cache(maxsize=8)
def _reference(B, T, H, groups, mask, rounded, io16):
    """The float64 reference of one case, computed once and never modified: forward, then backward FROM the saved
    tensors as the kernel will read them (the forward's, as float32 / bf16). With ``io16`` also the float32
    restatement's distance for condition (c)."""
    gates, w_hh, bias, dy = _inputs(B, T, H, groups, io16)
    kw = dict(groups=groups, reverse_mask=mask, round_operands=rounded)
    y, act, cs = lstm_ref.forward(gates, w_hh, bias, io16=io16, **kw)
    ref = dict(y=y, act=act, cs=cs)
    ref['act_fed'] = act.float()            # (io16: already representable in bf16)
    ref['cs_fed'] = cs.float()
    dg = lstm_ref.backward(ref['act_fed'], ref['cs_fed'], w_hh, dy, io16=io16, **kw)
    if io16:
        ref['dgates_unrounded'], ref['dgates'] = dg
        ref['act_unrounded'] = lstm_ref.forward(gates, w_hh, bias, **kw)[1]
        _, act32, _ = lstm_ref.forward(gates, w_hh, bias, io16=True, dtype=torch.float32, fast=True, **kw)
        _, dg32 = lstm_ref.backward(ref['act_fed'], ref['cs_fed'], w_hh, dy, io16=True, dtype=torch.float32, fast=True,
                                    **kw)
        ref['act_yardstick'], ref['dgates_yardstick'] = rel(act32, act), rel(dg32, ref['dgates'])
    else:
        ref['dgates'] = dg
    for v in ref.values():
        if torch.is_tensor(v):
            v.requires_grad_(False)
    return ref


def _guarded(n, dtype, dev):
    buf = torch.full((n + 2*GUARD,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    b = buf.cpu().float()
    return bool((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all())


def _written(view):
    """No element of the output proper still holds the sentinel."""
    return not bool((view.cpu().float() == SENTINEL).any())


def _identical(chk, what, buf, first):
    """Bit-identical buffers (guard bands included); on a miss, how many elements differ and by how much."""
    same = torch.equal(buf, first)
    if not same:
        d = (buf.double() - first.double()).abs()
        print(f'{chk.case}: {what}: {int((buf != first).sum())} of {buf.numel()} elements differ, '
              f'max |difference| {float(d.max()):.3e}')
    chk.true(what, same)


def _stored_bf16(chk, what, got, rounded_ref, unrounded_ref, yardstick, case):
    """Conditions (a), (b), (c) of the module docstring on a tensor the kernel stores as bf16."""
    assert got.dtype == torch.bfloat16
    chk.hold(f'{what} (a) vs unrounded', rel(got, unrounded_ref), TOL_BF16_STORED)
    want16 = rounded_ref.to(torch.bfloat16)
    assert torch.equal(want16.double(), rounded_ref.double())
    flipped = float((got.view(torch.int16) != want16.view(torch.int16)).double().mean())
    chk.hold(f'{what} (b) share of differing bf16 patterns', flipped, MAX_FLIPPED)
    print(f'{case}: {what} float32-restatement yardstick = {yardstick:.3e}')
    chk.hold(f'{what} (c) vs rounded', rel(got, rounded_ref), max(TOL_BF16_OPERANDS, 4*yardstick))


# ---- brv_lstm_tile_* -------------------------------------------------------------------------------------------------
def _tile_case(variant, per, T, groups, mask, strided, lowp):
    hip = _lib()
    lib, dev = hip.lib(), _cuda()
    H, B = H128, per*groups
    case = f'tile v{variant} lowp{lowp} per{per} T{T} G{groups} mask{mask:#b} {"strided" if strided else "plain"}'
    assert lib.brv_lstm_tile_supported(H)
    assert lib.brv_lstm_tile_variant(B, groups, lowp) == variant, \
        (case, 'runs variant', lib.brv_lstm_tile_variant(B, groups, lowp))
    io16, rounded = lowp == 2, lowp != 0
    io = torch.bfloat16 if io16 else torch.float32
    gates, w_hh, bias, dy = _inputs(B, T, H, groups, io16)
    ref = _reference(B, T, H, groups, mask, rounded, io16)
    ld, goff = (groups*H, H) if strided else (H, per*T*H)
    idx = lstm_ref.y_index(B, T, H, groups, ld, goff)
    chk = _Checks(case)
    tol_y = TOL_BF16_OPERANDS if rounded else TOL_F32
    tol_g = TOL_BF16_OPERANDS if rounded else TOL_F32_GRAD

    gates_d = lstm_ref.interleave(gates).to(io).to(dev)
    w_d, b_d = w_hh.to(dev), bias.to(dev)

    def forward(saved):
        y_buf, y = _guarded(B*T*H, torch.float32, dev)
        a_buf, a = _guarded(B*T*4*H, io, dev)
        c_buf, c = _guarded(B*T*H, torch.float32, dev)
        hip.call('brv_lstm_tile_forward', gates_d, w_d, b_d, y, a if saved else None, c if saved else None, B, T, H,
                 groups, mask, ld, goff, lowp, hip.stream())
        torch.cuda.synchronize()
        return (y_buf, y), (a_buf, a), (c_buf, c)

    (y_buf, y), (a_buf, a), (c_buf, c) = forward(True)
    for name, buf, view in (('y', y_buf, y), ('act', a_buf, a), ('cs', c_buf, c)):
        chk.true(f'{name} guard bands', _guards_intact(buf))
        chk.true(f'{name} fully written', _written(view))
    y_got = y.cpu()[idx]
    act_got = lstm_ref.deinterleave(a.cpu().view(B, T, 4*H))
    chk.hold('y', rel(y_got, ref['y']), tol_y)
    chk.hold('cs', rel(c.cpu().view(B, T, H), ref['cs']), tol_y)
    if io16:
        _stored_bf16(chk, 'act', act_got, ref['act'], ref['act_unrounded'], ref['act_yardstick'], case)
    else:
        chk.hold('act', rel(act_got, ref['act']), tol_y)
    (y2_buf, y2), _, _ = forward(True)
    _identical(chk, 'second run bit-identical', y2_buf, y_buf)
    (y3_buf, y3), (a3_buf, _), (c3_buf, _) = forward(False)
    chk.hold('act == NULL: y', rel(y3.cpu()[idx], ref['y']), tol_y)
    _identical(chk, 'act == NULL: bit-identical y', y3_buf, y_buf)
    chk.true('act == NULL: act / cs untouched',
             bool((a3_buf == SENTINEL).all()) and bool((c3_buf == SENTINEL).all()))

    # backward on the reference's saved tensors
    act_d = lstm_ref.interleave(ref['act_fed']).to(io).to(dev)
    cs_d = ref['cs_fed'].to(dev)
    dy_d = lstm_ref.place_y(dy, groups, ld, goff).to(dev)
    assert dy_d.numel() == B*T*H
    g_buf, g = _guarded(B*T*4*H, io, dev)
    hip.call('brv_lstm_tile_backward', act_d, cs_d, w_d, dy_d, g, B, T, H, groups, mask, ld, goff, lowp, hip.stream())
    torch.cuda.synchronize()
    chk.true('dgates guard bands', _guards_intact(g_buf))
    chk.true('dgates fully written', _written(g))
    dg_got = lstm_ref.deinterleave(g.cpu().view(B, T, 4*H))
    if io16:
        _stored_bf16(chk, 'dgates', dg_got, ref['dgates'], ref['dgates_unrounded'], ref['dgates_yardstick'], case)
    else:
        chk.hold('dgates', rel(dg_got, ref['dgates']), tol_g)
    g2_buf, g2 = _guarded(B*T*4*H, io, dev)
    hip.call('brv_lstm_tile_backward', act_d, cs_d, w_d, dy_d, g2, B, T, H, groups, mask, ld, goff, lowp, hip.stream())
    torch.cuda.synchronize()
    _identical(chk, 'backward: second run bit-identical', g2_buf, g_buf)
    chk.done()


#              chains per group, T, groups, reverse_mask, strided
TILE_F32 = [(1, 1, 1, 0, False), (15, 2, 1, 0b101, False), (16, 9, 1, 0, False), (17, 1, 1, 0, False),
            (37, 9, 1, 0, False), (1, 9, 3, 0b010, False), (15, 1, 3, 0, True), (16, 2, 3, 0b101, False),
            (17, 9, 3, 0b010, True), (37, 2, 3, 0b101, True)]
# around the three-ahead prologue (T <= 3) and the four-way rotation of the register sets (T = 4, 5, 9)
Q4 = [(1, 1, 1, 0, False), (3, 2, 1, 0, False), (4, 3, 1, 0, False), (5, 4, 1, 0, False), (37, 5, 1, 0, False),
      (5, 9, 1, 0b101, False), (1, 2, 3, 0b010, True), (3, 3, 3, 0b101, False), (3, 4, 3, 0, True),
      (5, 1, 3, 0b010, True), (37, 9, 3, 0b101, True)]


@pytest.mark.parametrize('per,T,groups,mask,strided', TILE_F32)
def test_tile_fp32_kernels(per, T, groups, mask, strided):
    """lstm_tile_fwd_kernel / lstm_tile_bwd_kernel (variant 0: 16 chains per workgroup, exact fp32 MFMA): fewer chains
    than a tile, a full tile, a tail tile of one and of five, T below and above the double buffer, three groups with
    the middle or the outer ones reversed, both output layouts."""
    _tile_case(0, per, T, groups, mask, strided, 0)


@pytest.mark.parametrize('lowp', [1, 2])
@pytest.mark.parametrize('per,T,groups,mask,strided', Q4)
def test_q4_kernels(per, T, groups, mask, strided, lowp):
    """lstm_q4_fwd_kernel / lstm_q4_bwd_kernel<IO16> (variant 2: 4 chains per workgroup, bf16 MFMA; IO16 = lowp 2)
    against the reference that rounds the same operands. T = 1, 2, 3: the prologue's clamped fetches; T = 4, 5, 9: the
    rotation. Condition (c) at lowp 2: the float32-restatement yardstick of these cases is at most 1.5e-4 (act, 5 chains
    x 9 steps) and 8.4e-6 (dgates) at one group, 3.5e-5 / 5.4e-5 at 3 x 37 chains x 9 steps; measured on the kernels:
    act at most 2.9e-5, dgates at most 6.8e-5 (bound there 2.2e-4)."""
    _tile_case(2, per, T, groups, mask, strided, lowp)


def _smallest_variant_1(groups, lowp):
    """The smallest chain count per group at which the library takes the 16-chain bf16 kernels: by its rule (0.72
    rounds of 4-chain workgroups >= 2.4 rounds of 16-chain ones) 12 CUs + 1 chains in all, the last tile holding
    one live chain."""
    lib = _lib().lib()
    cus = torch.cuda.get_device_properties(_cuda()).multi_processor_count
    for per in range(1, 20*cus//groups + 1):
        if lib.brv_lstm_tile_variant(per*groups, groups, lowp) == 1:
            return per
    pytest.fail(f'no chain count up to 20 x {cus} CUs takes variant 1 (groups {groups}, lowp {lowp}): '
                'lstm_tile_fwd_bf16_kernel / lstm_tile_bwd_bf16_kernel are dead code')


@pytest.mark.parametrize('lowp', [1, 2])
@pytest.mark.parametrize('T,groups,mask,strided', [(1, 1, 0, False), (3, 1, 0, False), (3, 2, 2, True)])
def test_tile_bf16_kernels(T, groups, mask, strided, lowp):
    """lstm_tile_fwd_bf16_kernel / lstm_tile_bwd_bf16_kernel<IO16> (variant 1), reached at the smallest chain count
    the library's own rule sends there (3073 on 256 CUs; 1537 per group with two groups): a tail tile with ONE live
    chain. Condition (c) at lowp 2: yardstick at most 2.7e-5 (act) and 3.2e-5 (dgates), so the bound is its floor of
    2e-4; measured on the kernels: act at most 3.1e-5, dgates at most 2.8e-5."""
    per = _smallest_variant_1(groups, lowp)
    cus = torch.cuda.get_device_properties(_cuda()).multi_processor_count
    print(f'variant 1 from {per} chains per group ({groups} groups) on {cus} CUs')
    if groups == 1:
        assert per == 12*cus + 1, (per, cus)
    _tile_case(1, per, T, groups, mask, strided, lowp)


# ---- brv_lstm_recurrent_* (one chain per workgroup, torch's gate order, plain layout) --------------------------------
def _recurrent_case(kernel, H, per, T, groups, bf16):
    hip = _lib()
    dev = _cuda()
    B = per*groups
    case = f'{kernel} H{H} per{per} T{T} G{groups}'
    fwd = 'brv_lstm_recurrent_forward' + ('_bf16' if bf16 else '')
    bwd = 'brv_lstm_recurrent_backward' + ('_bf16' if bf16 else '')
    if bf16:
        assert hip.lib().brv_lstm_recurrent_bf16_supported(H)
    gates, w_hh, bias, dy = _inputs(B, T, H, groups, False)
    ref = _reference(B, T, H, groups, 0, bf16, False)
    chk = _Checks(case)
    tol_y = TOL_BF16_OPERANDS if bf16 else TOL_F32
    tol_g = TOL_BF16_OPERANDS if bf16 else TOL_F32_GRAD
    gates_d, w_d, b_d = gates.to(dev), w_hh.to(dev), bias.to(dev)

    def forward(saved):
        y_buf, y = _guarded(B*T*H, torch.float32, dev)
        a_buf, a = _guarded(B*T*4*H, torch.float32, dev)
        c_buf, c = _guarded(B*T*H, torch.float32, dev)
        hip.call(fwd, gates_d, w_d, b_d, y, a if saved else None, c if saved else None, B, T, H, groups, hip.stream())
        torch.cuda.synchronize()
        return (y_buf, y), (a_buf, a), (c_buf, c)

    (y_buf, y), (a_buf, a), (c_buf, c) = forward(True)
    for name, buf, view in (('y', y_buf, y), ('act', a_buf, a), ('cs', c_buf, c)):
        chk.true(f'{name} guard bands', _guards_intact(buf))
        chk.true(f'{name} fully written', _written(view))
    chk.hold('y', rel(y.cpu().view(B, T, H), ref['y']), tol_y)
    chk.hold('act', rel(a.cpu().view(B, T, 4*H), ref['act']), tol_y)
    chk.hold('cs', rel(c.cpu().view(B, T, H), ref['cs']), tol_y)
    (y2_buf, _), _, _ = forward(True)
    _identical(chk, 'second run bit-identical', y2_buf, y_buf)
    (y3_buf, y3), (a3_buf, _), (c3_buf, _) = forward(False)
    chk.hold('act == NULL: y', rel(y3.cpu().view(B, T, H), ref['y']), tol_y)
    _identical(chk, 'act == NULL: bit-identical y', y3_buf, y_buf)
    chk.true('act == NULL: act / cs untouched',
             bool((a3_buf == SENTINEL).all()) and bool((c3_buf == SENTINEL).all()))

    act_d, cs_d, dy_d = ref['act_fed'].to(dev), ref['cs_fed'].to(dev), dy.to(dev)
    g_buf, g = _guarded(B*T*4*H, torch.float32, dev)
    hip.call(bwd, act_d, cs_d, w_d, dy_d, g, B, T, H, groups, hip.stream())
    torch.cuda.synchronize()
    chk.true('dgates guard bands', _guards_intact(g_buf))
    chk.true('dgates fully written', _written(g))
    chk.hold('dgates', rel(g.cpu().view(B, T, 4*H), ref['dgates']), tol_g)
    g2_buf, g2 = _guarded(B*T*4*H, torch.float32, dev)
    hip.call(bwd, act_d, cs_d, w_d, dy_d, g2, B, T, H, groups, hip.stream())
    torch.cuda.synchronize()
    _identical(chk, 'backward: second run bit-identical', g2_buf, g_buf)
    chk.done()


# ring of 8 slots filled 4 steps ahead: T below the prefetch distance, at it, around the ring depth, two laps
RING = [(1, 1, 1), (3, 3, 1), (4, 1, 2), (5, 3, 2), (8, 1, 1), (9, 3, 1), (17, 1, 2)]


@pytest.mark.parametrize('T,per,groups', RING)
def test_quad_kernels(T, per, groups):
    """lstm_fwd_quad_kernel<HAS_ACT> / lstm_bwd_quad_kernel (H = 128, fp32; the backward reads its saved tensors
    through the 8-slot LDS-DMA ring)."""
    _recurrent_case('quad', 128, per, T, groups, False)


@pytest.mark.parametrize('T,per,groups', RING)
def test_mv_kernels(T, per, groups):
    """lstm_fwd_mv_kernel<HAS_ACT> / lstm_bwd_mv_kernel (H = 128, bf16 MFMA, the same ring in both directions) against
    the reference that rounds the same operands."""
    _recurrent_case('mv', 128, per, T, groups, True)


@pytest.mark.parametrize('H,T', [(16, 1), (16, 37), (32, 2), (32, 3), (112, 1), (112, 37)])
def test_reg_kernels(H, T):
    """lstm_fwd_reg_kernel / lstm_bwd_reg_kernel (H <= 128, H % 16 == 0: one wavefront at H = 16, seven at 112; the
    backward loads two steps ahead), two groups of three chains."""
    _recurrent_case('reg', H, 3, T, 2, False)


@pytest.mark.parametrize('H,T', [(24, 1), (24, 37), (136, 1), (136, 37), (264, 1), (264, 37)])
def test_generic_kernels(H, T):
    """lstm_recurrent_kernel / lstm_bwd_kernel (any other H: not a multiple of 16, just above 128, more units than the
    256 threads of a workgroup), two groups of three chains."""
    _recurrent_case('generic', H, 3, T, 2, False)


# ---- the autograd wrappers at their edges ---------------------------------------------------------------------------
def _grads_close(chk, named_got, named_want, tol):
    for (name, got), want in zip(named_got, named_want):
        chk.hold(f'd{name}', rel(got, want), tol)


def _rounded_projection(x, w_ih):
    """gates_in as brv_gemm_bf16 forms it: both operands rounded to bf16, summed exactly (float64 here)."""
    return lstm_ref.round_bf16(x).double() @ lstm_ref.round_bf16(w_ih).double().t()


@pytest.mark.parametrize('use_amp', [False, True])
@pytest.mark.parametrize('S', [1, 2])
def test_bilstm_wrapper_at_one_and_two_steps(S, use_amp):
    """``_bilstm`` (``_BiLSTMFn``: two groups of one launch, the second reversed, strided output), 130 chains, S = 1
    (dw_hh is zeros, no shifted-view product) and S = 2 (that product with a reduction length of one per chain).
    fp32 against CPU nn.LSTM: y 1e-5, every gradient 1e-4. use_amp (bf16 gate inputs and saved activations,
    lstm_q4_*<true>): y, stored as fp32, within 2e-4 of lstm_ref on the bf16-rounded input projection; dw_hh is
    exactly zero at S = 1 either way."""
    from brever_amd.models._ops import amp
    from brever_amd.models.tfgridnet import _bilstm
    import copy
    hip = _lib()
    dev = _cuda()
    torch.manual_seed(40 + S)
    N, I, H = 130, 8, H128
    assert hip.lib().brv_lstm_tile_variant(2*N, 2, 2 if use_amp else 0) == (2 if use_amp else 0)
    ref = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True)
    x = torch.randn(N, S, I, requires_grad=True)
    gy = torch.randn(N, S, 2*H)
    y, _ = ref(x)
    y.backward(gy)
    dut = copy.deepcopy(ref).to(dev)
    dut.zero_grad()
    xd = x.detach().to(dev).requires_grad_(True)
    with amp(use_amp):
        yd = _bilstm(xd, dut)
        yd.backward(gy.to(dev))
    torch.cuda.synchronize()
    chk = _Checks(f'_bilstm S{S} amp{int(use_amp)}')
    if not use_amp:
        chk.hold('y', rel(yd, y.detach()), TOL_F32)
        chk.hold('dx', rel(xd.grad, x.grad), TOL_F32_GRAD)
        _grads_close(chk, ((n, q.grad) for (n, _), q in zip(ref.named_parameters(), dut.parameters())),
                     (p.grad for p in ref.parameters()), TOL_F32_GRAD)
    else:
        sfx = ('', '_reverse')
        w_ih = [getattr(ref, 'weight_ih_l0' + s).detach() for s in sfx]
        # (the projection is STORED as bf16 here)
        gates = torch.cat([lstm_ref.round_bf16(_rounded_projection(x.detach(), w)) for w in w_ih])
        w_hh = torch.stack([getattr(ref, 'weight_hh_l0' + s).detach() for s in sfx])
        bias = torch.stack([(getattr(ref, 'bias_ih_l0' + s) + getattr(ref, 'bias_hh_l0' + s)).detach() for s in sfx])
        want, _, _ = lstm_ref.forward(gates, w_hh, bias, groups=2, reverse_mask=2, round_operands=True)
        chk.hold('y vs rounded reference', rel(yd.cpu().double(), lstm_ref.place_y(want, 2, 2*H, H).view(N, S, 2*H)),
                 TOL_BF16_OPERANDS)
        chk.true('y moved by the rounding', rel(yd, y.detach()) > 0)
        for q in list(dut.parameters()) + [xd]:
            chk.true('finite gradient', bool(torch.isfinite(q.grad).all()))
    if S == 1:
        for s in ('', '_reverse'):
            chk.true('dw_hh exactly zero', int(torch.count_nonzero(getattr(dut, 'weight_hh_l0' + s).grad)) == 0)
    chk.done()


@pytest.mark.parametrize('use_amp', [False, True])
@pytest.mark.parametrize('B,T', [(127, 1), (127, 2), (128, 1), (128, 2)])
def test_lstm_function_on_both_sides_of_the_tile_threshold(B, T, use_amp):
    """``LSTMFunction`` with two groups of 127 chains (254 < TILE_MIN_CHAINS: the quad kernels, or the mv kernels
    under use_amp) and of 128 (256: lstm_tile_* variant 0, or lstm_q4_*<false> under use_amp), T = 1 (dw_hh is zeros)
    and T = 2 (the shifted-view product with one frame per chain). fp32 against CPU nn.LSTM: y 1e-5, every gradient
    1e-4; use_amp: y within 2e-4 of lstm_ref on the rounded-operand input projection."""
    from brever_amd.models._ops import LSTMFunction, amp
    hip = _lib()
    dev = _cuda()
    torch.manual_seed(100*B + T)
    G, I, H = 2, 8, H128
    tiled = G*B >= (LSTMFunction.TILE_MIN_CHAINS_LOWP if use_amp else LSTMFunction.TILE_MIN_CHAINS)
    assert tiled == (B == 128)
    if tiled:
        assert hip.lib().brv_lstm_tile_variant(G*B, G, int(use_amp)) == (2 if use_amp else 0)
    names = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')
    refs = [torch.nn.LSTM(I, H, batch_first=True) for _ in range(G)]
    xs = [torch.randn(B, T, I, requires_grad=True) for _ in range(G)]
    gy = torch.randn(G, B, T, H)
    ys = []
    for m, x, g in zip(refs, xs, gy):
        y, _ = m(x)
        y.backward(g)
        ys.append(y.detach())
    xd = torch.stack([x.detach() for x in xs]).to(dev).requires_grad_(True)
    pd = [torch.stack([getattr(m, n).detach() for m in refs]).to(dev).requires_grad_(True) for n in names]
    with amp(use_amp):
        yd = LSTMFunction.apply(xd, *pd)
        yd.backward(gy.to(dev))
    torch.cuda.synchronize()
    chk = _Checks(f'LSTMFunction B{B} T{T} amp{int(use_amp)}')
    if not use_amp:
        for g in range(G):
            chk.hold(f'y[{g}]', rel(yd[g], ys[g]), TOL_F32)
            chk.hold(f'dx[{g}]', rel(xd.grad[g], xs[g].grad), TOL_F32_GRAD)
            _grads_close(chk, ((f'{n}[{g}]', p.grad[g]) for n, p in zip(names, pd)),
                         (getattr(refs[g], n).grad for n in names), TOL_F32_GRAD)
    else:
        gates = torch.cat([_rounded_projection(xs[g].detach(), refs[g].weight_ih_l0.detach()) for g in range(G)])
        w_hh = torch.stack([m.weight_hh_l0.detach() for m in refs])
        bias = torch.stack([(m.bias_ih_l0 + m.bias_hh_l0).detach() for m in refs])
        want, _, _ = lstm_ref.forward(gates, w_hh, bias, groups=G, round_operands=True)
        chk.hold('y vs rounded reference', rel(yd.cpu().view(G*B, T, H), want), TOL_BF16_OPERANDS)
        chk.true('y moved by the rounding', rel(yd.cpu().view(G*B, T, H), torch.cat(ys)) > 0)
        for q in pd + [xd]:
            chk.true('finite gradient', bool(torch.isfinite(q.grad).all()))
    if T == 1:
        chk.true('dw_hh exactly zero', int(torch.count_nonzero(pd[1].grad)) == 0)
    chk.done()
