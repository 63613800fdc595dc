"""The general matrix-product kernels of csrc/stft.hip (gemm_f32_kernel, gemm_bf16_kernel with its vector, scalar
and column-matrix loaders, gemm32_kernel) against the float64 reference of tests/gemm_ref.py, at a few tiles.

Every case runs twice: with small integers, where every partial sum is exact in fp32 in any order, so the result must
EQUAL the reference (any mis-indexed, dropped or doubled element shows, at any reduction split), and with randn data
against the project's rel-L2 bounds. Operands sit in NaN-filled storage (NaN in the leading-dimension padding, in
front of the first and behind the last element), the result in sentinel-filled storage that must come back unchanged
outside its M x N blocks."""
import pytest
import torch

from gemm_ref import column_matrix, conv_grid, product, round_bf16, tconv_grid

pytestmark = pytest.mark.gpu

TOL_F32, TOL_BF16_F32, TOL_BF16_BF16 = 2e-6, 2e-5, 4e-3
SENTINEL = 12345.0
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
_WORST = {}                    # entry point -> largest rel-L2 / bound seen


def _embed(vals, ld, gap, front, dtype):
    """``vals`` (batch, kbatch, rows, cols) inside NaN: leading dimension ``ld``, ``gap`` NaNs between the kbatch
    and batch items, ``front`` before the first element, 8 behind the last. Returns (buffer, batch stride, kbatch
    stride); the operand starts at buffer[front]."""
    batch, kbatch, R, Cc = vals.shape
    assert ld >= Cc
    kbs = R*ld + gap
    bs = kbatch*kbs + gap
    n = front + (batch - 1)*bs + (kbatch - 1)*kbs + (R - 1)*ld + Cc + 8
    buf = torch.full((n,), float('nan'), dtype=dtype)
    buf.as_strided(vals.shape, (bs, kbs, ld, 1), front).copy_(vals)
    return buf, bs, kbs


def _splits(batch, M, N, K, kbatch, flags):
    """The dispatcher divides a reduction over workgroups (fp32 atomics) when the output has few tiles and the
    reduction 16 k-tiles or more; never for a bf16 result."""
    tiles = ((M + 127)//128)*((N + 127)//128)*batch
    return tiles < 128 and ((K + 31)//32)*kbatch >= 16 and not flags & 2


def _vector(entry, M, N, K, ta, tb, lda, ldb, gap, a_front):
    """The 16-byte loaders are taken when strides, bases and the extents along the contiguous axes are whole
    float4s (a column-matrix operand: only its pixel count matters)."""
    q4 = lambda v: v % 4 == 0                                        # noqa: E731
    ok = q4(lda) and q4(gap) and q4(a_front) and q4(M if ta else K) and q4(K if tb else N)
    return ok and (entry == 'conv' or q4(ldb))


def _run(entry, data, seed, batch, M, N, K, ta=0, tb=0, kbatch=1, lda_pad=4, ldb_pad=8, ldd_pad=3, d_gap=0, gap=4,
         a_front=4, bias=None, acc=0, flags=0, conv=None):
    """One case on the GPU, checked against the reference; returns the (batch, M, N) result on the CPU.

    entry: 'f32' | 'bf16' | 'mixed' | 'conv'. data: 'int' (exact pass) | 'randn'. conv: (mode, (C, H, W), kernel,
    stride, padding, grid) -- b is then that image's column matrix, (rows, pixels) as stored."""
    from brever_amd import hip
    lib = hip.lib()
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(seed)
    assert K*kbatch <= 2048
    lowp = entry != 'f32'

    def draw(*shape, wide=False):
        if data == 'int':
            r = 8 if wide else 4
            return torch.randint(-r, r + 1, shape, generator=gen).float()
        return torch.randn(*shape, generator=gen)

    a_dt = torch.bfloat16 if flags & 4 else torch.float32
    b_dt = torch.bfloat16 if flags & 1 else torch.float32
    d_dt = torch.bfloat16 if flags & 2 else torch.float32
    a = draw(batch, kbatch, *((K, M) if ta else (M, K))).to(a_dt)
    lda = a.shape[-1] + lda_pad
    a_buf, a_bs, a_kbs = _embed(a, lda, gap, a_front, a_dt)
    if conv:
        mode, (C, H, W), kern, stride, pad, grid = conv
        img = draw(batch, kbatch, C, H, W)
        b_buf, b_bs, b_kbs = _embed(img.reshape(batch, kbatch, 1, C*H*W), C*H*W, 5, 3, torch.float32)
        b_front, ldb = 3, 0
        b = column_matrix(round_bf16(img), mode, kern, stride, pad, grid)
        assert b.shape[-2:] == ((N, K) if tb else (K, N))
    else:
        b = draw(batch, kbatch, *((N, K) if tb else (K, N))).to(b_dt)
        ldb = b.shape[-1] + ldb_pad
        b_front = 4
        b_buf, b_bs, b_kbs = _embed(b, ldb, gap, b_front, b_dt)
    bv = draw(M if bias == 'row' else N, wide=True) if bias else None
    d0 = draw(batch, M, N, wide=True)
    ra, rb = (round_bf16(a), round_bf16(b)) if lowp else (a, b)
    want = product(ra, rb, ta, tb, bv, bias == 'col', d0 if acc else None)

    ldd = N + ldd_pad
    d_bs = M*ldd + d_gap
    d_front, guard = 4, 2*ldd + 64                         # two guard rows and more behind the last item
    d_init = torch.full((d_front + batch*d_bs + guard,), SENTINEL).to(d_dt)
    d_init.as_strided((batch, M, N), (d_bs, ldd, 1), d_front).copy_(d0)
    ad, bd = a_buf.to(dev), b_buf.to(dev)
    bvd = bv.to(dev) if bias else None
    code = 2 if bias == 'col' else acc
    outs = []
    for rep in range(2):
        d = d_init.to(dev)
        pa, pb, pd = hip.ptr(ad[a_front:]), hip.ptr(bd[b_front:]), hip.ptr(d[d_front:])
        head = (pa, pb, pd, batch, M, N, K, lda)
        tail = (a_bs, b_bs, d_bs, ta, tb, kbatch, a_kbs, b_kbs, hip.ptr(bvd), code)
        if entry == 'f32':
            st = lib.brv_gemm_f32(*head, ldb, ldd, *tail, hip.stream())
        elif entry == 'bf16':
            st = lib.brv_gemm_bf16(*head, ldb, ldd, *tail, hip.stream())
        elif entry == 'mixed':
            st = lib.brv_gemm_bf16_mixed(*head, ldb, ldd, *tail, flags, hip.stream())
        else:
            (kh, kw), (sh, sw), (ph, pw), (Ho, Wo) = kern, stride, pad, grid
            st = lib.brv_gemm_bf16_conv(*head, ldd, *tail, mode, C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo,
                                        hip.stream())
        hip.check(st, entry)
        torch.cuda.synchronize()
        outs.append(d.cpu())
    what = (entry, data, batch, M, N, K, ta, tb, kbatch, bias, acc, flags, conv and conv[:1] + conv[2:])
    full = outs[0]
    got = full.as_strided((batch, M, N), (d_bs, ldd, 1), d_front).clone()
    # nothing but the M x N blocks is written: padding columns, the gap between items, the guard behind the last
    blank, before = full.clone(), d_init.clone()
    for t in (blank, before):
        t.as_strided((batch, M, N), (d_bs, ldd, 1), d_front).zero_()
    assert torch.equal(blank, before), ('wrote outside the M x N blocks', what)
    assert bool(torch.isfinite(got.float()).all()), ('NaN / inf in the result: read outside an operand', what)
    if not _splits(batch, M, N, K, kbatch, flags):
        assert torch.equal(outs[0], outs[1]), ('not repeatable', what)
    if data == 'int':
        exact = want.float().to(d_dt)
        bad = int((got.float() != exact.float()).sum())
        assert bad == 0, ('%d of %d elements differ from the exact result' % (bad, got.numel()), what)
    else:
        rel = float((got.double() - want).norm()/want.norm())
        tol = TOL_F32 if not lowp else TOL_BF16_BF16 if flags & 2 else TOL_BF16_F32
        name = entry + ('/bf16 result' if flags & 2 else '')
        _WORST[name] = max(_WORST.get(name, 0.0), rel/tol)
        print('%-18s rel %.3e  bound %.0e  ratio %.3f  %s' % (name, rel, tol, rel/tol, what[2:]))
        assert rel <= tol, (rel, tol, what)
    return got


def _both(entry, seed, *args, **kw):
    return [_run(entry, data, seed, *args, **kw) for data in ('int', 'randn')]


def _report():
    print('largest rel-L2 / bound so far: ' + ', '.join('%s %.3f' % kv for kv in sorted(_WORST.items())))


# ---- brv_gemm_f32 below 3e7 multiply-adds: gemm_f32_kernel<TA, TB> ------------------------------------------------

@pytest.mark.parametrize('ta,tb', LAYOUTS)
def test_gemm_f32_small_products(ta, tb):
    """The 128 x 128 fp32 kernel at M = N = K = 1, one-wide rows and columns, one past a tile in every extent, odd
    leading dimensions, a batch, row / column bias and a reduction over operand pairs."""
    s = 100 + 2*ta + tb
    kw = dict(ta=ta, tb=tb, lda_pad=1, ldb_pad=1, ldd_pad=1, gap=3)
    _both('f32', s, 1, 1, 1, 1, **kw)                                                # F1
    _both('f32', s + 10, 1, 1, 130, 33, **kw)                                        # F2
    _both('f32', s + 20, 1, 129, 1, 31, **kw)                                        # F3
    odd = lambda n: 3 if n % 2 == 0 else 2                                           # noqa: E731
    _both('f32', s + 30, 3, 129, 130, 65, ta=ta, tb=tb, lda_pad=odd(129 if ta else 65),
          ldb_pad=odd(65 if tb else 130), ldd_pad=odd(130), gap=3, bias='row')       # F4: every ld odd
    _both('f32', s + 40, 2, 40, 36, 96, kbatch=3, bias='col', **kw)                  # F5
    _report()


@pytest.mark.parametrize('ta,tb', LAYOUTS)
def test_gemm_f32_split_reduction_zero_fills_and_adds_the_bias_once(ta, tb):
    """K = 1024 over one 40 x 36 tile per item: the reduction is divided over workgroups that add with atomics into a
    result the dispatcher zeroes first -- one contiguous fill (batch 1, and a batch without gaps), one per item
    (batch stride > M*N), a 2-D fill (ldd > N) -- or, accumulating, into the caller's d; the bias is added by one
    workgroup only."""
    s = 200 + 2*ta + tb
    M, N, K = 40, 36, 1024
    assert _splits(1, M, N, K, 1, 0) and _splits(3, M, N, K, 1, 0)
    kw = dict(ta=ta, tb=tb)
    _both('f32', s, 1, M, N, K, ldd_pad=0, **kw)                                     # F6a
    _both('f32', s + 10, 3, M, N, K, ldd_pad=0, **kw)                                # F6b
    _both('f32', s + 20, 3, M, N, K, ldd_pad=0, d_gap=8, **kw)                       # F6c
    _both('f32', s + 30, 2, M, N, K, ldd_pad=3, **kw)                                # F6d
    _both('f32', s + 40, 2, M, N, K, ldd_pad=3, bias='row', acc=1, **kw)             # F6e
    _both('f32', s + 50, 2, M, N, K, ldd_pad=0, bias='col', **kw)                    # column bias under atomics
    _report()


# ---- brv_gemm_bf16 / brv_gemm_bf16_mixed: gemm_bf16_kernel<TA, TB, VEC> -------------------------------------------

@pytest.mark.parametrize('ta,tb', LAYOUTS)
def test_gemm_bf16_vector_and_scalar_loaders(ta, tb):
    """B1: whole float4s everywhere with a K tail of 4 (the vector loader's k-contiguous and row-contiguous forms);
    B2: the same data with a's base one element further, which takes the scalar loader -- same LDS image, same MFMA
    order, no split, so the result is bit-identical; B3: tails everywhere, operand pairs, column bias; B4: split
    reduction, fresh and accumulating."""
    s = 300 + 2*ta + tb
    kw = dict(ta=ta, tb=tb)
    assert _vector('bf16', 132, 136, 36, ta, tb, (132 if ta else 36) + 4, (36 if tb else 136) + 8, 4, 4)
    assert not _splits(2, 132, 136, 36, 1, 0)
    b1 = _both('bf16', s, 2, 132, 136, 36, **kw)
    b2 = _both('bf16', s, 2, 132, 136, 36, a_front=5, **kw)
    for v, w, data in zip(b1, b2, ('int', 'randn')):
        assert torch.equal(v, w), ('scalar and vector loaders differ', data, ta, tb)
    b2b = _both('bf16', s, 2, 132, 136, 36, ldb_pad=9, **kw)                         # scalar through b's stride
    for v, w, data in zip(b1, b2b, ('int', 'randn')):
        assert torch.equal(v, w), ('scalar and vector loaders differ', data, ta, tb)
    _both('bf16', s + 10, 2, 130, 131, 70, kbatch=2, bias='col', lda_pad=1, ldb_pad=1, gap=3, **kw)      # B3
    assert _splits(1, 40, 36, 1024, 1, 0)
    for acc in (0, 1):                                                               # B4
        _both('bf16', s + 20 + acc, 1, 40, 36, 1024, acc=acc, **kw)
        _both('bf16', s + 22 + acc, 1, 40, 36, 1024, acc=acc, bias='row', lda_pad=1, **kw)
    _report()


@pytest.mark.parametrize('flags,ta,tb', [(1, 0, 0), (2, 0, 0), (4, 0, 0), (5, 0, 0), (3, 0, 0), (7, 0, 0),
                                         (5, 1, 1), (7, 1, 1), (5, 1, 0), (7, 0, 1)])
def test_gemm_bf16_mixed_flags(flags, ta, tb):
    """bf16 tensors in memory (bit 0: b, bit 2: a, bit 1: the result), 8-byte aligned bases and strides in
    elements: vector form with a K tail, scalar form, and the same data through both."""
    s = 400 + 16*flags + 2*ta + tb
    kw = dict(ta=ta, tb=tb, flags=flags)
    assert _vector('mixed', 72, 136, 68, ta, tb, (72 if ta else 68) + 4, (68 if tb else 136) + 8, 4, 4)
    v = _both('mixed', s, 2, 72, 136, 68, bias='row', **kw)
    w = _both('mixed', s, 2, 72, 136, 68, bias='row', a_front=5, **kw)
    for x, y, data in zip(v, w, ('int', 'randn')):
        assert torch.equal(x, y), ('scalar and vector loaders differ', data, flags, ta, tb)
    _both('mixed', s + 1, 2, 72, 136, 68, kbatch=2, bias='col', **kw)
    if flags == 7:
        _both('mixed', s + 2, 2, 70, 134, 66, lda_pad=1, ldb_pad=1, gap=3, **kw)     # B5 scalar
    if flags == 2:
        # a bf16 result is never split: few tiles and a long reduction must still repeat bit for bit (_run asserts)
        assert not _splits(1, 72, 136, 1024, 1, flags) and _splits(1, 72, 136, 1024, 1, 0)
        _both('mixed', s + 3, 1, 72, 136, 1024, **kw)
    _report()


def test_gemm_bf16_mixed_refuses_a_bf16_result_that_accumulates():
    from brever_amd import hip
    lib = hip.lib()
    dev = torch.device('cuda')
    M, N, K = 8, 8, 8
    a, b = torch.ones(M, K, device=dev), torch.ones(K, N, device=dev)
    d = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=dev)
    st = lib.brv_gemm_bf16_mixed(hip.ptr(a), hip.ptr(b), hip.ptr(d), 1, M, N, K, K, N, N, 0, 0, 0, 0, 0, 1, 0, 0,
                                 None, 1, 2, hip.stream())
    torch.cuda.synchronize()
    assert st != 0 and lib.brv_last_error()
    assert bool((d == 3.0).all())


# ---- brv_gemm_bf16_conv: the column matrix read in place (CV loaders) ---------------------------------------------

#        name       image        kernel  stride  padding output_padding
CONV = {'C1':      ((3, 16, 21), (5, 2), (2, 1), (2, 0), (1, 0)),    # DCCRN; mode-1 grid 8 x 20
        'C1odd':   ((3, 16, 22), (5, 2), (2, 1), (2, 0), (1, 0)),    # grid 8 x 21: 4-pixel groups wrap grid rows
        'C1ragged': ((3, 14, 22), (5, 2), (2, 1), (2, 0), (0, 0)),   # grids 7 x 21 and 27 x 23: odd pixel counts, scalar
        'C2':      ((5, 6, 6), (3, 3), (1, 1), (1, 1), (0, 0)),      # Wo = 6, both image edges, khw = 9
        'C3':      ((2, 8, 8), (7, 7), (1, 1), (3, 3), (0, 0)),      # khw = 49 > one k-tile
        'C4':      ((4, 8, 12), (2, 3), (2, 3), (0, 1), (0, 0))}     # sw = 3: no 16-byte path


def _conv_case(name, mode):
    size, kern, stride, pad, op = CONV[name]
    grid = conv_grid(size[1:], kern, stride, pad) if mode == 1 else tconv_grid(size[1:], kern, stride, pad, op)
    return (mode, size, kern, stride, pad, grid), size[0]*kern[0]*kern[1], grid[0]*grid[1]


def _conv_pair(seed, batch, M, N, K, conv, **kw):
    """The case through the vector column loader (float-reciprocal division, carried (c, i, j)) and, with lda one
    longer, through the scalar one (integer division per element): two index computations that must agree bit for
    bit wherever the reduction is not split. Returns whether the first run took the vector kernel."""
    ta, tb = kw.get('ta', 0), kw.get('tb', 0)
    pad = kw.pop('lda_pad', 4)
    first = _both('conv', seed, batch, M, N, K, conv=conv, lda_pad=pad, **kw)
    vec = _vector('conv', M, N, K, ta, tb, (M if ta else K) + pad, 0, 4, 4)
    if vec:
        second = _both('conv', seed, batch, M, N, K, conv=conv, lda_pad=pad + 1, **kw)
        if not _splits(batch, M, N, K, kw.get('kbatch', 1), 0):
            for v, w, data in zip(first, second, ('int', 'randn')):
                assert torch.equal(v, w), ('scalar and vector column loaders differ', data, conv, kw)
    return vec


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('name', list(CONV))
def test_gemm_bf16_conv_geometries(name, mode):
    """a @ col(image) (tb = 0: K = window rows, N = pixels) and a @ col(image)^T summed over two images (tb = 1, the
    weight-gradient form: K = pixels, N = window rows), a as stored and transposed, im2col and its gather transpose."""
    conv, rows, pix = _conv_case(name, mode)
    s = 500 + 50*list(CONV).index(name) + 10*mode
    M, nvec = 24, 0
    for ta in (0, 1):
        nvec += _conv_pair(s + ta, 1, M, pix, rows, conv, ta=ta, tb=0)
        nvec += _conv_pair(s + 2 + ta, 1, M, rows, pix, conv, ta=ta, tb=1, kbatch=2)
    if pix % 4 == 0:
        assert nvec >= 2, 'the vector column loader was not reached'
    else:
        assert nvec == 0
    _report()


def test_gemm_bf16_conv_split_reduction_over_images():
    """C5: weight-gradient form over 4 images of 256 pixels: 32 k-tiles, split with atomics over image pairs."""
    for mode in (1, 2):
        conv = (mode, (4, 16, 16), (3, 3), (1, 1), (1, 1), (16, 16))
        assert _splits(1, 24, 36, 256, 4, 0)
        for ta in (0, 1):
            _conv_pair(600 + 2*mode + ta, 1, 24, 36, 256, conv, ta=ta, tb=1, kbatch=4)
            _conv_pair(610 + 2*mode + ta, 1, 24, 36, 256, conv, ta=ta, tb=1, kbatch=4, acc=1, bias='row')
    _report()


def test_gemm_bf16_conv_bias_accumulate_and_batch_stride():
    """C6 on the column path: row bias, accumulate, a batch of images with a gap between the results."""
    for mode in (1, 2):
        c1, rows, pix = _conv_case('C1', mode)
        for ta in (0, 1):
            _conv_pair(700 + 2*mode + ta, 1, 24, pix, rows, c1, ta=ta, bias='row')
            _conv_pair(710 + 2*mode + ta, 2, 24, pix, rows, c1, ta=ta, d_gap=8, ldd_pad=0)
            _conv_pair(720 + 2*mode + ta, 2, 24, pix, rows, c1, ta=ta, d_gap=8, bias='col')
        c2, rows, pix = _conv_case('C2', mode)
        for ta in (0, 1):
            _conv_pair(730 + 2*mode + ta, 1, 24, pix, rows, c2, ta=ta, acc=1)
    _report()


def test_gemm_bf16_conv_refusals():
    from brever_amd import hip
    lib = hip.lib()
    dev = torch.device('cuda')
    C, H, W, kh, kw_, M = 2, 6, 8, 3, 3, 4
    rows, pix = C*kh*kw_, H*W
    a = torch.ones(M, rows, device=dev)
    img = torch.ones(C, H, W, device=dev)
    d = torch.full((M, pix), 3.0, device=dev)

    def call(mode, N, K, Ho, Wo):
        st = lib.brv_gemm_bf16_conv(hip.ptr(a), hip.ptr(img), hip.ptr(d), 1, M, N, K, rows, pix, 0, 0, 0, 0, 0, 1,
                                    0, 0, None, 0, mode, C, H, W, kh, kw_, 1, 1, 1, 1, Ho, Wo, hip.stream())
        torch.cuda.synchronize()
        return st
    for args in ((3, pix, rows, H, W), (0, pix, rows, H, W),        # mode
                 (1, pix, rows - 1, H, W),                          # rows != C*kh*kw
                 (1, pix, rows, H, W - 1), (2, pix - 4, rows, H, W)):   # pixels != Ho*Wo
        assert call(*args) != 0, args
        assert lib.brv_last_error(), args
        assert bool((d == 3.0).all()), args
    assert call(1, pix, rows, H, W) == 0
    assert float(d.max()) == C*kh*kw_ and float(d.min()) == C*4        # whole window inside / a corner


# ---- brv_matmul_f32: gemm32_kernel, 64 x 64 tile (mel filterbank, DCT) --------------------------------------------

@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (3, 65, 66, 33), (2, 64, 130, 31)], ids=lambda c: '%dx%dx%dx%d' % c)
@pytest.mark.parametrize('shared_a', [True, False])
def test_matmul_f32(shape, shared_a):
    """d[z] = a[z | 0] @ b[z], contiguous: one a for every item (a_batch_stride 0) or one each."""
    from brever_amd import hip
    lib = hip.lib()
    dev = torch.device('cuda')
    batch, M, N, K = shape
    for data in ('int', 'randn'):
        gen = torch.Generator().manual_seed(800 + sum(shape) + shared_a)
        draw = (lambda *s: torch.randint(-4, 5, s, generator=gen).float()) if data == 'int' else \
               (lambda *s: torch.randn(*s, generator=gen))
        a = draw(1 if shared_a else batch, 1, M, K)
        b = draw(batch, 1, K, N)
        a_buf, a_bs, _ = _embed(a, K, 0, 4, torch.float32)
        b_buf, b_bs, _ = _embed(b, N, 0, 4, torch.float32)
        assert a_bs == M*K and b_bs == K*N
        want = product(a, b, 0, 0)
        d_init = torch.full((4 + batch*M*N + 64,), SENTINEL)
        ad, bd = a_buf.to(dev), b_buf.to(dev)
        outs = []
        for rep in range(2):
            d = d_init.to(dev)
            hip.check(lib.brv_matmul_f32(hip.ptr(ad[4:]), hip.ptr(bd[4:]), hip.ptr(d[4:]), batch, M, N, K,
                                         0 if shared_a else a_bs, hip.stream()), 'brv_matmul_f32')
            torch.cuda.synchronize()
            outs.append(d.cpu())
        assert torch.equal(outs[0], outs[1])
        full = outs[0]
        assert torch.equal(full[:4], d_init[:4]) and torch.equal(full[-64:], d_init[-64:])
        got = full[4:-64].reshape(batch, M, N)
        assert bool(torch.isfinite(got).all())
        if data == 'int':
            assert torch.equal(got, want.float())
        else:
            rel = float((got.double() - want).norm()/want.norm())
            _WORST['matmul_f32'] = max(_WORST.get('matmul_f32', 0.0), rel/TOL_F32)
            print('matmul_f32 rel %.3e  bound %.0e  ratio %.3f  %s' % (rel, TOL_F32, rel/TOL_F32, shape))
            assert rel <= TOL_F32, (rel, shape)
    _report()
