"""NumPy restatement of the GPU FLAC encoder's decision rule without LPC, brute force over the stated
search space; never the code under test. ``min_frame_bytes`` is the length of the shortest frame the search space
holds for a block: header, subframes, padding and both CRCs.

Search space: per coded channel CONSTANT (all samples equal), VERBATIM, FIXED of order 0 ... 4 with order < block
size; residuals in partitioned Rice code, partition orders 0 ... 4 where the block divides and every partition keeps a
residual, per partition any parameter 0 ... 14 with 4-bit parameters or 0 ... 30 with 5-bit ones; stereo as
independent, left/side, side/right or mid/side. The minimum over all of it is what the encoder has to reach; which
of several equally short codings it writes (its order of ties) does not change the length.
"""
import numpy as np

MAX_PORDER = 4
BLOCK_CODES = {192: 1, **{576 << k: 2 + k for k in range(4)}, **{256 << k: 8 + k for k in range(8)}}
FIXED = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]]


def quantise(x, bps):
    """The encoder's rule for float samples: clip(rint(x 2^(bps-1))), round half to even, in float64."""
    full = 2.0**(bps - 1)
    return np.clip(np.rint(np.asarray(x, dtype=np.float64)*full), -full, full - 1).astype(np.int64)


def number_bytes(number):
    """Bytes of the frame number in the UTF-8-like coding."""
    if number < 0x80:
        return 1
    return 1 + next(e for e in range(1, 7) if number < 1 << (5*e + 6))


def header_bits(block, rate, number):
    extra = 0 if block in BLOCK_CODES else 8 if block <= 256 else 16
    return 8*(4 + number_bytes(number) + 1) + extra          # rates without a code come "from STREAMINFO"


def rice_bits(res, block, order):
    """Fewest bits of the residual section (method, partition order, parameters, codes)."""
    res = np.asarray(res, dtype=np.int64)
    u = np.where(res >= 0, 2*res, -2*res - 1)
    best = None
    for porder in range(MAX_PORDER + 1):
        if block % (1 << porder) or (block >> porder) <= order:
            break
        size = block >> porder
        for pbits, kmax in ((4, 14), (5, 30)):
            total = 0
            for part in range(1 << porder):
                lo, hi = max(part*size - order, 0), (part + 1)*size - order
                chunk = u[lo:hi]
                total += pbits + min(int((chunk >> k).sum()) + len(chunk)*(k + 1) for k in range(kmax + 1))
            best = total if best is None else min(best, total)
    return 2 + 4 + best


def subframe_bits(x, width):
    """(bits, kind) of the shortest subframe of the samples ``x``, ``width`` bits each; kind is 'constant',
    'verbatim' or 'fixedN'. Ties go to the earlier of that list."""
    x = np.asarray(x, dtype=np.int64)
    n = len(x)
    cands = [(8 + n*width, 'verbatim')]
    if (x == x[0]).all():
        cands.insert(0, (8 + width, 'constant'))
    for order in range(5):
        if order >= n:
            break
        res = x[order:].copy()
        for j, c in enumerate(FIXED[order]):
            res -= c*x[order - 1 - j:n - 1 - j]
        cands.append((8 + order*width + rice_bits(res, n, order), f'fixed{order}'))
    return min(cands, key=lambda c: c[0])


def frame_choice(block_samples, bps, rate=16000, number=0):
    """``block_samples``: int array (channels, n). Returns (bytes of the shortest frame, channel assignment code,
    the kinds of its subframes)."""
    x = np.asarray(block_samples, dtype=np.int64)
    channels, n = x.shape
    if channels == 1:
        bits, kind = subframe_bits(x[0], bps)
        body, assignment, kinds = bits, 0, [kind]
    else:
        left, right = x
        sub = dict(l=subframe_bits(left, bps), r=subframe_bits(right, bps),
                   m=subframe_bits((left + right) >> 1, bps), s=subframe_bits(left - right, bps + 1))
        options = [(1, 'l', 'r'), (8, 'l', 's'), (9, 's', 'r'), (10, 'm', 's')]
        assignment, a, b = min(options, key=lambda o: sub[o[1]][0] + sub[o[2]][0])
        body, kinds = sub[a][0] + sub[b][0], [sub[a][1], sub[b][1]]
    bits = header_bits(n, rate, number) + body
    return (bits + 7)//8 + 2, assignment, kinds


def min_frame_bytes(block_samples, bps, rate=16000, number=0):
    return frame_choice(block_samples, bps, rate, number)[0]


def stream_frame_bytes(pcm, bps, block, rate=16000):
    """Per frame of the stream of ``pcm`` (channels, n): (bytes, assignment, kinds)."""
    pcm = np.asarray(pcm, dtype=np.int64)
    return [frame_choice(pcm[:, s:s + block], bps, rate, k) for k, s in enumerate(range(0, pcm.shape[1], block))]


def decision_blocks(bps, n, seed):
    """Seeded stereo blocks (2, n) that make every subframe kind and every channel assignment win somewhere, and
    two shorter ones at the end."""
    rng = np.random.default_rng(seed)
    full = 2**(bps - 1)
    walk = rng.integers(-40, 41, n).cumsum()
    smooth = rng.integers(-3, 4, n).cumsum().cumsum()
    noise = rng.integers(-full, full, n)
    other = rng.integers(-300, 300, n)
    ramp = 5*np.arange(n) - 90
    clip = lambda v: np.clip(v, -full, full - 1)               # noqa: E731
    blocks = [np.stack([clip(a), clip(b)]) for a, b in (
        (walk, other), (walk, walk + rng.integers(-2, 3, n)), (walk + rng.integers(-2, 3, n), walk),
        (walk + other, walk - other), (noise, rng.integers(-full, full, n)), (np.full(n, 77), np.zeros(n, dtype=np.int64)),
        (ramp, smooth), (rng.integers(-3, 4, n), rng.integers(-1, 2, n)), (noise, noise), (noise, clip(-noise)),
        (1000 + rng.integers(-20, 21, n), np.full(n, 1000)))]
    return blocks + [b[:, :n - 3] for b in blocks[:2]]
