"""Test infrastructure (never imported by the product): a differentiable restatement of ``oracle/stoi.py`` in
torch, fp64 by default, operation by operation -- ``resample_poly`` as upfirdn, Hann frames, the 40 dB frame
selection, overlap-add, a 512-point rfft, one-third octave bands, 30-frame segments, both correlation forms.

Only ``processed`` is differentiated: frame selection and everything computed from ``clean`` are constants. Two
conventions go beyond the oracle's values, both about derivatives: ``sqrt`` has derivative 0 at 0 (band
magnitudes, segment norms, row and column norms), and STOI's clip passes the gradient to the scaled estimate
where it is not above the bound and nowhere else.

Also here: the signal recipe and the cases of the criteria's tests, and the per-frame energies the threshold
clearance condition is checked on.
"""
import numpy as np
import torch

from oracle import stoi as O

# (fs, n): the shapes of the GPU tests; kept / all frames and the closest frame to the 40 dB threshold are
# recorded in tests/test_stoi_loss_host.py
BATCH_FS, BATCH_LENGTHS = 16000, (24000, 17777, 16000, 6000)
SINGLE_CASES = ((8000, 12000), (10000, 16000))
ZERO_STRETCH = (5000, 9000)                       # at 10 kHz, n = 16000


def signals(fs, n):
    """``(target, estimate)`` float64 arrays of the tests' recipe: coloured noise with gaps, plus white noise."""
    from scipy.signal import lfilter
    t = np.arange(n)/fs
    env = (np.sin(2*np.pi*3*t) > -0.3)*(0.5 + 0.5*np.sin(2*np.pi*1.3*t))
    target = lfilter([1], [1, -1.3, 0.6], np.random.default_rng(1).standard_normal(n))*env*0.05
    estimate = target + 0.03*np.random.default_rng(2).standard_normal(n)
    return target, estimate


def sqrt0(s):
    """``sqrt`` whose derivative at 0 is 0."""
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def norm0(x, dim):
    return sqrt0((x*x).sum(dim=dim, keepdim=True))


def resample(x, fs):
    """``oracle.stoi.resample_oct(x, 10000, fs)``: scipy's ``resample_poly`` with the given window, as upfirdn
    ``y[m] = sum_i h[(m + n_pre_remove) down - i up] x[i]`` on the pre-padded filter."""
    g = np.gcd(O.FS, fs)
    up, down = O.FS//g, fs//g
    h = O.resample_filter(up, down)
    h = h/np.sum(h)*up
    half = (len(h) - 1)//2
    n_pre_pad = down - half % down
    hpad = np.concatenate([np.zeros(n_pre_pad), h])
    n_pre_remove = (half + n_pre_pad)//down
    n = x.shape[0]
    n_out = -(-n*up//down)
    c = (np.arange(n_out) + n_pre_remove)*down                      # filter index = c - i up
    taps = -(-len(hpad)//up) + 1
    i = (c//up)[:, None] - np.arange(taps)[None, :]                 # descending from the last i with c - i up >= 0
    k = c[:, None] - i*up
    ok = (i >= 0) & (i < n) & (k >= 0) & (k < len(hpad))
    w = torch.as_tensor(np.where(ok, hpad[np.clip(k, 0, len(hpad) - 1)], 0.0), dtype=x.dtype)
    return (w*x[torch.as_tensor(np.clip(i, 0, n - 1))]).sum(1)


def frames(x):
    """The Hann frames of ``oracle.stoi._frames``: ``len(range(0, len(x) - 256, 128))`` of them."""
    nf = len(range(0, x.shape[0] - O.N_FRAME, O.N_FRAME//2))
    w = torch.as_tensor(np.hanning(O.N_FRAME + 2)[1:-1], dtype=x.dtype)
    if nf == 0:
        return x.new_zeros(0, O.N_FRAME)
    return x.unfold(0, O.N_FRAME, O.N_FRAME//2)[:nf]*w


def frame_energies(clean, fs):
    """fp64 energies (dB) of the clean frames at 10 kHz: what the frame selection compares."""
    x = torch.as_tensor(np.asarray(clean, dtype=np.float64))
    if fs != O.FS:
        x = resample(x, fs)
    xf = frames(x)
    return (20*torch.log10(xf.norm(dim=1) + O.EPS)).numpy()


def overlap_add(fr):
    k = fr.shape[0]
    hop = O.N_FRAME//2
    out = fr.new_zeros(O.N_FRAME + (k - 1)*hop if k > 0 else 0)
    if k > 0:
        idx = (torch.arange(k)[:, None]*hop + torch.arange(O.N_FRAME)[None, :]).reshape(-1)
        out = out.index_add(0, idx, fr.reshape(-1))
    return out


def band_spectrogram(x, obm):
    spec = torch.fft.rfft(frames(x), n=O.NFFT)                      # (frames, bins)
    power = spec.real**2 + spec.imag**2
    return sqrt0(obm @ power.T)                                     # (bands, frames)


def row_col_normalize(s):
    s = s - s.mean(dim=2, keepdim=True)
    s = s/(norm0(s, 2) + O.EPS)
    s = s - s.mean(dim=1, keepdim=True)
    return s/(norm0(s, 1) + O.EPS)


def stoi(clean, processed, fs, extended, dtype=torch.float64):
    """STOI / ESTOI of ``processed`` against ``clean`` (1-D, equal length) as a 0-d tensor of ``dtype``,
    differentiable in ``processed`` when that is a tensor that requires grad."""
    x = torch.as_tensor(clean).detach().to(dtype)
    y = torch.as_tensor(processed).to(dtype)
    if x.shape != y.shape:
        raise ValueError('clean and processed must have the same shape')
    if fs != O.FS:
        x, y = resample(x, fs), resample(y, fs)
    xf, yf = frames(x), frames(y)
    if xf.shape[0] == 0:
        return y.sum()*0 + 1e-5
    energies = 20*torch.log10(xf.norm(dim=1) + O.EPS)
    keep = (energies.max() - O.DYN_RANGE - energies) < 0
    x, y = overlap_add(xf[keep]), overlap_add(yf[keep])
    if x.shape[0] <= O.N_FRAME:
        return y.sum()*0 + 1e-5
    obm = torch.as_tensor(O.third_octave_matrix()[0], dtype=dtype)
    xb, yb = band_spectrogram(x, obm), band_spectrogram(y, obm)
    if xb.shape[1] < O.N:
        return y.sum()*0 + 1e-5
    xs = xb.unfold(1, O.N, 1).permute(1, 0, 2)                      # (segments, bands, 30)
    ys = yb.unfold(1, O.N, 1).permute(1, 0, 2)
    if extended:
        return (row_col_normalize(xs)*row_col_normalize(ys)/O.N).sum()/xs.shape[0]
    scale = norm0(xs, 2)/(norm0(ys, 2) + O.EPS)
    u, v = ys*scale, xs*(1 + 10**(-O.BETA/20))
    yp = torch.where(u <= v, u, v.detach())
    yp = yp - yp.mean(dim=2, keepdim=True)
    xs = xs - xs.mean(dim=2, keepdim=True)
    yp = yp/(norm0(yp, 2) + O.EPS)
    xs = xs/(norm0(xs, 2) + O.EPS)
    return (yp*xs).sum()/(xs.shape[0]*xs.shape[1])


def value_and_grad(clean, processed, fs, extended, dtype=torch.float64):
    """``(value, d value/d processed)`` as a float and a float64 array."""
    y = torch.as_tensor(np.asarray(processed)).to(dtype).requires_grad_(True)
    d = stoi(clean, y, fs, extended, dtype)
    g, = torch.autograd.grad(d, y)
    return float(d.detach()), g.double().numpy()
