"""NumPy restatement (float64) of the reference's signal effects, the yardstick of the mixture-effects tests:
``colored_noise`` on a given white row, ``match_ltas``, ``calc_ltas`` and ``BRIRDecay`` on a given tail noise.

Written from the behaviour recorded in tests/golden/mixture_fx.npz (tests/test_mixture_fx_host.py holds it to
that fixture at 1e-12). Also: the loader of that fixture and the small pool behind tests/golden/pool_draws.json."""
import os

import numpy as np

import mixture_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'mixture_fx.npz')
DRAWS = os.path.join(HERE, 'golden', 'pool_draws.json')
ALPHA = dict(brown=2, pink=1, white=0, blue=-1, violet=-2)
N_FFT, HOP = 512, 256


def color_scaling(color, m):
    """s_k = f_k^(-alpha/2) on the one-sided bins of a length-m transform, f_k = k/m, s_0 := s_1."""
    f = np.arange(m//2 + 1)/m
    f[0] = f[1]
    return f**(-ALPHA[color]/2)


def colorize(x, color):
    x = np.asarray(x, dtype=np.float64)
    return np.fft.irfft(np.fft.rfft(x)*color_scaling(color, len(x)), len(x))


def window():
    return 0.5 - 0.5*np.cos(2*np.pi*np.arange(N_FFT)/N_FFT)          # periodic Hann


def stft(x):
    """x (n, channels) -> X (bins, channels, frames): 256 zeros in front, zero fill behind, ceil(n/256) + 1
    frames, the spectrum divided by the window sum."""
    n, w = len(x), window()
    frames = -(-n//HOP) + 1
    padded = np.zeros((HOP*(frames + 1), x.shape[1]))
    padded[HOP:HOP + n] = x
    seg = np.stack([padded[HOP*t:HOP*t + N_FFT] for t in range(frames)], axis=-1)      # (512, channels, frames)
    return np.fft.rfft(seg*w[:, None, None], axis=0)/w.sum()


def match_ltas(x, ltas):
    x = np.asarray(x, dtype=np.float64)
    if len(x) < N_FFT:
        raise ValueError(f'match_ltas needs at least {N_FFT} samples, got {len(x)}')
    flat = x.ndim == 1
    x2 = x.reshape(len(x), -1)
    n, w = len(x2), window()
    X = stft(x2)
    power = np.mean(np.abs(X)**2, axis=(1, 2))
    X = X*np.sqrt(ltas/power)[:, None, None]
    seg = np.fft.irfft(X, N_FFT, axis=0)*w[:, None, None]*w.sum()
    frames = X.shape[-1]
    y, env = np.zeros((HOP*(frames + 1), x2.shape[1])), np.zeros(HOP*(frames + 1))
    for t in range(frames):
        y[HOP*t:HOP*t + N_FFT] += seg[..., t]
        env[HOP*t:HOP*t + N_FFT] += w**2
    y = y/np.where(env > 1e-10, env, 1.0)[:, None]
    y = y[HOP:HOP + n]
    return y.ravel() if flat else y


def smooth_ltas(ltas, n_oct=3):
    """The reference's 1/3-octave Gaussian smoothing of bins 1.. (its normalisation divides COLUMN j by the sum
    of ROW j, and its width is that of the column's bin; both kept)."""
    f = np.arange(1, len(ltas))
    sigma = (f/n_oct)/np.pi
    g = np.exp(-0.5*(np.subtract.outer(f, f)/sigma)**2)/(sigma*(2*np.pi)**0.5)
    g = g/g.sum(axis=1)
    out = np.array(ltas, dtype=np.float64)
    out[1:] = g@out[1:]
    return out


def calc_ltas(files):
    ltas = np.zeros(N_FFT//2 + 1)
    for x in files:
        X = stft(np.asarray(x, dtype=np.float64).reshape(-1, 1))
        ltas += np.mean(np.abs(X)**2, axis=(1, 2))
    return smooth_ltas(ltas)


def decay_length(taps, rt60, delay, fs=16000):
    return max(int(round(2*(rt60 + delay)*fs)), taps)


def brir_decay(brir, noise, rt60, drr, delay, fs=16000):
    """``noise``: the white (or coloured) tail noise, at least n - i0 samples; returns (decayed BRIR, i0)."""
    brir = np.asarray(brir, dtype=np.float64)
    if rt60 == 0:
        return brir, None
    n = decay_length(len(brir), rt60, delay, fs)
    i0 = int(round(delay*fs)) + int(min(np.argmax(np.abs(brir), axis=0)))
    padded = np.zeros((n, 2))
    padded[:len(brir)] = brir
    tail = np.zeros((n, 2))
    t = np.arange(n - i0).reshape(-1, 1)/fs
    tail[i0:] = np.exp(-t/rt60*3*np.log(10))*np.asarray(noise, dtype=np.float64)[:n - i0].reshape(-1, 1)
    return padded + mixture_ref.snr_gain(padded, tail, drr)*tail, i0


def golden():
    return np.load(GOLDEN)


def draw_pool():
    """The fixed small pool whose draws tests/golden/pool_draws.json records."""
    rng = np.random.default_rng(7)
    speech = [rng.standard_normal(n).astype(np.float32) for n in (900, 1300, 1100, 777)]
    noises = [rng.standard_normal(n).astype(np.float32) for n in (2000, 1500, 400)]
    brirs = [[rng.standard_normal((300, 2)).astype(np.float32) for _ in range(3)],
             [rng.standard_normal((257, 2)).astype(np.float32) for _ in range(2)]]
    return dict(speech=speech, noises=noises, brirs=brirs)


# the two configurations of pool_draws.json: every option at its default; the parent commit's options all on
DRAW_CONFIGS = dict(default=dict(seed=3), parent_options=dict(seed=5, padding=0.005, diffuse=True,
                                                              rms_jitter=(-3.0, 3.0), noise_count=(1, 3)))


def whole_cases():
    """The whole mixtures of the fixture: inputs (float32), what the reference was asked for, and the recorded
    ``components`` (all nine, float64), ``gains``, ``labels``, ``speech_idx``, ``length``, ``f32err``."""
    z = golden()
    ltas, out, i = z['calc_ltas'], [], 0
    while f'w{i}_target' in z.files:
        k = f'w{i}_'
        nn, nd, eq = (int(v) for v in z[k + 'counts'])
        padding, ndr, snr, tmr, jitter = (float(v) for v in z[k + 'params'])
        opt = lambda v: None if np.isnan(v) else v                      # noqa: E731
        T = int(z[k + 'length'])
        stored = [z[k + n] if k + n in z.files else np.zeros((T, 2))
                  for n in ('early_speech', 'late_speech', 'dir_noise', 'diffuse')]
        out.append(dict(
            target=z[k + 'target'], brir=z[k + 'brir'], noise_types=[str(t) for t in z[k + 'noise_types']],
            noises=[z[f'{k}noise{j}'] for j in range(nn)], noise_brirs=[z[f'{k}noise_brir{j}'] for j in range(nn)],
            diffuse=[z[f'{k}diffuse_in{j}'] for j in range(nd)],
            diffuse_brirs=[z[f'{k}diffuse_brir{j}'] for j in range(nd)],
            tails=[z[f'{k}tail{j}'] for j in range(1 + nn)], decay=tuple(float(v) for v in z[k + 'decay']),
            diffuse_color=str(z[k + 'diffuse_color']), ltas_eq=bool(eq), ltas=ltas,
            kwargs=dict(padding=padding, ndr=opt(ndr), snr=opt(snr), tmr=opt(tmr), rms_jitter=jitter),
            components=mixture_ref.derive(*stored), gains=z[k + 'gains'], labels=z[k + 'labels'],
            speech_idx=tuple(int(v) for v in z[k + 'speech_idx']), length=T,
            f32err=dict(zip(mixture_ref.COMPONENTS, (float(v) for v in z[k + 'f32err'])))))
        i += 1
    return out


def run_whole(c, fs=16000):
    """The reference's make_from_metadata order on a case of ``whole_cases``: decayed BRIRs for the target and the
    directional noises, synthetic noises coloured or matched, the diffuse sum coloured and matched, then the
    level steps of ``mixture_ref.mixture``. Returns what that returns."""
    from mixture_ref import derive, energy, snr_gain, spatialize, split_brir
    rt60, drr, delay = c['decay']
    kw = c['kwargs']
    n_pad = round(kw['padding']*fs)
    idx = (n_pad, n_pad + len(c['target']))
    brir = brir_decay(c['brir'], c['tails'][0], rt60, drr, delay, fs)[0]
    he, hl = split_brir(brir, round(50e-3*fs), round(1e-3*fs))
    x = np.pad(np.asarray(c['target'], dtype=np.float64), n_pad)
    early = np.pad(spatialize(x, he), ((n_pad, n_pad), (0, 0)))
    late = np.pad(spatialize(x, hl), ((n_pad, n_pad), (0, 0)))
    dirn, diff = np.zeros(early.shape), np.zeros(early.shape)
    for kind, xn, hn, tail in zip(c['noise_types'], c['noises'], c['noise_brirs'], c['tails'][1:]):
        xn = np.asarray(xn, dtype=np.float64)
        if kind == 'ssn':
            xn = match_ltas(xn, c['ltas'])
        elif kind != 'file':
            xn = colorize(xn, kind[len('colored_'):])
        dirn = dirn + spatialize(xn, brir_decay(hn, tail, rt60, drr, delay, fs)[0])
    for xn, hn in zip(c['diffuse'], c['diffuse_brirs']):
        diff = diff + spatialize(colorize(xn, c['diffuse_color']), np.asarray(hn, dtype=np.float64))
    if c['ltas_eq'] and c['diffuse']:
        diff = match_ltas(diff, c['ltas'])
    g, sl = [1.0, 1.0, 1.0, 1.0], slice(*idx)
    if kw['ndr'] is not None:
        g[0] = snr_gain(dirn, diff, kw['ndr'])
        diff = g[0]*diff
    if kw['snr'] is not None:
        g[1] = snr_gain(early, late + dirn + diff, kw['snr'], sl)
        dirn, diff = g[1]*dirn, g[1]*diff
    if kw['tmr'] is not None:
        g[2] = (energy(early)*(1/kw['tmr'] - 1)/energy(late + dirn + diff))**0.5
        late, dirn, diff = g[2]*late, g[2]*dirn, g[2]*diff
    mix = (early + late) + (dirn + diff)
    rms_max = (np.mean(mix**2, axis=0)**0.5).max()
    g[3] = 10**((20*np.log10(rms_max) + kw['rms_jitter'])/20)/rms_max
    early, late, dirn, diff = g[3]*early, g[3]*late, g[3]*dirn, g[3]*diff
    comp = derive(early, late, dirn, diff)
    et = energy(early, sl)
    labels = [et/(et + energy(m, sl)) for m in (comp['background'], comp['noise'], late)]
    return comp, g, labels, idx
