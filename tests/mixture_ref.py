"""NumPy restatement (float64) of the reference's ``Mixture`` recipe, the yardstick of the mixture tests.

Written from the behaviour recorded in tests/golden/mixture.npz (tests/test_mixture_host.py holds it to that
fixture at 1e-12): split_brir with its max_itd peak correction, spatialisation truncated to the input length,
padding before and again after it, energies of the channel mean, and the order add_speech, add_noises, diffuse
sum, set_ndr, set_snr over speech_idx, set_tmr, set_rms(get_rms() + jitter)."""
import os

import numpy as np

COMPONENTS = ('mixture', 'foreground', 'background', 'speech', 'noise', 'early_speech', 'late_speech',
              'dir_noise', 'diffuse')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mixture.npz')


def split_brir(brir, boundary=800, max_delay=16):
    mag = np.abs(brir)
    peak = np.argmax(mag, axis=0)
    strong = 0 if mag[peak[0], 0] > mag[peak[1], 1] else 1
    weak = 1 - strong
    peak[weak] = peak[strong] + np.argmax(mag[peak[strong]:peak[strong] + max_delay, weak])
    early = brir.copy()
    for ear in range(2):
        early[peak[ear] + boundary:, ear] = 0
    return early, brir - early


def spatialize(x, brir):
    return np.stack([np.convolve(x, brir[:, ear])[:len(x)] for ear in range(2)], axis=1)


def energy(x, sl=slice(None)):
    return float(np.sum(x[sl].mean(axis=1)**2))


def snr_gain(signal, noise, snr, sl=slice(None)):
    es, en = energy(signal, sl), energy(noise, sl)
    if es == 0:
        raise ValueError('cannot scale noise signal if target signal is 0')
    if en == 0:
        raise ValueError('cannot scale noise signal if it equals 0')
    return (10**(-snr/10)*es/en)**0.5


def mixture(target, brir, noises=(), noise_brirs=(), diffuse=(), diffuse_brirs=(), padding=0.0, ndr=None,
            snr=None, tmr=None, rms_jitter=0.0, fs=16000):
    """Returns (components dict of (frames, 2) float64, gains [ndr, snr, tmr, rms], labels [tmr, tnr, trr],
    speech_idx)."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)                      # noqa: E731
    n_pad = round(padding*fs)
    idx = (n_pad, n_pad + len(target))
    he, hl = split_brir(f64(brir), round(50e-3*fs), round(1e-3*fs))
    x = np.pad(f64(target), n_pad)
    early = np.pad(spatialize(x, he), ((n_pad, n_pad), (0, 0)))
    late = np.pad(spatialize(x, hl), ((n_pad, n_pad), (0, 0)))
    dirn, diff = np.zeros(early.shape), np.zeros(early.shape)
    for xn, hn in zip(noises, noise_brirs):
        dirn = dirn + spatialize(f64(xn), f64(hn))
    for xn, hn in zip(diffuse, diffuse_brirs):
        diff = diff + spatialize(f64(xn), f64(hn))
    g = [1.0, 1.0, 1.0, 1.0]
    sl = slice(*idx)
    if ndr is not None:
        g[0] = snr_gain(dirn, diff, ndr)
        diff = g[0]*diff
    if snr is not None:
        g[1] = snr_gain(early, late + dirn + diff, snr, sl)
        dirn, diff = g[1]*dirn, g[1]*diff
    if tmr is not None:
        g[2] = (energy(early)*(1/tmr - 1)/energy(late + dirn + diff))**0.5
        late, dirn, diff = g[2]*late, g[2]*dirn, g[2]*diff
    mix = (early + late) + (dirn + diff)
    rms_max = (np.mean(mix**2, axis=0)**0.5).max()
    g[3] = 10**((20*np.log10(rms_max) + rms_jitter)/20)/rms_max
    early, late, dirn, diff = g[3]*early, g[3]*late, g[3]*dirn, g[3]*diff
    comp = derive(early, late, dirn, diff)
    et = energy(early, sl)
    labels = [et/(et + energy(m, sl)) for m in (comp['background'], comp['noise'], late)]
    return comp, g, labels, idx


def derive(early, late, dirn, diff):
    """All nine components from the four stored ones, by Mixture's own properties."""
    noise = dirn + diff
    speech = early + late
    return dict(mixture=speech + noise, foreground=early, background=late + noise, speech=speech, noise=noise,
                early_speech=early, late_speech=late, dir_noise=dirn, diffuse=diff)


def golden_cases():
    """The cases of tests/golden/mixture.npz: dicts with the inputs (float32 arrays), ``kwargs`` for ``mixture``
    above, and the recorded ``components`` (all nine, float64), ``gains``, ``labels``, ``speech_idx``,
    ``length`` and ``f32err`` (name -> the float32 direct convolution's rel-L2 error)."""
    z = np.load(GOLDEN)
    assert tuple(z['components']) == COMPONENTS
    out = []
    i = 0
    while f'c{i}_target' in z.files:
        k = f'c{i}_'
        nn, nd = (int(v) for v in z[k + 'counts'])
        padding, ndr, snr, tmr, jitter = (float(v) for v in z[k + 'params'])
        opt = lambda v: None if np.isnan(v) else v                      # noqa: E731
        T = int(z[k + 'length'])
        stored = [z[k + n] if k + n in z.files else np.zeros((T, 2))
                  for n in ('early_speech', 'late_speech', 'dir_noise', 'diffuse')]
        out.append(dict(
            target=z[k + 'target'], brir=z[k + 'brir'],
            noises=[z[f'{k}noise{j}'] for j in range(nn)], noise_brirs=[z[f'{k}noise_brir{j}'] for j in range(nn)],
            diffuse=[z[f'{k}diffuse_in{j}'] for j in range(nd)],
            diffuse_brirs=[z[f'{k}diffuse_brir{j}'] for j in range(nd)],
            kwargs=dict(padding=padding, ndr=opt(ndr), snr=opt(snr), tmr=opt(tmr), rms_jitter=jitter),
            components=derive(*stored), gains=z[k + 'gains'], labels=z[k + 'labels'],
            speech_idx=tuple(int(v) for v in z[k + 'speech_idx']), length=T,
            f32err=dict(zip(COMPONENTS, (float(v) for v in z[k + 'f32err'])))))
        i += 1
    return out


def run_case(c):
    return mixture(c['target'], c['brir'], c['noises'], c['noise_brirs'], c['diffuse'], c['diffuse_brirs'],
                   **c['kwargs'])
