"""Generate tests/golden/mixture_fx.npz from the *imported reference*: ``colored_noise``, ``match_ltas``,
``AudioFileLoader.calc_ltas``, ``BRIRDecay`` and two whole mixtures in ``make_from_metadata`` order.

Runs only where the reference checkout is mounted (``BREVER_REFERENCE``, default /root/reference); nothing of the
reference is copied -- the fixture holds seeded float32 inputs and recorded outputs. The stand-ins of
make_golden_mixture.py for ``sofa`` and ``soundfile`` are used again.

    python tests/golden/make_golden_mixture_fx.py

The reference draws its white noise inside ``colored_noise`` from ``np.random.RandomState(seed).randn(n)``; the
draws are injected by putting a stand-in for ``RandomState`` in place that hands out the recorded float32 rows
(a longer row is cut to the ``n`` asked for: a white sequence's prefix). ``sf.read`` and ``get_speech_files``
are stubbed for ``calc_ltas``.

Beside every output ``<key>`` lies ``<key>_f32err``: the rel-L2 error against the float64 reference of a CPU
float32 restatement of the same step -- colouring as a float32 linear convolution of the periodic extension
with the float32 filter, ``match_ltas`` with float32 frames, spectra and overlap-add, the decay with a float32
tail and sum, the mixtures from those and float32 direct convolutions with the reference's gains. This is the
yardstick the GPU test scales its bounds from.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden_mixture import COMPONENTS, FS, load_reference, make_brir          # noqa: E402
import mixture_fx_ref as R                                                           # noqa: E402

f32, f64 = np.float32, np.float64
COLORS = ('brown', 'pink', 'blue', 'violet')


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, f64) - b)/np.linalg.norm(b))


class Draws:
    """Stands in for ``np.random.RandomState``: ``RandomState(seed).randn(n)`` hands out the next queued row."""

    def __init__(self, rows):
        self.rows = list(rows)

    def __call__(self, seed=None):
        return self

    def randn(self, n):
        x = self.rows.pop(0)
        assert len(x) >= n, (len(x), n)
        return np.asarray(x[:n], f64)


def with_draws(rows, fn):
    keep, draws = np.random.RandomState, Draws(rows)
    np.random.RandomState = draws
    try:
        out = fn()
    finally:
        np.random.RandomState = keep
    assert not draws.rows, 'a queued draw was not taken'
    return out


# -- float32 restatements ------------------------------------------------------------------------------------------
def colorize32(x, color):
    m = len(x)
    h = np.fft.irfft(R.color_scaling(color, m), m).astype(f32)
    xx = np.concatenate([x, x]).astype(f32)
    return np.convolve(xx, h)[m:2*m].astype(f32)


def match32(x, ltas):
    flat = x.ndim == 1
    x2 = np.asarray(x, f32).reshape(len(x), -1)
    n, w = len(x2), R.window().astype(f32)
    wsum = f32(R.window().sum())
    frames = -(-n//256) + 1
    padded = np.zeros((256*(frames + 1), x2.shape[1]), f32)
    padded[256:256 + n] = x2
    seg = np.stack([padded[256*t:256*t + 512] for t in range(frames)], axis=-1)*w[:, None, None]
    X = (np.fft.rfft(seg, axis=0)/wsum).astype(np.complex64)
    power = np.mean(np.abs(X.astype(np.complex128))**2, axis=(1, 2))
    X = (X*np.sqrt(ltas/power).astype(f32)[:, None, None]).astype(np.complex64)
    seg = np.fft.irfft(X, 512, axis=0).astype(f32)*w[:, None, None]*wsum
    y, env = np.zeros_like(padded), np.zeros(len(padded), f32)
    for t in range(frames):
        y[256*t:256*t + 512] += seg[..., t]
        env[256*t:256*t + 512] += w*w
    y = (y/env.clip(1e-10)[:, None])[256:256 + n]
    return y.ravel() if flat else y


def decay32(brir, noise, rt60, drr, delay):
    n = R.decay_length(len(brir), rt60, delay)
    i0 = int(round(delay*FS)) + int(min(np.argmax(np.abs(brir), axis=0)))
    padded = np.zeros((n, 2), f32)
    padded[:len(brir)] = brir
    t = (np.arange(n - i0)/FS).astype(f32)
    tail = np.zeros((n, 2), f32)
    tail[i0:] = (np.exp(-t/f32(rt60)*f32(3*np.log(10)))*np.asarray(noise[:n - i0], f32)).reshape(-1, 1)
    es, en = np.sum(padded.astype(f64).mean(axis=1)**2), np.sum(tail.astype(f64).mean(axis=1)**2)
    return padded + f32((10**(-drr/10)*es/en)**0.5)*tail


def spat32(x, h):
    x, h = np.asarray(x, f32), np.asarray(h, f32)
    return np.stack([np.convolve(x, h[:, e])[:len(x)] for e in range(2)], axis=1).astype(f32)


# -- the cases -------------------------------------------------------------------------------------------------------
def color_cases(M, rng, out):
    for m in (200, 512, 2600, 4099):
        x = rng.standard_normal(m).astype(f32)
        out[f'color_x_{m}'] = x
        for color in COLORS:
            y = with_draws([x], lambda: M.colored_noise(color, m))
            out[f'color_{color}_{m}'] = y
            out[f'color_{color}_{m}_f32err'] = np.array(rel(colorize32(x, color), y))
            print('colour', color, m, f'f32 {float(out[f"color_{color}_{m}_f32err"]):.2e}')


def ltas_cases(M, rng, out):
    ltas = (10**rng.uniform(-4, -1, 257)).astype(f32)
    out['match_ltas'] = ltas
    for n, ch in ((512, 2), (513, 1), (4099, 2)):
        x = (0.1*rng.standard_normal((n, ch) if ch == 2 else n)).astype(f32)
        y = M.match_ltas(f64(x), f64(ltas))
        out[f'match_x_{n}'], out[f'match_y_{n}'] = x, y
        out[f'match_y_{n}_f32err'] = np.array(rel(match32(x, f64(ltas)), y))
        print('match_ltas', n, ch, f'f32 {float(out[f"match_y_{n}_f32err"]):.2e}')


def calc_ltas_case(rng, out):
    import brever.mixture.io as IO
    files = {f'file{i}': (0.1*rng.standard_normal(n)).astype(f32) for i, n in enumerate((700, 1300, 2049))}

    class Loader:
        get_speech_files = staticmethod(lambda speaker: list(files))

    IO.sf.read = lambda name: (f64(files[name]), FS)
    for i, x in enumerate(files.values()):
        out[f'calc_file{i}'] = x
    out['calc_ltas'] = IO.AudioFileLoader.calc_ltas(Loader(), 'speaker')
    print('calc_ltas', out['calc_ltas'][:4])
    return out['calc_ltas']


def decay_cases(M, rng, out):
    for i, (rt60, delay, drr, right) in enumerate(((0.05, 0.01, 10.0, False), (0.01, 0.005, 20.0, False),
                                                   (0.05, 0.01, 15.0, True))):
        h = make_brir(rng, 800, 31, right_larger=right)
        n = R.decay_length(800, rt60, delay)
        noise = rng.standard_normal(n).astype(f32)
        y = with_draws([noise], lambda: M.BRIRDecay(rt60, drr, delay, 'white', FS)(f64(h), seed=0))
        assert y.shape == (n, 2) and n == (1920, 800, 1920)[i]
        out[f'decay_h_{i}'], out[f'decay_noise_{i}'], out[f'decay_y_{i}'] = h, noise, y
        out[f'decay_params_{i}'] = np.array([rt60, drr, delay])
        out[f'decay_y_{i}_f32err'] = np.array(rel(decay32(h, noise, rt60, drr, delay), y))
        print('decay', i, n, f'f32 {float(out[f"decay_y_{i}_f32err"]):.2e}')


def whole_mixtures(rng):
    sig = lambda n: (0.1*rng.standard_normal(n)).astype(f32)                         # noqa: E731
    white = lambda n: rng.standard_normal(n).astype(f32)                             # noqa: E731
    nan, T = float('nan'), 2600
    tails = lambda k, rt60, delay, taps: [white(R.decay_length(t, rt60, delay)) for t in taps[:k]]   # noqa: E731
    a = dict(target=sig(T), brir=make_brir(rng, 1000, 25, decoy=400), noise_types=['file', 'ssn'],
             noises=[sig(T), white(T)], noise_brirs=[make_brir(rng, 700, 30), make_brir(rng, 901, 51)],
             diffuse=[white(T), white(T)], diffuse_brirs=[make_brir(rng, 600, 20), make_brir(rng, 640, 22)],
             diffuse_color='pink', ltas_eq=True, decay=(0.05, 12.0, 0.01), padding=0.0, ndr=5.0, snr=-3.0, tmr=nan,
             rms_jitter=2.5)
    a['tails'] = tails(3, 0.05, 0.01, [1000, 700, 901])
    n_pad = round(0.005*FS)
    b = dict(target=sig(T - 4*n_pad), brir=make_brir(rng, 1025, 37, right_larger=True, decoy=500),
             noise_types=['colored_violet'], noises=[white(T)], noise_brirs=[make_brir(rng, 300, 12, right_larger=True)],
             diffuse=[], diffuse_brirs=[], diffuse_color='white', ltas_eq=False, decay=(0.04, 8.0, 0.006),
             padding=0.005, ndr=nan, snr=nan, tmr=0.4, rms_jitter=-1.0)
    b['tails'] = tails(2, 0.04, 0.006, [1025, 300])
    return [a, b]


def run_whole(M, c, ltas):
    """The reference's make_from_metadata order on one case; returns the Mixture and the gains it applied."""
    gains = {}
    keep = {name: getattr(M, name) for name in ('adjust_snr', 'adjust_rms')}
    for name in keep:
        def spy(*a, _f=keep[name], _n=name, **k):
            y, g = _f(*a, **k)
            gains.setdefault(_n, []).append(g)
            return y, g
        setattr(M, name, spy)
    try:
        rt60, drr, delay = c['decay']
        decay = M.BRIRDecay(rt60, drr, delay, 'white', FS)
        tails = list(c['tails'])
        mix = M.Mixture()
        brir = with_draws([tails[0]], lambda: decay(f64(c['brir']), seed=0))
        mix.add_speech(f64(c['target']), brir, 50e-3, c['padding'], FS)
        xs = []
        for kind, x in zip(c['noise_types'], c['noises']):
            if kind == 'file':
                xs.append(f64(x))
            elif kind == 'ssn':
                xs.append(M.match_ltas(with_draws([x], lambda: M.colored_noise('white', len(mix))), f64(ltas)))
            else:
                xs.append(with_draws([x], lambda: M.colored_noise(kind[8:], len(mix))))
        brirs = [with_draws([t], lambda: decay(f64(h))) for t, h in zip(tails[1:], c['noise_brirs'])]
        mix.add_noises(xs, brirs)
        if c['diffuse']:
            with_draws(c['diffuse'], lambda: mix.add_diffuse_noise([f64(h) for h in c['diffuse_brirs']],
                                                                   c['diffuse_color'],
                                                                   f64(ltas) if c['ltas_eq'] else None))
        gains['adjust_snr'] = []                     # (the decays called it too)
        g = dict(ndr=1.0, snr=1.0, tmr=1.0)
        if not np.isnan(c['ndr']):
            mix.set_ndr(c['ndr'])
            g['ndr'] = gains['adjust_snr'].pop()
        if not np.isnan(c['snr']):
            mix.set_snr(c['snr'])
            g['snr'] = gains['adjust_snr'].pop()
        if not np.isnan(c['tmr']):
            scale = mix.scale_background
            mix.scale_background = lambda gain: (g.update(tmr=float(gain)), scale(gain))
            mix.set_tmr(c['tmr'])
        mix.set_rms(mix.get_rms() + c['rms_jitter'])
        g['rms'] = gains['adjust_rms'].pop()
    finally:
        for name, fn in keep.items():
            setattr(M, name, fn)
    return mix, g


def whole32(M, c, ltas, mix, g):
    """The same mixture from the float32 restatements above, the reference's gains and float32 sums."""
    rt60, drr, delay = c['decay']
    n_pad, T = round(c['padding']*FS), len(mix)
    brir = decay32(c['brir'], c['tails'][0], rt60, drr, delay)
    he, hl = M.split_brir(f64(brir), 50e-3, FS)
    x = np.pad(c['target'], n_pad)
    pad2 = lambda y: np.pad(y, ((n_pad, n_pad), (0, 0)))                            # noqa: E731
    early, late = pad2(spat32(x, he))*f32(g['rms']), pad2(spat32(x, hl))*f32(g['tmr']*g['rms'])
    dirn, diff = np.zeros((T, 2), f32), np.zeros((T, 2), f32)
    for kind, xn, hn, tail in zip(c['noise_types'], c['noises'], c['noise_brirs'], c['tails'][1:]):
        if kind == 'ssn':
            xn = match32(xn, f64(ltas))
        elif kind != 'file':
            xn = colorize32(xn, kind[8:])
        dirn = dirn + spat32(xn, decay32(hn, tail, rt60, drr, delay))
    for xn, hn in zip(c['diffuse'], c['diffuse_brirs']):
        diff = diff + spat32(colorize32(xn, c['diffuse_color']) if c['diffuse_color'] != 'white' else xn, hn)
    if c['ltas_eq'] and c['diffuse']:
        diff = match32(diff, f64(ltas))
    dirn = dirn*f32(g['snr']*g['tmr']*g['rms'])
    diff = diff*f32(g['ndr']*g['snr']*g['tmr']*g['rms'])
    comp = dict(early_speech=early, late_speech=late, dir_noise=dirn, diffuse=diff, foreground=early,
                speech=early + late, noise=dirn + diff)
    comp['background'] = late + comp['noise']
    comp['mixture'] = comp['speech'] + comp['noise']
    return comp


def main():
    M = load_reference()
    rng = np.random.default_rng(20261019)
    out = {'components': np.array(COMPONENTS)}
    color_cases(M, rng, out)
    ltas_cases(M, rng, out)
    ltas = calc_ltas_case(rng, out)
    decay_cases(M, rng, out)
    for i, c in enumerate(whole_mixtures(rng)):
        mix, g = run_whole(M, c, ltas)
        k = f'w{i}_'
        out[k + 'target'], out[k + 'brir'] = c['target'], c['brir']
        for stem, group in (('noise', 'noises'), ('noise_brir', 'noise_brirs'), ('diffuse_in', 'diffuse'),
                            ('diffuse_brir', 'diffuse_brirs'), ('tail', 'tails')):
            for j, a in enumerate(c[group]):
                out[f'{k}{stem}{j}'] = a
        out[k + 'noise_types'] = np.array(c['noise_types'])
        out[k + 'diffuse_color'] = np.array(c['diffuse_color'])
        out[k + 'counts'] = np.array([len(c['noises']), len(c['diffuse']), int(c['ltas_eq'])])
        out[k + 'decay'] = np.array(c['decay'])
        out[k + 'params'] = np.array([c['padding'], c['ndr'], c['snr'], c['tmr'], c['rms_jitter']])
        for name in ('early_speech', 'late_speech', 'dir_noise', 'diffuse'):
            if getattr(mix, name) is not None:
                out[k + name] = getattr(mix, name)
        out[k + 'gains'] = np.array([g['ndr'], g['snr'], g['tmr'], g['rms']])
        out[k + 'labels'] = np.array([mix.get_long_term_label(n) for n in ('tmr', 'tnr', 'trr')])
        out[k + 'speech_idx'] = np.array(mix.speech_idx)
        out[k + 'length'] = np.array(len(mix))
        r32 = whole32(M, c, ltas, mix, g)
        err = []
        for name in COMPONENTS:
            ref = getattr(mix, name)
            err.append(0.0 if ref is None or not np.any(ref) else rel(r32[name], ref))
        out[k + 'f32err'] = np.array(err)
        print('mixture', i, len(mix), mix.speech_idx, 'gains', out[k + 'gains'], 'labels', out[k + 'labels'])
        print('   f32 rel-L2', ' '.join(f'{e:.2e}' for e in err))
    path = os.path.join(HERE, 'mixture_fx.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
