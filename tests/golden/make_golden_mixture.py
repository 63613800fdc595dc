"""Generate tests/golden/mixture.npz from the *imported reference* ``brever.mixture.mixture.Mixture``.

Runs only where the reference checkout is mounted (``BREVER_REFERENCE``, default /root/reference); nothing
of the reference is copied -- the fixture holds seeded inputs and recorded outputs. ``brever.mixture`` imports
``sofa`` and ``soundfile``, absent here and not part of the arithmetic: empty stand-ins go into ``sys.modules``
before the import.

    python tests/golden/make_golden_mixture.py

Each case follows ``RandomMixtureMaker.make_from_metadata``: add_speech, add_noises, add_diffuse_noise,
set_ndr, set_snr, set_tmr, set_rms(get_rms() + rms_jitter). The diffuse noise signals are drawn here and handed
to ``Mixture.add_diffuse_noise`` through its ``colored_noise`` hook, so the method itself runs. All inputs are
float32 values (stored as float32, given to the reference as float64).

Recorded per case ``c<i>_``:
  inputs   target, brir, noise<j>, noise_brir<j>, diffuse<j>, diffuse_brir<j>,
           params = [padding, ndr, snr, tmr, rms_jitter] (nan = not set)
  outputs  early_speech, late_speech, dir_noise, diffuse (float64, final gains applied): the four stored
           components. The other five are their sums by ``Mixture``'s own properties (speech = early + late,
           noise = dir + diffuse, mixture = speech + noise, foreground = early, background = late + noise);
           storing all nine in float64 would pass the 1 MiB limit of a committed file.
           gains = [ndr, snr, tmr, rms] (1 = not applied), labels = [tmr, tnr, trr], speech_idx, length
  f32err   rel-L2 error, per component in COMPONENTS order, of a CPU float32 restatement (direct
           ``np.convolve`` in float32, the reference's gains applied in float32, sums in float32) against
           the float64 reference: the yardstick the GPU test scales its bound from.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('BREVER_REFERENCE', '/root/reference')
COMPONENTS = ('mixture', 'foreground', 'background', 'speech', 'noise', 'early_speech', 'late_speech',
              'dir_noise', 'diffuse')
FS = 16000


def load_reference():
    for name in ('sofa', 'soundfile'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    import brever.mixture.mixture as M
    return M


def make_brir(rng, taps, peak, right_larger=False, decoy=None):
    """Decaying-noise BRIR with a direct-sound peak per ear, 5 samples apart. ``decoy``: a late reflection in
    the weaker ear that exceeds that ear's direct sound, so that split_brir's max_itd correction acts."""
    t = np.arange(taps)[:, None]
    h = 0.05*rng.standard_normal((taps, 2))*np.exp(-t/(0.25*taps))
    strong, weak = (1, 0) if right_larger else (0, 1)
    h[peak, strong] = 1.0
    h[peak + 5, weak] = 0.6
    if decoy is not None:
        h[decoy, weak] = 0.8
    return h.astype(np.float32)


def cases():
    rng = np.random.default_rng(20261018)
    sig = lambda n: (0.1*rng.standard_normal(n)).astype(np.float32)      # noqa: E731
    nan = float('nan')
    out = []
    # 0: plain speech, BRIR of 1300 taps, no padding
    out.append(dict(target=sig(4000), brir=make_brir(rng, 1300, 40), noises=[], noise_brirs=[], diffuse=[],
                    diffuse_brirs=[], padding=0.0, ndr=nan, snr=nan, tmr=nan, rms_jitter=0.0))
    # 1: odd lengths, taps one over a block multiple, padded before and again after spatialisation
    out.append(dict(target=sig(5003), brir=make_brir(rng, 2049, 33), noises=[], noise_brirs=[], diffuse=[],
                    diffuse_brirs=[], padding=0.01, ndr=nan, snr=nan, tmr=nan, rms_jitter=0.0))
    # 2: two directional noises, two diffuse BRIRs, ndr + snr + rms_jitter
    n = 2600
    out.append(dict(target=sig(n), brir=make_brir(rng, 1000, 25, decoy=400),
                    noises=[sig(n), sig(n)], noise_brirs=[make_brir(rng, 700, 30), make_brir(rng, 901, 51)],
                    diffuse=[sig(n), sig(n)], diffuse_brirs=[make_brir(rng, 600, 20), make_brir(rng, 640, 22)],
                    padding=0.0, ndr=5.0, snr=-3.0, tmr=nan, rms_jitter=2.5))
    # 3: tmr set, the right ear's peak is the larger one (and the left ear has a louder late reflection)
    n_pad = round(0.005*FS)
    n = 2400 + 4*n_pad
    out.append(dict(target=sig(2400), brir=make_brir(rng, 1025, 37, right_larger=True, decoy=500),
                    noises=[sig(n)], noise_brirs=[make_brir(rng, 300, 12, right_larger=True)],
                    diffuse=[], diffuse_brirs=[], padding=0.005, ndr=nan, snr=nan, tmr=0.4, rms_jitter=-1.0))
    return out


def run_reference(M, c):
    """The reference's Mixture on one case; returns it with the four gains it applied."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)                      # noqa: E731
    gains = {}
    for name in ('adjust_snr', 'adjust_rms'):
        def spy(*a, _f=getattr(M, name), _n=name, **k):
            y, g = _f(*a, **k)
            gains.setdefault(_n, []).append(g)
            return y, g
        setattr(M, name, spy)
    mix = M.Mixture()
    mix.add_speech(f64(c['target']), f64(c['brir']), 50e-3, c['padding'], FS)
    if c['noises']:
        mix.add_noises([f64(x) for x in c['noises']], [f64(h) for h in c['noise_brirs']])
    if c['diffuse']:
        drawn = iter(c['diffuse'])
        keep = M.colored_noise
        M.colored_noise = lambda color, n: f64(next(drawn))
        mix.add_diffuse_noise([f64(h) for h in c['diffuse_brirs']], 'white')
        M.colored_noise = keep
    pre = {k: None if getattr(mix, k) is None else getattr(mix, k).copy()
           for k in ('early_speech', 'late_speech', 'dir_noise', 'diffuse')}
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
    return mix, pre, g


def float32_restatement(c, mix, g):
    """The same mixture from float32 direct convolutions, the reference's gains and float32 sums."""
    n_pad = round(c['padding']*FS)
    T = len(mix)

    def spat(x, h):
        x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
        return np.stack([np.convolve(x, h[:, e])[:len(x)] for e in range(2)], axis=1).astype(np.float32)

    M = sys.modules['brever.mixture.mixture']
    he, hl = M.split_brir(np.asarray(c['brir'], np.float64), 50e-3, FS)
    x = np.pad(c['target'], n_pad)
    pad2 = lambda y: np.pad(y, ((n_pad, n_pad), (0, 0)))                 # noqa: E731
    f = np.float32
    early = pad2(spat(x, he))*f(g['rms'])
    late = pad2(spat(x, hl))*f(g['tmr']*g['rms'])
    zero = np.zeros((T, 2), np.float32)
    dirn, diff = zero.copy(), zero.copy()
    for xn, hn in zip(c['noises'], c['noise_brirs']):
        dirn = dirn + spat(xn, hn)
    for xn, hn in zip(c['diffuse'], c['diffuse_brirs']):
        diff = diff + spat(xn, hn)
    dirn = dirn*f(g['snr']*g['tmr']*g['rms'])
    diff = diff*f(g['ndr']*g['snr']*g['tmr']*g['rms'])
    comp = dict(early_speech=early, late_speech=late, dir_noise=dirn, diffuse=diff, foreground=early,
                speech=early + late, noise=dirn + diff)
    comp['background'] = late + comp['noise']
    comp['mixture'] = comp['speech'] + comp['noise']
    return comp


def main():
    M = load_reference()
    out = {'components': np.array(COMPONENTS)}
    for i, c in enumerate(cases()):
        mix, pre, g = run_reference(M, c)
        k = f'c{i}_'
        out[k + 'target'], out[k + 'brir'] = c['target'], c['brir']
        for group in ('noises', 'noise_brirs', 'diffuse', 'diffuse_brirs'):
            stem = {'noises': 'noise', 'noise_brirs': 'noise_brir', 'diffuse': 'diffuse_in',
                    'diffuse_brirs': 'diffuse_brir'}[group]
            for j, a in enumerate(c[group]):
                out[f'{k}{stem}{j}'] = a
        out[k + 'counts'] = np.array([len(c['noises']), len(c['diffuse'])])
        out[k + 'params'] = np.array([c['padding'], c['ndr'], c['snr'], c['tmr'], c['rms_jitter']])
        for name in ('early_speech', 'late_speech', 'dir_noise', 'diffuse'):
            if getattr(mix, name) is not None:
                out[k + name] = getattr(mix, name)
        out[k + 'gains'] = np.array([g['ndr'], g['snr'], g['tmr'], g['rms']])
        out[k + 'labels'] = np.array([mix.get_long_term_label(n) for n in ('tmr', 'tnr', 'trr')])
        out[k + 'speech_idx'] = np.array(mix.speech_idx)
        out[k + 'length'] = np.array(len(mix))
        f32 = float32_restatement(c, mix, g)
        err = []
        for name in COMPONENTS:
            ref = getattr(mix, name)
            if ref is None or not np.any(ref):
                err.append(0.0)
                continue
            err.append(float(np.linalg.norm(f32[name] - ref)/np.linalg.norm(ref)))
        out[k + 'f32err'] = np.array(err)
        print(i, len(mix), mix.speech_idx, 'gains', out[k + 'gains'], 'labels', out[k + 'labels'])
        print('   f32 direct rel-L2', ' '.join(f'{e:.2e}' for e in err))
    path = os.path.join(HERE, 'mixture.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
