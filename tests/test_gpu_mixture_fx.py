"""The mixture effects on the GPU -- colouring, LTAS matching, BRIR decay and whole mixtures that use them --
against the reference's recorded output (tests/golden/mixture_fx.npz).

Bound on every signal, the rule of tests/test_gpu_mixture.py: max(8 x the recorded rel-L2 error of a CPU float32
restatement of the same step against the float64 reference, 2^-23). The floor is one fp32 rounding. Gains, labels
and the LTAS vector: relative 1e-5. Batch independence, the filter cache and determinism: bitwise."""
import numpy as np
import pytest
import torch

import mixture_fx_ref as R
from mixture_ref import COMPONENTS, golden_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
COLORS = ('brown', 'pink', 'blue', 'violet')
LENGTHS = (200, 512, 2600, 4099)
FLOOR = 2.0**-23


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _rel(a, b):
    return float(np.linalg.norm(a - b)/np.linalg.norm(b))


def _hold(got, ref, yardstick, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = _rel(got, ref), max(8*yardstick, FLOOR)
    print(f'{what}: rel-L2 {err:.3e} (float32 restatement {yardstick:.3e}, bound {bound:.3e})')
    assert err <= bound, (what, err, bound)


@pytest.fixture(scope='module')
def z():
    return R.golden()


@pytest.fixture(scope='module')
def mixture():
    from brever_amd import mixture
    return mixture


# -- colouring ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def coloured(z, mixture):
    """All sixteen colour cases in ONE batch: ragged lengths, four filters per length."""
    keys = [(c, m) for m in LENGTHS for c in COLORS]
    out = mixture.colorize([_dev(z[f'color_x_{m}']) for _, m in keys], [c for c, _ in keys])
    return dict(zip(keys, out))


@pytest.mark.parametrize('m', LENGTHS)
@pytest.mark.parametrize('color', COLORS)
def test_colouring_matches_the_reference(z, coloured, color, m):
    _hold(coloured[(color, m)], z[f'color_{color}_{m}'], float(z[f'color_{color}_{m}_f32err']), f'{color} {m}')


def test_coloured_rows_batched_equal_alone_bitwise_and_the_filter_cache_repeats(z, mixture, coloured):
    for (color, m), batched in coloured.items():
        x = _dev(z[f'color_x_{m}'])
        hits = mixture.color_filters.hits
        alone = mixture.colorize([x], color)[0]
        assert mixture.color_filters.hits == hits + 1              # the batch above left the filter resident
        assert torch.equal(alone, batched), (color, m)
    mixture.color_filters.clear()
    misses = mixture.color_filters.misses
    cold = mixture.colorize([x], 'pink')[0]
    warm = mixture.colorize([x], 'pink')[0]
    assert mixture.color_filters.misses == misses + 1 and torch.equal(cold, warm)
    assert torch.equal(cold, coloured[('pink', LENGTHS[-1])])
    white = mixture.colorize([x], 'white')[0]
    assert torch.equal(white, x)
    small = mixture.FilterCache(max_bytes=4*3000)                 # holds one filter of 2600, not two
    for color in ('pink', 'blue', 'pink'):
        small.get(color, 2600, DEV)
    assert small.misses == 3 and small.bytes == 4*2600


def test_more_than_512_partitions_is_refused(mixture):
    with pytest.raises(ValueError, match='larger block'):
        mixture.colorize([torch.zeros(512*64 + 1, device=DEV)], 'pink', block=64)


def test_pink_noise_has_equal_power_per_octave(mixture):
    """4096 samples: the octaves from bin 8 up hold the same power within 1.5 dB. The float64 restatement of the
    reference stays within 0.5 dB for this seed; an inverted exponent (blue) is 20 dB off."""
    x = np.random.default_rng(9).standard_normal(4096).astype(np.float32)

    def spread(y):
        p = np.abs(np.fft.rfft(np.asarray(y, np.float64)))**2
        db = np.array([10*np.log10(p[lo:2*lo].sum()) for lo in (8, 16, 32, 64, 128, 256, 512, 1024)])
        return float(np.abs(db - db.mean()).max())

    ref, got = spread(R.colorize(x, 'pink')), spread(mixture.colorize([_dev(x)], 'pink')[0].cpu().numpy())
    print(f'octave spread: reference {ref:.2f} dB, engine {got:.2f} dB')
    assert ref < 1.5 and got < 1.5
    assert spread(mixture.colorize([_dev(x)], 'blue')[0].cpu().numpy()) > 10


# -- LTAS --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def matched(z, mixture):
    return mixture.match_ltas([_dev(z[f'match_x_{n}']) for n in (512, 513, 4099)], z['match_ltas'].astype(np.float64))


@pytest.mark.parametrize('k, n', enumerate((512, 513, 4099)))
def test_match_ltas_matches_the_reference(z, mixture, matched, k, n):
    _hold(matched[k], z[f'match_y_{n}'], float(z[f'match_y_{n}_f32err']), f'match_ltas {n}')
    alone = mixture.match_ltas([_dev(z[f'match_x_{n}'])], z['match_ltas'].astype(np.float64))[0]
    assert torch.equal(alone, matched[k])                          # ragged batch == alone, bitwise


def test_speech_ltas_matches_calc_ltas(z, mixture):
    got = mixture.speech_ltas([_dev(z[f'calc_file{i}']) for i in range(3)])
    print('calc_ltas: max relative error', float(np.abs(got/z['calc_ltas'] - 1).max()))
    np.testing.assert_allclose(got, z['calc_ltas'], rtol=1e-5)
    with pytest.raises(ValueError, match='512'):
        mixture.match_ltas([torch.zeros(511, device=DEV)], z['match_ltas'])


def test_a_bin_of_zero_power_is_zeroed_not_divided_by(z, mixture):
    """The reference divides by the zero (inf, then NaN samples); the kernel zeroes the bin, as its header says. A
    silent signal next to a live one: zeros out, and the live one keeps its bits."""
    x = _dev(z['match_x_513'])
    silent, live = mixture.match_ltas([torch.zeros(700, 2, device=DEV), x], z['match_ltas'].astype(np.float64))
    assert silent.shape == (700, 2) and not silent.any()
    assert torch.equal(live, mixture.match_ltas([x], z['match_ltas'].astype(np.float64))[0])


# -- BRIRDecay -----------------------------------------------------------------------------------------------------
def _decay_args(z, ids):
    p = [z[f'decay_params_{i}'] for i in ids]
    return ([_dev(z[f'decay_h_{i}']) for i in ids], [_dev(z[f'decay_noise_{i}']) for i in ids],
            [float(v[0]) for v in p], [float(v[1]) for v in p], [float(v[2]) for v in p])


@pytest.fixture(scope='module')
def decayed(z, mixture):
    return mixture.decay_brirs(*_decay_args(z, range(3)))


@pytest.mark.parametrize('i', range(3))
def test_brir_decay_matches_the_reference(z, mixture, decayed, i):
    _hold(decayed[i], z[f'decay_y_{i}'], float(z[f'decay_y_{i}_f32err']), f'decay {i}')
    assert torch.equal(mixture.decay_brirs(*_decay_args(z, [i]))[0], decayed[i])


def test_brir_decay_status(z, mixture):
    h, noise, rt60, drr, delay = _decay_args(z, [0])
    with pytest.raises(ValueError, match='cannot scale noise signal if target signal is 0'):
        mixture.decay_brirs([torch.zeros_like(h[0])], noise, rt60, drr, delay)
    with pytest.raises(ValueError, match='cannot scale noise signal if it equals 0'):
        mixture.decay_brirs(h, [torch.zeros_like(noise[0])], rt60, drr, delay)
    i0 = round(delay[0]*16000) + int(np.argmax(np.abs(z['decay_h_0']), axis=0).min())
    right = mixture.decay_brirs(h, noise, rt60, drr, delay, tail_lengths=[1920 - i0])[0]
    assert torch.equal(right, mixture.decay_brirs(h, noise, rt60, drr, delay)[0])
    with pytest.raises(ValueError, match='claimed length'):
        mixture.decay_brirs(h, noise, rt60, drr, delay, tail_lengths=[1920 - i0 + 1])
    with pytest.raises(ValueError, match='claimed length'):                 # fewer noise samples than the tail
        mixture.decay_brirs(h, [noise[0][:100]], rt60, drr, delay)
    assert mixture.decay_brirs(h, noise, 0.0, drr, delay)[0] is h[0]       # rt60 = 0: the BRIR itself


# -- whole mixtures --------------------------------------------------------------------------------------------------
def _run_whole(mixture, cases):
    """The pre-pass through the public functions, one call each for all cases, then ``mix``. A case without
    ``decay`` is a plain one (tests/golden/mixture.npz)."""
    brirs, tails, rt60, drr, delay, slot = [], [], [], [], [], []
    for c in cases:
        hs = [c['brir']] + list(c['noise_brirs'])
        slot.append(range(len(brirs), len(brirs) + len(hs)))
        brirs += [_dev(h) for h in hs]
        d = c.get('decay') or (0.0, 0.0, 0.0)
        tails += [_dev(t) for t in c.get('tails') or [np.zeros(1)]*len(hs)]
        rt60 += [d[0]]*len(hs)
        drr += [d[1]]*len(hs)
        delay += [d[2]]*len(hs)
    brirs = mixture.decay_brirs(brirs, tails, rt60, drr, delay)
    rows, colors, ssn = [], [], []
    noises = [[_dev(x) for x in c['noises']] for c in cases]
    diffuse = [[_dev(x) for x in c['diffuse']] for c in cases]
    for i, c in enumerate(cases):
        for j, kind in enumerate(c.get('noise_types') or []):
            if kind == 'ssn':
                ssn.append((i, j))
            elif kind != 'file':
                rows.append((noises, i, j))
                colors.append(kind[len('colored_'):])
        if c.get('diffuse_color', 'white') != 'white':
            rows += [(diffuse, i, j) for j in range(len(c['diffuse']))]
            colors += [c['diffuse_color']]*len(c['diffuse'])
    if rows:
        for (group, i, j), y in zip(rows, mixture.colorize([g[i][j] for g, i, j in rows], colors)):
            group[i][j] = y
    ltas = None
    if ssn:
        ltas = _dev(cases[ssn[0][0]]['ltas']).double()
        for (i, j), y in zip(ssn, mixture.match_ltas([noises[i][j] for i, j in ssn], ltas)):
            noises[i][j] = y
    opt = lambda key: [c['kwargs'].get(key) for c in cases]              # noqa: E731
    kw = {}
    if any(c.get('ltas_eq') for c in cases):
        kw = dict(diffuse_ltas=[bool(c.get('ltas_eq')) for c in cases], ltas=_dev(cases[0]['ltas']).double())
    return mixture.mix([_dev(c['target']) for c in cases], [brirs[s[0]] for s in slot], noises,
                       [[brirs[k] for k in s[1:]] for s in slot], diffuse,
                       [[_dev(h) for h in c['diffuse_brirs']] for c in cases],
                       ndr=opt('ndr'), snr=opt('snr'), tmr=opt('tmr'), rms_jitter=opt('rms_jitter'),
                       padding=opt('padding'), **kw).check()


@pytest.fixture(scope='module')
def whole():
    return R.whole_cases()


@pytest.fixture(scope='module')
def plain():
    return golden_cases()[2]                   # two directional noises, two white diffuse noises, ndr + snr


@pytest.fixture(scope='module')
def together(mixture, whole, plain):
    return _run_whole(mixture, [whole[0], plain, whole[1]])


@pytest.mark.parametrize('i', range(2))
def test_whole_mixture_matches_the_reference(whole, together, i):
    c, k = whole[i], (0, 2)[i]
    assert together.lengths[k] == c['length'] and together.speech_idx[k] == c['speech_idx']
    for name in COMPONENTS:
        ref = c['components'][name]
        if not ref.any():
            assert not together.item(k, name).any(), name
            continue
        _hold(together.item(k, name), ref, c['f32err'][name], f'mixture {i} {name}')
    np.testing.assert_allclose(together.gains[k, 4:].cpu().numpy(), c['gains'], rtol=1e-5)
    np.testing.assert_allclose(together.labels[k].cpu().numpy(), c['labels'], rtol=1e-5)


def test_whole_mixtures_batched_equal_alone_bitwise(mixture, whole, plain, together):
    alone = [_run_whole(mixture, [c]) for c in (whole[0], plain, whole[1])]
    k = plain['kwargs']                        # the entry point as it was: no new option present
    untouched = mixture.mix([_dev(plain['target'])], [_dev(plain['brir'])], [[_dev(x) for x in plain['noises']]],
                            [[_dev(h) for h in plain['noise_brirs']]], [[_dev(x) for x in plain['diffuse']]],
                            [[_dev(h) for h in plain['diffuse_brirs']]], ndr=[k['ndr']], snr=[k['snr']], tmr=[k['tmr']],
                            rms_jitter=[k['rms_jitter']], padding=[k['padding']]).check()
    for k, one in enumerate(alone):
        for other in ([one, untouched] if k == 1 else [one]):
            for name in COMPONENTS:
                assert torch.equal(together.item(k, name), other.item(0, name)), (k, name)
            assert torch.equal(together.gains[k], other.gains[0]) and torch.equal(together.labels[k], other.labels[0])


def test_diffuse_ltas_needs_the_ltas(mixture, whole):
    c = dict(whole[0], kwargs=dict(whole[0]['kwargs']))
    x, h = _dev(c['target']), _dev(c['brir'])
    with pytest.raises(ValueError, match='ltas'):
        mixture.mix([x], [h], diffuse=[[x]], diffuse_brirs=[[h]], diffuse_ltas=[True])
    with pytest.raises(ValueError, match='512'):
        mixture.mix([x[:500]], [h], diffuse=[[x[:500]]], diffuse_brirs=[[h]], diffuse_ltas=[True],
                    ltas=_dev(c['ltas']).double())


# -- PoolMixtureMaker ------------------------------------------------------------------------------------------------
def _maker_pools():
    rng = np.random.default_rng(13)
    speech = [(0.1*rng.standard_normal(n)).astype(np.float32) for n in (1900, 2301, 1500)]
    noises = [(0.1*rng.standard_normal(n)).astype(np.float32) for n in (5000, 4100)]
    brirs = [[(0.05*rng.standard_normal((t, 2))).astype(np.float32) for t in (900, 1025)],
             [(0.05*rng.standard_normal((t, 2))).astype(np.float32) for t in (300, 257, 640)]]
    for room in brirs:
        for k, h in enumerate(room):
            h[10 + k, 0], h[14, 1] = 1.0, 0.8
    return dict(speech=speech, noises=noises, brirs=brirs)


ALL_ON = dict(diffuse=True, diffuse_color='pink', diffuse_ltas_eq=True, decay=True, decay_color='brown',
              decay_rt60=(0.02, 0.06), synthetic_noises=('ssn', 'colored_violet', 'colored_white'), noise_count=(1, 3),
              padding=0.005, rms_jitter=(-2.0, 2.0))


def test_maker_with_every_option_is_deterministic_and_feeds_the_dataset(mixture):
    from brever_amd import data
    sources = ['mixture', 'foreground', 'diffuse', 'dir_noise']
    kw = dict(seed=2, device=DEV, **ALL_ON, **_maker_pools())
    runs = []
    for batch in (4, 4, 7):                    # 7 mixtures as 4 + 3 (twice) and in one batch
        maker = mixture.PoolMixtureMaker(None, sources, 7, batch=batch, **kw)
        maker.set_epoch(3)
        runs.append([maker[i] for i in range(7)])
    kinds = {n.get('type', 'file') for m in maker.draw(3) for n in m['noises']}
    assert len(kinds) >= 3, kinds              # files and synthetic noises were both drawn
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for a in runs[0]:
        assert all(np.isfinite(x).all() and x.any() for x in a)
    data.set_mixture_maker(lambda path, sources, size: mixture.PoolMixtureMaker(path, sources, size, batch=4, **kw))
    try:
        ds = data.BreverDataset('unused', sources=sources, dynamic_mixing=True, dynamic_mixtures_per_epoch=7)
        ds.set_epoch(3)
        maker = mixture.PoolMixtureMaker(None, sources, 7, **kw)
        meta = maker.draw(3)
        direct = maker.synthesize(meta).check()
        for i in range(7):
            item = ds[i]
            assert item.shape == (len(sources), 2, meta[i]['frames'])
            for k, name in enumerate(sources):
                assert torch.equal(item[k], direct.item(i, name).cpu().T), (i, name)
                assert np.array_equal(runs[0][i][k], direct.item(i, name).cpu().numpy()), (i, name)
    finally:
        data.set_mixture_maker(None)


def test_maker_without_the_new_options_is_unchanged_by_them(mixture):
    """A maker whose decay is on with ``rt60 = 0`` (the identity) gives, for the same draws, bitwise what a maker
    without the option gives: the pre-pass leaves a mixture that asks for nothing as it was."""
    kw = dict(seed=5, diffuse=True, noise_count=(1, 2), device=DEV, **_maker_pools())
    a = mixture.PoolMixtureMaker(None, ['mixture', 'diffuse'], 5, **kw)
    b = mixture.PoolMixtureMaker(None, ['mixture', 'diffuse'], 5, decay=True, decay_rt60=(0.0, 0.0), **kw)
    ra = a.synthesize(a.draw(1)).check()
    meta = b.draw(1)
    assert all(m['decay']['rt60'] == 0 for m in meta)
    for m, n in zip(meta, a.draw(1)):          # the other maker's draws, the decay key kept
        m.update(n)
    rb = b.synthesize(meta).check()
    for i in range(5):
        for name in ('mixture', 'diffuse'):
            assert torch.equal(ra.item(i, name), rb.item(i, name)), (i, name)
