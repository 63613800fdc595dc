"""The batched mixture engine on the GPU against the reference's recorded mixtures (tests/golden/mixture.npz)
and the NumPy restatement of tests/mixture_ref.py.

Bound on every component: 8 x the rel-L2 error that a CPU float32 DIRECT convolution of the same inputs has
against the float64 reference (recorded in the fixture per case and component; computed here the same way
for the shapes the fixture does not hold). The engine keeps fp32 spectra through the partition sum, which is
what the factor covers. Gains and labels: relative 1e-5. Batch independence: bitwise."""
import numpy as np
import pytest
import torch

from mixture_ref import COMPONENTS, golden_cases, run_case, split_brir

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _run(cases, **kw):
    from brever_amd import mixture
    opt = lambda key: [c['kwargs'].get(key) for c in cases]              # noqa: E731
    return mixture.mix([_dev(c['target']) for c in cases], [_dev(c['brir']) for c in cases],
                       [[_dev(x) for x in c['noises']] for c in cases],
                       [[_dev(h) for h in c['noise_brirs']] for c in cases],
                       [[_dev(x) for x in c['diffuse']] for c in cases],
                       [[_dev(h) for h in c['diffuse_brirs']] for c in cases],
                       ndr=opt('ndr'), snr=opt('snr'), tmr=opt('tmr'), rms_jitter=opt('rms_jitter'),
                       padding=opt('padding'), **kw)


def _rel(a, b):
    return float(np.linalg.norm(a - b)/np.linalg.norm(b))


def _f32_direct_error(c, ref, gains):
    """rel-L2 error per component of float32 direct convolutions (the reference's gains, float32 sums) against
    the float64 components ``ref``: the fixture's yardstick, for a case the fixture does not hold."""
    f = np.float32
    n_pad = round(c['kwargs']['padding']*16000)

    def spat(x, h):
        x, h = np.asarray(x, f), np.asarray(h, f)
        return np.stack([np.convolve(x, h[:, e])[:len(x)] for e in range(2)], axis=1).astype(f)

    he, hl = split_brir(np.asarray(c['brir'], np.float64))
    x = np.pad(np.asarray(c['target'], f), n_pad)
    pad2 = lambda y: np.pad(y, ((n_pad, n_pad), (0, 0)))                 # noqa: E731
    g_ndr, g_snr, g_tmr, g_rms = gains
    early, late = pad2(spat(x, he))*f(g_rms), pad2(spat(x, hl))*f(g_tmr*g_rms)
    dirn, diff = np.zeros_like(early), np.zeros_like(early)
    for xn, hn in zip(c['noises'], c['noise_brirs']):
        dirn = dirn + spat(xn, hn)
    for xn, hn in zip(c['diffuse'], c['diffuse_brirs']):
        diff = diff + spat(xn, hn)
    dirn, diff = dirn*f(g_snr*g_tmr*g_rms), diff*f(g_ndr*g_snr*g_tmr*g_rms)
    noise, speech = dirn + diff, early + late
    got = dict(mixture=speech + noise, foreground=early, background=late + noise, speech=speech, noise=noise,
               early_speech=early, late_speech=late, dir_noise=dirn, diffuse=diff)
    return {k: _rel(got[k], ref[k]) if ref[k].any() else 0.0 for k in COMPONENTS}


def _check(res, i, ref, gains, labels, f32err, what):
    """Every component, the gains and the labels of mixture ``i`` of ``res`` against a float64 reference."""
    for name in COMPONENTS:
        got = res.item(i, name).cpu().numpy().astype(np.float64)
        assert got.shape == ref[name].shape, (what, name)
        if not ref[name].any():
            assert not got.any(), (what, name)
            continue
        err, bound = _rel(got, ref[name]), 8*f32err[name]
        print(f'{what} {name}: rel-L2 {err:.3e} (float32 direct {f32err[name]:.3e}, bound {bound:.3e})')
        assert err <= bound, (what, name, err, bound)
    np.testing.assert_allclose(res.gains[i, 4:].cpu().numpy(), gains, rtol=1e-5, err_msg=what)
    np.testing.assert_allclose(res.labels[i].cpu().numpy(), labels, rtol=1e-5, err_msg=what)


@pytest.fixture(scope='module')
def cases():
    return golden_cases()


@pytest.fixture(scope='module')
def alone(cases):
    return [_run([c]).check() for c in cases]


@pytest.fixture(scope='module')
def batched(cases):
    """All four cases in ONE batch: ragged lengths, tap counts, noise counts, paddings."""
    return _run(cases).check()


@pytest.mark.parametrize('i', range(4))
def test_golden_case_matches_the_reference(cases, batched, i):
    c = cases[i]
    assert batched.lengths[i] == c['length'] and batched.speech_idx[i] == c['speech_idx']
    _check(batched, i, c['components'], c['gains'], c['labels'], c['f32err'], f'case {i}')


def test_batched_equals_alone_bitwise(cases, alone, batched):
    """Every component, gain and label of a mixture is bitwise what it is when that mixture runs alone."""
    for i in range(len(cases)):
        for name in COMPONENTS:
            assert torch.equal(batched.item(i, name), alone[i].item(0, name)), (i, name)
        assert torch.equal(batched.gains[i], alone[i].gains[0]), i
        assert torch.equal(batched.labels[i], alone[i].labels[0]), i


@pytest.mark.parametrize('taps', [100, 513])
def test_brir_shorter_than_a_block_and_one_tap_over_two_blocks(taps):
    rng = np.random.default_rng(taps)
    h = (0.05*rng.standard_normal((taps, 2))).astype(np.float32)
    h[7, 0], h[11, 1] = 1.0, 0.7
    n = 1500
    c = dict(target=(0.1*rng.standard_normal(n)).astype(np.float32), brir=h,
             noises=[(0.1*rng.standard_normal(n)).astype(np.float32)], noise_brirs=[h[::-1].copy()],
             diffuse=[], diffuse_brirs=[], kwargs=dict(padding=0.0, snr=3.0, rms_jitter=1.0))
    ref, gains, labels, _ = run_case(c)
    _check(_run([c]).check(), 0, ref, gains, labels, _f32_direct_error(c, ref, gains), f'taps {taps}')


def test_more_frames_than_one_chunk_of_the_product_kernel():
    """66 000 samples are 258 frames of 256: the product kernel's second frame chunk, with a slot of one job
    (its H tile stays resident) and a slot of two (reloaded per chunk), the partitions reaching back across
    the chunk boundary."""
    rng = np.random.default_rng(5)
    n = 66000
    sig = lambda: (0.1*rng.standard_normal(n)).astype(np.float32)        # noqa: E731
    hs = [(0.05*rng.standard_normal((t, 2))*np.exp(-np.arange(t)[:, None]/200)).astype(np.float32)
          for t in (1100, 300, 600)]
    for h in hs:
        h[5, 0], h[9, 1] = 1.0, 0.8
    c = dict(target=sig(), brir=hs[0], noises=[sig(), sig()], noise_brirs=hs[1:], diffuse=[], diffuse_brirs=[],
             kwargs=dict(padding=0.0, snr=0.0, rms_jitter=0.0))
    ref, gains, labels, _ = run_case(c)
    _check(_run([c]).check(), 0, ref, gains, labels, _f32_direct_error(c, ref, gains), 'two chunks')


def test_zero_energies_raise_value_error(cases):
    c = cases[2]
    with pytest.raises(ValueError, match='target signal is 0'):
        _run([dict(c, target=np.zeros_like(c['target']))]).check()
    with pytest.raises(ValueError, match='equals 0'):
        _run([dict(c, diffuse=[np.zeros_like(x) for x in c['diffuse']])]).check()
    # a healthy mixture in the same batch keeps its result; the error names the other one
    res = _run([c, dict(c, target=np.zeros_like(c['target']))])
    with pytest.raises(ValueError, match='mixture 1'):
        res.check()
    _check(res, 0, c['components'], c['gains'], c['labels'], c['f32err'], 'next to a zero target')


def _maker_pools():
    rng = np.random.default_rng(11)
    speech = [(0.1*rng.standard_normal(n)).astype(np.float32) for n in (1900, 2301, 1500)]
    noises = [(0.1*rng.standard_normal(n)).astype(np.float32) for n in (5000, 4100)]
    brirs = [[(0.05*rng.standard_normal((t, 2))).astype(np.float32) for t in (900, 1025)],
             [(0.05*rng.standard_normal((t, 2))).astype(np.float32) for t in (300, 257, 640)]]
    for room in brirs:
        for h in room:
            h[10, 0], h[14, 1] = 1.0, 0.8
    return dict(speech=speech, noises=noises, brirs=brirs)


def test_dataset_over_pool_maker_yields_the_engines_output():
    from brever_amd import data, mixture
    sources = ['mixture', 'foreground']
    kw = dict(seed=2, padding=0.005, noise_count=(1, 2), rms_jitter=(-2.0, 2.0), batch=4, device=DEV,
              **_maker_pools())
    data.set_mixture_maker(lambda path, sources, size: mixture.PoolMixtureMaker(path, sources, size, **kw))
    try:
        ds = data.BreverDataset('unused', sources=sources, dynamic_mixing=True, dynamic_mixtures_per_epoch=6)
        epochs = []
        for epoch in (0, 1):
            ds.set_epoch(epoch)
            items = [ds[i] for i in range(len(ds))]
            maker = mixture.PoolMixtureMaker(None, sources, 6, **kw)
            meta = maker.draw(epoch)
            assert [m['frames'] for m in meta] == ds.get_file_lengths()
            direct = maker.synthesize(meta).check()            # all six in ONE batch; the dataset's came in 4 + 2
            for i, item in enumerate(items):
                assert item.shape == (2, 2, meta[i]['frames']) and item.dtype == torch.float32
                for k, name in enumerate(sources):
                    assert torch.equal(item[k], direct.item(i, name).cpu().T), (epoch, i, name)
            epochs.append(items)
        assert any(a.shape != b.shape or not torch.equal(a, b) for a, b in zip(*epochs))
    finally:
        data.set_mixture_maker(None)


def test_same_seed_and_epoch_give_bitwise_equal_mixtures_with_diffuse_noise():
    """... whatever the batch size: a mixture's white noises come from a seed of its own."""
    from brever_amd import mixture
    kw = dict(seed=5, diffuse=True, noise_count=(1, 1), device=DEV, **_maker_pools())
    runs = []
    for batch in (3, 3, 2, 5):                     # 5 mixtures as 3 + 2 (twice), 2 + 2 + 1 (the queue drains), 5
        maker = mixture.PoolMixtureMaker(None, ['mixture', 'diffuse'], 5, batch=batch, **kw)
        maker.set_epoch(3)
        runs.append([maker[i] for i in range(5)])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for a in runs[0]:
        assert a[1].any() and a[0].shape == a[1].shape and a[0].shape[1] == 2
