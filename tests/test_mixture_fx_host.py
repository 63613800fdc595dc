"""The mixture effects on the host: the NumPy restatement (tests/mixture_fx_ref.py) against the reference's recorded
output, the C ABI of libbrever_mixfx.so (header, exports, refusals) and the draws of PoolMixtureMaker with the new
options off (the recorded draws of the commit before them) and on. No GPU."""
import ctypes
import json

import numpy as np
import pytest

import mixture_fx_ref as R
from brever_amd import hip, mixture
from mixture_ref import COMPONENTS

COLORS = ('brown', 'pink', 'blue', 'violet')
LENGTHS = (200, 512, 2600, 4099)


def _rel(a, b):
    return float(np.linalg.norm(a - b)/np.linalg.norm(b))


@pytest.fixture(scope='module')
def z():
    return R.golden()


# -- the restatement against the fixture -----------------------------------------------------------------------------
def test_fixture_holds_the_cases_and_yardsticks(z):
    for m in LENGTHS:
        for color in COLORS:
            assert z[f'color_{color}_{m}'].shape == (m,)
            assert 3e-8 < float(z[f'color_{color}_{m}_f32err']) < 3e-7
    assert [z[f'match_x_{n}'].shape for n in (512, 513, 4099)] == [(512, 2), (513,), (4099, 2)]
    for n in (512, 513, 4099):
        assert 5e-8 < float(z[f'match_y_{n}_f32err']) < 2e-7
    assert [len(z[f'calc_file{i}']) for i in range(3)] == [700, 1300, 2049]
    assert [z[f'decay_y_{i}'].shape[0] for i in range(3)] == [1920, 800, 1920]
    lead = [np.argmax(np.abs(z[f'decay_h_{i}']), axis=0) for i in range(3)]
    assert lead[0][0] < lead[0][1] and lead[2][1] < lead[2][0]             # once the right ear leads
    cases = R.whole_cases()
    assert [c['noise_types'] for c in cases] == [['file', 'ssn'], ['colored_violet']]
    assert cases[0]['diffuse_color'] == 'pink' and cases[0]['ltas_eq'] and len(cases[0]['diffuse']) == 2
    assert None not in (cases[0]['kwargs']['ndr'], cases[0]['kwargs']['snr'])
    assert cases[1]['kwargs']['tmr'] is not None and cases[1]['kwargs']['padding'] == 0.005
    assert [c['length'] for c in cases] == [2600, 2600]


def test_colouring_restatement_and_the_convolution_identity(z):
    for m in LENGTHS:
        x = z[f'color_x_{m}'].astype(np.float64)
        for color in COLORS:
            ref = z[f'color_{color}_{m}']
            assert _rel(R.colorize(x, color), ref) < 1e-12, (color, m)
            # what the engine computes: the linear convolution of [x, x] with h_m = irfft(s, m), samples [m, 2m)
            h = np.fft.irfft(R.color_scaling(color, m), m)
            assert _rel(np.convolve(np.concatenate([x, x]), h)[m:2*m], ref) < 1e-11, (color, m)
    assert np.array_equal(R.colorize(x, 'white'), np.fft.irfft(np.fft.rfft(x), len(x)))


def test_match_ltas_and_calc_ltas_restatements(z):
    for n in (512, 513, 4099):
        got = R.match_ltas(z[f'match_x_{n}'], z['match_ltas'].astype(np.float64))
        assert got.shape == z[f'match_y_{n}'].shape
        assert _rel(got, z[f'match_y_{n}']) < 1e-12, n
    np.testing.assert_allclose(R.calc_ltas([z[f'calc_file{i}'] for i in range(3)]), z['calc_ltas'], rtol=1e-12)
    np.testing.assert_allclose(mixture.smooth_ltas(R.calc_ltas([z['calc_file0']])*0 + np.arange(1.0, 258.0)),
                               R.smooth_ltas(np.arange(1.0, 258.0)), rtol=1e-15)
    with pytest.raises(ValueError, match='512'):
        R.match_ltas(np.ones(511), np.ones(257))


def test_brir_decay_restatement(z):
    for i in range(3):
        rt60, drr, delay = z[f'decay_params_{i}']
        got, i0 = R.brir_decay(z[f'decay_h_{i}'], z[f'decay_noise_{i}'], rt60, drr, delay)
        assert _rel(got, z[f'decay_y_{i}']) < 1e-12, i
    h = z['decay_h_0']
    assert R.brir_decay(h, None, 0.0, 10.0, 0.01)[0] is not None and np.array_equal(R.brir_decay(h, None, 0, 1, 1)[0], h)
    with pytest.raises(ValueError, match='target signal is 0'):
        R.brir_decay(np.zeros((800, 2)), z['decay_noise_0'], 0.05, 10.0, 0.01)


def test_whole_mixture_restatement():
    for c in R.whole_cases():
        comp, gains, labels, idx = R.run_whole(c)
        assert idx == c['speech_idx'] and len(comp['mixture']) == c['length']
        for name in COMPONENTS:
            ref = c['components'][name]
            if not ref.any():
                assert not comp[name].any(), name
                continue
            assert _rel(comp[name], ref) < 1e-12, (name, _rel(comp[name], ref))
        np.testing.assert_allclose(gains, c['gains'], rtol=1e-12)
        np.testing.assert_allclose(labels, c['labels'], rtol=1e-12)


def test_filter_the_engine_uploads_is_the_restatements(z):
    f = np.arange(4099//2 + 1)/4099
    f[0] = f[1]
    assert np.array_equal(f**(-1/2), R.color_scaling('pink', 4099)) and mixture.COLORS == R.ALPHA


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_mixfx_version', 'brv_mixfx_last_error', 'brv_mixfx_pack_periodic', 'brv_mixfx_copy_rows',
           'brv_mixfx_ltas_power', 'brv_mixfx_ltas_equalize', 'brv_mixfx_decay_brirs'}


def test_header_parses_and_every_export_resolves():
    with open(mixture.FX_HEADER_PATH) as f:
        table = hip.parse_header(f.read())
    assert set(table) == EXPORTS == set(mixture.FX_SIGNATURES)
    lib = mixture.fx_lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        if name not in ('brv_mixfx_version', 'brv_mixfx_last_error'):
            # the conventions of the other libraries: int status, a stream as the last argument
            assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr, name
    assert lib.brv_mixfx_version() >= 100
    # a library of its own: nothing of it is declared in, or exported by, the other two
    assert not any(n.startswith('brv_mixfx_') for n in list(hip.SIGNATURES) + list(mixture.SIGNATURES))
    assert not hasattr(mixture.lib(), 'brv_mixfx_version')


# Number arguments that a call would ACCEPT (by position) where all ones would not be: the pool lengths of the
# decay hold an ear pair.
BASELINE = {'brv_mixfx_decay_brirs': {6: 2, 8: 2}}


def _args(name, fill):
    _, argtypes = mixture.FX_SIGNATURES[name]
    base = BASELINE.get(name, {})
    return [None if i == len(argtypes) - 1 else fill if t is hip._c_ptr else base.get(i, 1)
            for i, t in enumerate(argtypes)]


@pytest.mark.parametrize('name', sorted(EXPORTS - {'brv_mixfx_version', 'brv_mixfx_last_error'}))
def test_every_export_refuses_null_and_zero_arguments(name):
    lib = mixture.fx_lib()
    _, argtypes = mixture.FX_SIGNATURES[name]
    buf = ctypes.create_string_buffer(64)            # never read: each call below is refused on the host
    other = 'brv_mixfx_copy_rows' if name != 'brv_mixfx_copy_rows' else 'brv_mixfx_pack_periodic'
    assert getattr(lib, other)(*_args(other, None)) == -1
    sentinel = lib.brv_mixfx_last_error()
    assert sentinel
    assert getattr(lib, name)(*_args(name, None)) == -1
    null_msg = lib.brv_mixfx_last_error()
    assert null_msg and b'null' in null_msg and null_msg != sentinel
    for i, t in enumerate(argtypes[:-1]):
        if t is hip._c_ptr:
            continue
        args = _args(name, buf)
        args[i] = 0
        assert getattr(lib, name)(*args) == -1, (name, i)
        msg = lib.brv_mixfx_last_error()
        assert msg and msg != null_msg and b'requires' in msg, (name, i, msg)
    with pytest.raises(RuntimeError, match=name):
        mixture.fx_call(name, *_args(name, None))


# -- PoolMixtureMaker: draws --------------------------------------------------------------------------------------
def test_default_draws_are_the_recorded_ones():
    with open(R.DRAWS) as f:
        recorded = json.load(f)
    assert set(recorded) == set(R.DRAW_CONFIGS)
    for name, kw in R.DRAW_CONFIGS.items():
        maker = mixture.PoolMixtureMaker(None, ['mixture'], 12, **kw, **R.draw_pool())
        for epoch in (0, 3):
            assert maker.draw(epoch) == recorded[name][str(epoch)], (name, epoch)
        # the options spelt out at their defaults: the same
        spelt = mixture.PoolMixtureMaker(None, ['mixture'], 12, diffuse_color='white', diffuse_ltas_eq=False,
                                         decay=False, decay_color='white', synthetic_noises=(), **kw, **R.draw_pool())
        assert spelt.draw(3) == recorded[name]['3']


FX = dict(diffuse=True, diffuse_color='pink', diffuse_ltas_eq=True, decay=True, decay_color='white',
          decay_rt60=(0.02, 0.06), synthetic_noises=('ssn', 'colored_violet'), noise_count=(1, 3))


def test_draws_with_the_new_options_are_a_function_of_seed_and_epoch():
    a = mixture.PoolMixtureMaker(None, ['mixture'], 24, seed=3, **FX, **R.draw_pool())
    b = mixture.PoolMixtureMaker(None, ['mixture'], 24, seed=3, **FX, **R.draw_pool())
    c = mixture.PoolMixtureMaker(None, ['mixture'], 24, seed=4, **FX, **R.draw_pool())
    assert a.draw(0) == b.draw(0) and a.draw(5) == b.draw(5)
    assert a.draw(0) != a.draw(1) and a.draw(0) != c.draw(0)
    kinds, seeds = set(), []
    for m in a.draw(2):
        d = m['decay']
        assert 0.02 <= d['rt60'] <= 0.06 and 5 <= d['drr'] <= 35 and 0.075 <= d['delay'] <= 0.1
        assert d['color'] == 'white' and len(d['seeds']) == 1 + len(m['noises'])   # a tail seed per decayed BRIR
        assert m['diffuse_color'] == 'pink' and m['diffuse_ltas_eq'] is True
        seeds += d['seeds'] + [m['diffuse_seed']]
        for n in m['noises']:
            kinds.add(n.get('type', 'file'))
            if 'type' in n:
                seeds.append(n['seed'])
            else:
                assert n['i_start'] + m['frames'] <= len(R.draw_pool()['noises'][n['file']])
    assert kinds == {'file', 'ssn', 'colored_violet'} and len(set(seeds)) == len(seeds)
    with pytest.raises(ValueError, match='colored_'):
        mixture.PoolMixtureMaker(None, ['mixture'], 4, synthetic_noises=('colored_green',), **R.draw_pool())
    with pytest.raises(ValueError, match='color'):
        mixture.PoolMixtureMaker(None, ['mixture'], 4, diffuse_color='green', **R.draw_pool())


def test_ltas_over_fewer_than_512_samples_raises():
    pool = R.draw_pool()
    pool['speech'] = pool['speech'] + [np.ones(511, np.float32)]
    for kw in (dict(diffuse=True, diffuse_ltas_eq=True), dict(synthetic_noises=('ssn',))):
        with pytest.raises(ValueError, match='512'):
            mixture.PoolMixtureMaker(None, ['mixture'], 4, **kw, **pool)
    mixture.PoolMixtureMaker(None, ['mixture'], 4, diffuse_ltas_eq=True, **pool)       # no diffuse noise: no LTAS
    import torch
    with pytest.raises(ValueError, match='512'):
        mixture.match_ltas([torch.zeros(511)], np.ones(257))
