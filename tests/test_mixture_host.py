"""The mixture engine on the host: the NumPy restatement against the reference's recorded output, the C ABI of
libbrever_mix.so (header, exports, refusals) and the draws of PoolMixtureMaker. No GPU."""
import ctypes

import numpy as np
import pytest

from brever_amd import hip, mixture
from mixture_ref import COMPONENTS, golden_cases, run_case


def _rel(a, b):
    return float(np.linalg.norm(a - b)/np.linalg.norm(b))


@pytest.fixture(scope='module')
def cases():
    return golden_cases()


def test_golden_holds_the_cases_the_engine_is_checked_on(cases):
    assert len(cases) == 4
    assert (len(cases[0]['target']), cases[0]['brir'].shape[0], cases[0]['kwargs']['padding']) == (4000, 1300, 0.0)
    # odd length, taps one over a block multiple, padded before and again after spatialisation
    assert (len(cases[1]['target']), cases[1]['brir'].shape[0], cases[1]['kwargs']['padding']) == (5003, 2049, 0.01)
    assert cases[1]['length'] == 5643 and cases[1]['speech_idx'] == (160, 5163)
    k = cases[2]['kwargs']
    assert (len(cases[2]['noises']), len(cases[2]['diffuse_brirs'])) == (2, 2)
    assert None not in (k['ndr'], k['snr']) and k['rms_jitter'] != 0
    assert cases[3]['kwargs']['tmr'] is not None
    peaks = np.abs(cases[3]['brir']).max(axis=0)
    assert peaks[1] > peaks[0]
    for c in cases:
        for name in ('mixture', 'early_speech', 'late_speech'):
            assert 5e-8 < c['f32err'][name] < 3e-7, (name, c['f32err'][name])


def test_numpy_restatement_matches_the_reference_to_1e_12(cases):
    for c in cases:
        comp, gains, labels, idx = run_case(c)
        assert idx == c['speech_idx'] and len(comp['mixture']) == c['length']
        for name in COMPONENTS:
            ref = c['components'][name]
            if not ref.any():
                assert not comp[name].any(), name
                continue
            assert _rel(comp[name], ref) < 1e-12, (name, _rel(comp[name], ref))
        np.testing.assert_allclose(gains, c['gains'], rtol=1e-12)
        np.testing.assert_allclose(labels, c['labels'], rtol=1e-12)


def test_restatement_raises_on_zero_energies(cases):
    c = dict(cases[2])
    with pytest.raises(ValueError, match='target signal is 0'):
        run_case(dict(c, target=np.zeros_like(c['target'])))
    with pytest.raises(ValueError, match='equals 0'):
        run_case(dict(c, diffuse=[np.zeros_like(x) for x in c['diffuse']]))


# -- the C ABI ---------------------------------------------------------------------------------------------------
EXPORTS = {'brv_mix_version', 'brv_mix_last_error', 'brv_mix_pack_signals', 'brv_mix_pack_brirs',
           'brv_mix_partition_mac', 'brv_mix_energies', 'brv_mix_gains', 'brv_mix_compose'}


def test_header_parses_and_every_export_resolves():
    with open(mixture.HEADER_PATH) as f:
        table = hip.parse_header(f.read())
    assert set(table) == EXPORTS == set(mixture.SIGNATURES)
    lib = mixture.lib()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        if name not in ('brv_mix_version', 'brv_mix_last_error'):
            # the conventions of the main library: int status, a stream as the last argument
            assert restype is ctypes.c_int and argtypes[-1] is hip._c_ptr, name
    assert lib.brv_mix_version() >= 100
    # a library of its own: nothing of it is declared in, or exported by, the main one
    assert not any(n.startswith('brv_mix_') for n in hip.SIGNATURES)
    # the limits are the header's macros
    assert mixture._LIB.constants == {'BRV_MIX_ENERGY_CHUNK': 2048, 'BRV_MIX_MAX_PARTS': 512}
    assert (mixture.EN_CHUNK, mixture.MAX_PARTS) == (2048, 512)


# Number arguments that a call would ACCEPT (by position), where all ones would not be: with them as the baseline
# each value refused below is the sole cause of its -1. BAD: the refused value where 0 is a legal one.
BASELINE = {'brv_mix_pack_brirs': {3: 2}, 'brv_mix_partition_mac': {9: 2}}       # pool_len; hrows (an ear pair)
BAD = {'brv_mix_pack_brirs': {6: -1}}                                            # boundary: 0 is legal


def _args(name, fill):
    """Arguments for ``name``: ``fill`` for every pointer but the stream, an accepted value for every number."""
    _, argtypes = mixture.SIGNATURES[name]
    base = BASELINE.get(name, {})
    return [None if i == len(argtypes) - 1 else fill if t is hip._c_ptr else base.get(i, 1)
            for i, t in enumerate(argtypes)]


@pytest.mark.parametrize('name', sorted(EXPORTS - {'brv_mix_version', 'brv_mix_last_error'}))
def test_every_export_refuses_null_and_zero_arguments(name):
    lib = mixture.lib()
    _, argtypes = mixture.SIGNATURES[name]
    buf = ctypes.create_string_buffer(64)            # never read: each call below is refused on the host
    # a known message from another call first, so that each refusal shows it wrote its own
    assert lib.brv_mix_compose(None, None, None, None, None, 0, 0, 0, 0, None) == -1
    sentinel = lib.brv_mix_last_error()
    assert sentinel
    assert getattr(lib, name)(*_args(name, None)) == -1
    null_msg = lib.brv_mix_last_error()
    assert null_msg and b'null' in null_msg
    seen = set()
    for i, t in enumerate(argtypes[:-1]):
        if t is hip._c_ptr:
            continue
        args = _args(name, buf)
        args[i] = BAD.get(name, {}).get(i, 0)
        assert getattr(lib, name)(*args) == -1, (name, i)
        msg = lib.brv_mix_last_error()
        assert msg and msg != null_msg and b'requires' in msg, (name, i, msg)
        seen.add(msg)
    if name == 'brv_mix_pack_brirs':
        assert len(seen) == 2, seen                  # its numbers are checked in two groups: both were hit
    with pytest.raises(RuntimeError, match=name):
        mixture.call(name, *_args(name, None))


def test_partition_count_beyond_the_lds_tile_is_unsupported():
    lib = mixture.lib()
    buf = ctypes.create_string_buffer(64)
    args = _args('brv_mix_partition_mac', buf)
    args[9] = 2                                       # hrows: an ear pair
    args[-2] = mixture.MAX_PARTS + 1
    assert lib.brv_mix_partition_mac(*args) == -2
    assert b'512' in lib.brv_mix_last_error()


# -- PoolMixtureMaker: draws --------------------------------------------------------------------------------------
def _pools(rng):
    speech = [rng.standard_normal(n).astype(np.float32) for n in (900, 1300, 1100)]
    noises = [rng.standard_normal(n).astype(np.float32) for n in (2000, 1500, 400)]
    brirs = [[rng.standard_normal((300, 2)).astype(np.float32) for _ in range(3)],
             [rng.standard_normal((257, 2)).astype(np.float32) for _ in range(2)]]
    return speech, noises, brirs


def test_pool_maker_draws_are_a_function_of_seed_and_epoch(tmp_path):
    speech, noises, brirs = _pools(np.random.default_rng(0))
    kw = dict(speech=speech, noises=noises, brirs=brirs, padding=0.005, diffuse=True, rms_jitter=(-3.0, 3.0))
    a = mixture.PoolMixtureMaker(None, ['mixture', 'foreground'], 16, seed=3, **kw)
    b = mixture.PoolMixtureMaker(None, ['mixture', 'foreground'], 16, seed=3, **kw)
    c = mixture.PoolMixtureMaker(None, ['mixture', 'foreground'], 16, seed=4, **kw)
    assert a.draw(0) == b.draw(0) and a.draw(5) == b.draw(5)
    assert a.draw(0) != a.draw(1) and a.draw(0) != c.draw(0)
    assert a.file_lengths == b.file_lengths == [m['frames'] for m in a.draw(0)]
    n_pad = round(0.005*16000)
    for m in a.draw(2):
        assert m['frames'] == len(speech[m['target']]) + 4*n_pad
        assert 0 <= len(m['noises']) <= 3 and m['angle'] < len(brirs[m['room']])
        for n in m['noises']:                          # a noise segment of the mixture's length fits its file
            assert n['i_start'] + m['frames'] <= len(noises[n['file']])
        assert (m['ndr'] is not None) == bool(m['noises']) and -5 <= m['snr'] <= 10 and -3 <= m['rms_jitter'] <= 3
    # the same pools from a .npz at `path`
    arrays = {f'speech_{i}': x for i, x in enumerate(speech)}
    arrays.update({f'noise_{i}': x for i, x in enumerate(noises)})
    arrays.update({f'brir_{r}_{k}': h for r, room in enumerate(brirs) for k, h in enumerate(room)})
    np.savez(tmp_path/'pools.npz', **arrays)
    d = mixture.PoolMixtureMaker(str(tmp_path/'pools.npz'), ['mixture', 'foreground'], 16, seed=3,
                                 padding=0.005, diffuse=True, rms_jitter=(-3.0, 3.0))
    assert d.draw(1) == a.draw(1)
    with pytest.raises(ValueError, match='unknown source'):
        mixture.PoolMixtureMaker(None, ['mix'], 4, speech=speech, noises=noises, brirs=brirs)


def test_dataset_error_points_at_the_pool_maker():
    from brever_amd import data
    data.set_mixture_maker(None)
    with pytest.raises(NotImplementedError, match='PoolMixtureMaker'):
        data.BreverDataset('nowhere', dynamic_mixing=True)
