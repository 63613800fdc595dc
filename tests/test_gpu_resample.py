"""The Fourier resampler on the GPU (brever_amd/io.py, libbrever_resample.so) against the reference's recorded output
and the NumPy restatement (tests/resample_ref.py), and scripts/vbdemand_to_brever.py end to end on a miniature
archive. Lengths are the smallest at which each mechanism can break: degenerate and Nyquist cases up and down, odd
and even lengths at both rate pairs, chirp indices whose square passes 2^32, every decomposition of the transform
(rows only; one column level; two, at the odd length just above 2^20).

Measured on an MI355X: rel-L2 error 0 for the three one-sample outputs, 8.5e-17 .. 1.9e-15 otherwise, 0 .. 1.7 times the
yardstick of the same case (the bound is 8 times); no PCM sample differs."""
import os
import subprocess
import sys
import tarfile

import numpy as np
import pytest
import torch

import resample_ref as R
import vbdemand_fixture as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def io():
    from brever_amd import io
    return io


@pytest.fixture(scope='module')
def alone(io):
    """Every case resampled on its own, cold cache: {case: float64 host array}. Computed once."""
    cache = io.ChirpCache()
    return {case: io.resample(R.case_input(case), case[1], case[2], cache=cache) for case in R.CASES}


def test_values_within_8x_the_yardstick(alone):
    z = R.golden()
    worst = 0.0
    for case in R.CASES:
        ref, got = R.reference(case), alone[case]
        assert got.dtype == np.float64 and got.shape == ref.shape, case
        err, yard = R.rel(got, ref), float(z['yard_' + R.case_key(case)])
        print(case, f'rel-L2 {err:.3e} yardstick {yard:.3e}')
        assert err <= 8*yard, (case, err, yard)
        worst = max(worst, err)
    assert worst < 1e-13


def test_pcm_the_files_will_hold_is_the_references(alone):
    total = 0
    for case in R.PCM_CASES:
        ref, got = R.pcm16(R.reference(case)), R.pcm16(alone[case])
        assert np.array_equal(got, ref), (case, int((got != ref).sum()))
        total += ref.size
    assert total > 2e5


def test_ragged_batch_is_bitwise_each_case_alone_cold_and_warm(io, alone):
    cache = io.ChirpCache()
    xs = [R.case_input(c) for c in R.CASES]
    rates = [c[1] for c in R.CASES]
    # one target rate per call: the cases are grouped by it, all lengths and both source rates of a group together
    for new_fs in (16000, 48000):
        idx = [i for i, c in enumerate(R.CASES) if c[2] == new_fs]
        cold = io.resample_batch([xs[i] for i in idx], [rates[i] for i in idx], new_fs, cache=cache)
        hits, misses = cache.hits, cache.misses
        assert misses > 0
        warm = io.resample_batch([xs[i] for i in idx], [rates[i] for i in idx], new_fs, cache=cache)
        assert cache.misses == misses and cache.hits > hits                    # nothing is computed twice
        for i, a, b in zip(idx, cold, warm):
            assert a.is_cuda and a.dtype == torch.float64
            assert np.array_equal(a.cpu().numpy(), alone[R.CASES[i]]), R.CASES[i]
            assert torch.equal(a, b), R.CASES[i]
    # a cache too small for two entries of the class: each half evicts the other's spectrum, the values stay
    small = io.ChirpCache(max_bytes=4*16*8192)
    case = (4801, 48000, 16000, 2)
    assert small.slots(8192) == 1
    for _ in range(2):
        got = io.resample(R.case_input(case), case[1], case[2], cache=small)
        assert np.array_equal(got, alone[case])
    assert small.misses == 8 and small.hits == 0 and small.evictions == 7


def test_properties(io):
    n, m = 4801, 1601
    flat = io.resample(np.full(n, 0.37), 48000, 16000)
    assert flat.shape == (m,) and np.abs(flat - 0.37).max() < 1e-12
    t = np.arange(n)
    for cycles in (1, 37, 799):                                  # below both Nyquist limits (1601/2 = 800.5)
        x = np.sin(2*np.pi*cycles*t/n + 0.3)
        want = np.sin(2*np.pi*cycles*np.arange(m)/m + 0.3)
        assert np.abs(io.resample(x, 48000, 16000) - want).max() < 1e-10, cycles
    up = io.resample(np.sin(2*np.pi*5*np.arange(442)/442), 16000, 48000)
    assert np.abs(up - np.sin(2*np.pi*5*np.arange(1326)/1326)).max() < 1e-10
    x = R.case_input((4802, 48000, 16000, 1))
    same = io.resample(x, 16000, 16000)
    assert same.dtype == np.float64 and np.array_equal(same, x)
    y64 = io.resample_batch([x], 48000, 16000)[0]
    y32 = io.resample_batch([x], 48000, 16000, dtype=torch.float32)[0]
    assert y32.dtype == torch.float32 and torch.equal(y32, y64.to(torch.float32))
    # the kinds: a float32 device tensor gives a float32 device tensor, a host tensor a float64 host tensor
    d32 = io.resample(torch.from_numpy(x).float().cuda(), 48000, 16000)
    assert d32.is_cuda and d32.dtype == torch.float32 and torch.equal(d32, y32)
    h = io.resample(torch.from_numpy(x), 48000, 16000)
    assert not h.is_cuda and h.dtype == torch.float64 and torch.equal(h, y64.cpu())
    two = R.case_input((4801, 48000, 16000, 2))
    assert np.array_equal(io.resample(two.T.copy(), 48000, 16000, axis=1), io.resample(two, 48000, 16000).T)


def test_too_long_a_signal_is_refused_on_the_host(io):
    top = io.max_length()
    assert top >= 1 << 22
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=str(top)):
        io.plan(top + 1, 48000, 16000)
    with pytest.raises(ValueError, match=str(top)):
        io.resample_batch([torch.empty(top + 1, device='meta')], 48000, 16000)
    assert torch.cuda.memory_allocated() == before


def _run(*argv, cwd):
    return subprocess.run([sys.executable, *argv], capture_output=True, text=True, cwd=cwd)


def test_vbdemand_import_end_to_end_and_one_epoch(tmp_path):
    from brever_amd.data import BreverDataset
    sig = V.build(tmp_path/'DS_10283_2791.zip')
    out = str(tmp_path/'datasets')
    script = os.path.join(ROOT, 'scripts', 'vbdemand_to_brever.py')
    argv = [script, '--vbdemand_path', str(tmp_path/'DS_10283_2791.zip'), '--datasets_dir', out, '--batch', '4']
    done = _run(*argv, cwd=tmp_path)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-3000:]
    assert 'resample' in done.stdout and sorted(os.listdir(out)) == ['test', 'train', 'val']
    members = {}
    for split, items in V.expected(sig).items():
        path = os.path.join(out, split, 'vbdemand')
        with tarfile.open(os.path.join(path, 'audio.tar')) as tar:
            members[split] = tar.getnames()
        assert members[split] == [f'audio/{i:05d}_{s}.flac' for s in ('mixture', 'foreground') for i in range(len(items))]
        dset = BreverDataset(path, fs=16000)
        assert len(dset) == len(items)
        for i, (name, noisy, clean) in enumerate(items):
            item = dset[i]
            assert item.shape == (2, 1, -(-len(noisy)//3)) and item.dtype == torch.float32, (split, name)
            for row, pcm in zip(item[:, 0], (noisy, clean)):
                ref = R.pcm16(R.resample(pcm/32768.0, 48000, 16000))
                assert np.array_equal(np.round(row.numpy().astype(np.float64)*32768), ref), (split, name)
    assert [n for n, _, _ in V.expected(sig)['val']] == ['p226_001', 'p287_001', 'p226_002']       # only they
    for extra in ((), ('-f',)):                   # appending adds nothing; writing afresh reproduces the lists
        again = _run(*argv, *extra, cwd=tmp_path)
        assert again.returncode == 0, again.stderr[-3000:]
        for split in members:
            with tarfile.open(os.path.join(out, split, 'vbdemand', 'audio.tar')) as tar:
                assert tar.getnames() == members[split], (split, extra)
    # the imported sets train a tiny Conv-TasNet (the sizes of smoke()) for one epoch
    models = str(tmp_path/'models')
    init = _run('scripts/init_model.py', '--train_path', os.path.join(out, 'train', 'vbdemand'), '--val_path',
                os.path.join(out, 'val', 'vbdemand'), '--preload', 'true', '--workers', '0', '--epochs', '1',
                '--val_period', '1', '--batch_size', '2', '--val_metrics', 'snr', '--models_dir', models,
                'convtasnet', '--filters', '64', '--filter_length', '16', '--bottleneck_channels', '32',
                '--hidden_channels', '64', '--skip_channels', '32', '--layers', '3', '--repeats', '2', cwd=ROOT)
    assert init.returncode == 0, init.stderr[-3000:]
    model_dir = os.path.join(models, os.listdir(models)[0])
    train = _run('scripts/train_model.py', model_dir, cwd=ROOT)
    assert train.returncode == 0, train.stdout[-2000:] + train.stderr[-3000:]
    losses = np.load(os.path.join(model_dir, 'losses.npz'))
    assert np.isfinite(losses['train_loss']).all() and len(losses['train_loss']) == 1
