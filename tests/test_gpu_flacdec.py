"""FLAC members decoded on the GPU (brever_amd/flac_gpu.py, csrc/flacdec/): every comparison is an equality -- with the
integer PCM handed to the test encoder, or with the tensors of the host path. No test feeds the kernel a malformed
payload: tools/flac_core_check.cpp covers that ground on the CPU (tests/test_flacdec_host.py)."""
import os
import random
import subprocess
import sys
import tarfile

import numpy as np
import pytest
import torch

from brever_amd import flac_gpu
from helpers import flac_encode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tests/test_host.py::test_flac_decoder_round_trips
GRID = [
    dict(kind='fixed', order=0), dict(kind='fixed', order=1, stereo='left_side'),
    dict(kind='fixed', order=2, stereo='mid_side', porder=3),
    dict(kind='fixed', order=3, stereo='side_right', five_bit=True),
    dict(kind='fixed', order=4, escape=True), dict(kind='lpc', order=8, stereo='mid_side'),
    dict(kind='lpc', order=12, blocksize=4096, porder=4), dict(kind='verbatim'),
    dict(kind='fixed', order=2, bps=24, porder=0), dict(kind='lpc', order=4, bps=8),
]
EXTRA = [
    dict(kind='lpc', order=1, bps=24, stereo='mid_side'), dict(kind='lpc', order=32, bps=24, stereo='mid_side'),
    dict(kind='fixed', order=2, porder=0), dict(kind='fixed', order=3, porder=8, blocksize=192),   # forced down to 5
    dict(kind='fixed', order=2, five_bit=True, escape=True, stereo='mid_side'),
    dict(kind='fixed', order=1, bps=8), dict(kind='fixed', order=2, bps=12, stereo='left_side'),
    dict(kind='lpc', order=6, bps=20, stereo='side_right'), dict(kind='verbatim', bps=24, stereo='mid_side'),
]


def _recipe(bps, n=5000):
    rng = np.random.default_rng(5)
    t = np.arange(n)
    amp = 2**(bps - 3)
    left = amp*np.sin(2*np.pi*220*t/16000)*(0.6 + 0.4*np.sin(2*np.pi*3*t/16000)) + rng.normal(0, amp/200, n)
    right = 0.8*left + amp/8*np.sin(2*np.pi*950*t/16000) + rng.normal(0, amp/300, n)
    pcm = np.stack([left, right], axis=1).round().astype(np.int64)
    pcm[100:400] = 0                                     # a constant stretch
    pcm[1024:2048] = (pcm[1024:2048] >> 3) << 3          # wasted bits in one block
    return pcm


def _walk(n, channels=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(-300, 300, (n, channels)).cumsum(axis=0).clip(-30000, 30000)


@pytest.fixture(scope='module')
def decoder():
    return flac_gpu.FlacBatchDecoder('cuda')


def _ints(x, bps=16):
    return np.round(x.double().cpu().numpy()*2.0**(bps - 1)).astype(np.int64)


def _check_rows(batch, pcms, bps, windows=None):
    """Row i holds pcms[i] (frames, channels) cut to its window, and exact zeros everywhere else."""
    data = batch.check().data
    for i, pcm in enumerate(pcms):
        start, end = windows[i] if windows is not None else (0, len(pcm))
        assert batch.lengths[i] == end - start
        want = pcm[start:end]
        got = _ints(data[i, 0], bps[i] if isinstance(bps, list) else bps)
        assert np.array_equal(got[:, :len(want)].T, want), i
        assert not data[i, 0, :, len(want):].any(), i         # behind the member: zeros, behind the length too


def test_encoder_grid_as_one_batch(decoder):
    """Every subframe kind, predictor order, decorrelation, parameter width, escape, wasted bits and sample size in
    ONE batch per channel count, so that the kinds diverge inside a wave."""
    for channels in (1, 2):
        members, pcms, widths = [], [], []
        for kw in GRID + EXTRA:
            if channels == 1 and kw.get('stereo', 'independent') != 'independent':
                continue
            bps = kw.get('bps', 16)
            pcm = _recipe(bps)[:, :channels]
            members.append([flac_encode(pcm, **dict(kw, bps=bps))])
            pcms.append(pcm)
            widths.append(bps)
        batch = decoder.decode(members)
        assert batch.data.shape == (len(members), 1, channels, 5000)
        _check_rows(batch, pcms, widths)
        again = decoder.decode(members).check()
        assert torch.equal(again.data, batch.data)               # the same batch twice: bitwise equal
        alone = decoder.decode(members[3:4]).check()
        assert torch.equal(alone.data[0], batch.data[3])           # a member alone = the member inside a batch


def test_long_unary_runs(decoder):
    """Zeros with isolated spikes: Rice parameter 0 or 1 and runs of hundreds of bits, over several window refills."""
    pcm = np.zeros((3000, 1), dtype=np.int64)
    pcm[np.arange(37, 3000, 500), 0] = [700, -650, 900, -700, 650, -900]
    data = flac_encode(pcm, kind='fixed', order=0, porder=0, blocksize=1024)
    assert len(data) < 3000                                  # parameters of 0 / 1 were picked: about a bit a sample
    _check_rows(decoder.decode([[data]]), [pcm], 16)


@pytest.mark.parametrize('n, blocksize', [(1, 16), (15, 16), (16, 16), (17, 16), (191, 192), (193, 192)])
def test_short_files(decoder, n, blocksize):
    pcm = _walk(n, 2, seed=n)
    _check_rows(decoder.decode([[flac_encode(pcm, blocksize=blocksize, stereo='mid_side', order=1)]]), [pcm], 16)


def test_batches_across_wave_edges_and_unaligned_members(decoder):
    one, many = _walk(16, 1, 1), _walk(70*16, 1, 2)
    members = [[flac_encode(one, blocksize=16)], [flac_encode(many, blocksize=16)]]
    _check_rows(decoder.decode(members), [one, many], 16)         # a 1-frame member and a 70-frame member
    pcms = [_walk(65*16 - k, 1, 3 + k) for k in range(3)]          # 3 x 65 frames = 195 jobs
    members = [[flac_encode(p, blocksize=16, order=2, porder=1)] for p in pcms]
    for pads in ((0, 0, 0), (1, 1, 1), (2, 1, 3), (3, 3, 2)):
        batch = decoder.decode(members, pad_offsets=list(pads))
        assert batch.status.numel() == 195
        _check_rows(batch, pcms, 16)
    # the members' starts really were at 1, 2 and 3 modulo 4
    seen = set()
    for pads in ((1, 1, 1), (2, 1, 3), (3, 3, 2)):
        at = 0
        for m, p in zip(members, pads):
            at += p
            seen.add(at % 4)
            at += len(m[0]) - 42
    assert seen >= {1, 2, 3}


def test_a_batch_past_the_wide_group_threshold(decoder):
    """From 4096 jobs on a parse workgroup takes 64 frames instead of 16: 3 x 1400 frames, stereo, the last ones short."""
    pcms = [_walk(1400*16 - 3*k, 2, 20 + k) for k in range(3)]
    members = [[flac_encode(p, blocksize=16, order=1, porder=1, stereo='mid_side')] for p in pcms]
    batch = decoder.decode(members)
    assert batch.status.numel() == 4200
    _check_rows(batch, pcms, 16)


def test_windows(decoder):
    pcm = _walk(1000, 2, 9)
    data = flac_encode(pcm, blocksize=192, stereo='left_side')
    windows = [(200, 300), (300, 500), (900, 1200), (400, 400), (0, 1000), (191, 193)]
    batch = decoder.decode([[data]]*len(windows), windows)
    assert batch.data.shape == (6, 1, 2, 1000) and batch.lengths == [100, 200, 300, 0, 1000, 2]
    _check_rows(batch, [pcm]*len(windows), 16, windows)
    assert not batch.data[2, 0, :, 100:].any()               # the window ends past the file: zeros from sample 100 on
    # only the frames that overlap a window were made into jobs: 1 + 2 + 2 + 0 + 6 + 2
    assert batch.status.numel() == 13


def _stream32(pcm):
    """Mono, one VERBATIM frame, 32 bits per sample (sample size code 7), written with the encoder's own pieces."""
    from helpers import _BitWriter, _crc
    n = len(pcm)
    info = _BitWriter()
    for value, bits in ((n, 16), (n, 16), (0, 24), (0, 24), (16000, 20), (0, 3), (31, 5), (n, 36), (0, 128)):
        info.write(value, bits)
    bw = _BitWriter()
    for value, bits in ((0xfff8 >> 2, 14), (0, 2), (7, 4), (0, 4), (0, 4), (7, 3), (0, 1), (0, 8), (n - 1, 16)):
        bw.write(value, bits)
    bw.write(_crc(bytes(bw.out), 0x07, 8), 8)
    bw.write(1, 7); bw.write(0, 1)
    for v in pcm:
        bw.write(int(v), 32)
    bw.align()
    bw.write(_crc(bytes(bw.out), 0x8005, 16), 16)
    return b'fLaC' + bytes([0x80, 0, 0, 34]) + bytes(info.out) + bytes(bw.out)


def test_a_member_the_index_declines_goes_through_the_host(decoder):
    """32 bits per sample: the index says "not taken", the batch decoder reads the member with the host decoder and
    copies it in, next to a 16-bit member decoded by the kernels."""
    wide = np.random.default_rng(8).integers(-2**31, 2**31, 300)
    pcm = _walk(500, 1, 4)
    with pytest.raises(flac_gpu.FlacIndexError) as e:
        flac_gpu.index(_stream32(wide))
    assert e.value.code == flac_gpu.NOT_TAKEN
    batch = decoder.decode([[_stream32(wide)], [flac_encode(pcm, blocksize=192)]], windows=[(10, 300), None]).check()
    assert batch.lengths == [290, 500] and batch.data.shape == (2, 1, 1, 500)
    assert np.array_equal(batch.data[0, 0, 0, :290].cpu().numpy(), (wide[10:]/2.0**31).astype(np.float32))
    assert not batch.data[0, 0, 0, 290:].any()
    assert np.array_equal(_ints(batch.data[1, 0]).T, pcm)


def _dataset(root, lengths=(3000, 4100)):
    """tests/test_host.py::test_dataset_reads_flac_members: mid/side stereo, two sources, in audio.tar."""
    rng = np.random.default_rng(0)
    os.makedirs(root/'audio')
    for i, n in enumerate(lengths):
        for src in ('mixture', 'foreground'):
            pcm = rng.integers(-2000, 2000, (n, 2)).cumsum(axis=0).clip(-30000, 30000)
            (root/'audio'/f'{i:05d}_{src}.flac').write_bytes(flac_encode(pcm, stereo='mid_side', kind='fixed', order=2))
    with tarfile.open(root/'audio.tar', 'w') as tar:
        tar.add(root/'audio', arcname='audio')
    return str(root)


@pytest.fixture(scope='module')
def dataset_dir(tmp_path_factory):
    return _dataset(tmp_path_factory.mktemp('flacdset')/'dset')


@pytest.mark.parametrize('transform', [None, lambda s: s.mean(axis=-2)], ids=['raw', 'mono'])
@pytest.mark.parametrize('strategy', ['pass', 'drop', 'pad', 'overlap'])
def test_preload_equals_the_host_path(dataset_dir, monkeypatch, strategy, transform):
    from brever_amd.data import BreverDataset
    kw = dict(segment_length=0.08, segment_strategy=strategy, transform=transform)      # 1280 samples: files split
    host, dev = BreverDataset(dataset_dir, **kw), BreverDataset(dataset_dir, **kw)
    assert len(host) == {'pass': 7, 'drop': 5, 'pad': 7, 'overlap': 7}[strategy]
    calls = []
    real = flac_gpu.index
    monkeypatch.setattr(flac_gpu, 'index', lambda blob, name='<bytes>': calls.append(name) or real(blob, name))
    dev.preload('cuda')
    assert sorted(calls) == sorted(p for i in range(2) for p in dev.build_paths(i))       # each member once
    assert len(dev.preloaded_data) == len(host)
    for i in range(len(host)):
        assert dev[i].is_cuda and torch.equal(dev[i].cpu(), host[i]), i


def test_preload_of_members_the_index_declines(tmp_path, monkeypatch):
    """32-bit members in a dataset: indexed once each (not again inside the batch decoder), decoded on the host, equal
    to the host path; their sample rate is still checked against the dataset's."""
    from brever_amd.data import BreverDataset
    root = tmp_path/'wide'
    os.makedirs(root/'audio')
    rng = np.random.default_rng(3)
    for src in ('mixture', 'foreground'):
        (root/'audio'/f'00000_{src}.flac').write_bytes(_stream32(rng.integers(-2**31, 2**31, 700)))
    kw = dict(tar=False, segment_length=0.02, segment_strategy='pass')
    host, dev = BreverDataset(str(root), **kw), BreverDataset(str(root), **kw)
    calls = []
    real = flac_gpu.index
    monkeypatch.setattr(flac_gpu, 'index', lambda blob, name='<bytes>': calls.append(name) or real(blob, name))
    dev.preload('cuda')
    assert len(calls) == 2 and len(host) == 3
    for i in range(len(host)):
        assert dev[i].shape == (2, 1, host[i].shape[-1]) and torch.equal(dev[i].cpu(), host[i]), i
    other = BreverDataset(str(root), **kw)
    other.fs = 8000
    with pytest.raises(ValueError, match='sampling rate'):
        other.preload('cuda')


@pytest.mark.parametrize('strategy', ['pass', 'random'])
def test_prefetcher_decodes_compressed_batches(dataset_dir, strategy):
    from brever_amd.data import BreverDataLoader, BreverDataset, DevicePrefetcher, enable_gpu_decode
    mono = lambda s: s.mean(axis=-2)        # noqa: E731
    kw = dict(segment_length=0.05, segment_strategy=strategy, transform=mono)
    batches = [[0, 3, 5], [1, 2], [4, 6]] if strategy == 'pass' else [[0, 1], [1, 0]]
    out = []
    for gpu in (False, True):
        dset = BreverDataset(dataset_dir, **kw)
        if gpu:
            enable_gpu_decode(dset)
        random.seed(11)
        loader = BreverDataLoader(dset, batch_sampler=batches, num_workers=0)
        out.append([(b.clone(), n.clone()) for b, n in DevicePrefetcher(loader, 'cuda')])
    assert len(out[0]) == len(out[1]) == len(batches)
    for (b0, n0), (b1, n1) in zip(*out):
        assert b0.is_cuda and b1.is_cuda and b0.shape == b1.shape
        assert torch.equal(n0, n1) and torch.equal(b0, b1)


def test_train_model_script_losses_are_the_same_with_gpu_decode(tmp_path, dataset_dir):
    """scripts/train_model.py --gpu_decode on the FLAC dataset, on-the-fly batches, fp32 path (bitwise repeatable): the
    batches are the host path's, so the losses of the epoch are too."""
    def run(*a):
        return subprocess.run([sys.executable, *a], capture_output=True, text=True, cwd=ROOT, timeout=300)
    models = str(tmp_path/'models')
    os.makedirs(models)
    out = run('scripts/init_model.py', '--train_path', dataset_dir, '--val_path', dataset_dir, '--epochs', '1',
              '--val_period', '1', '--batch_size', '1', '--val_metrics', 'snr', '--workers', '0', '--use_amp',
              'false', '--models_dir', models, 'convtasnet', '--filters', '64', '--bottleneck_channels', '32',
              '--hidden_channels', '64', '--skip_channels', '32', '--layers', '2', '--repeats', '1')
    assert out.returncode == 0, out.stderr[-3000:]
    model_dir = os.path.join(models, os.listdir(models)[0])
    losses = []
    for flags in ((), ('--gpu_decode',)):
        out = run('scripts/train_model.py', model_dir, '-f', *flags)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        with np.load(os.path.join(model_dir, 'losses.npz')) as f:
            losses.append({k: f[k].copy() for k in f.files})
    assert set(losses[0]) == set(losses[1]) and 'train_loss' in losses[0]
    for k in losses[0]:
        assert np.isfinite(losses[0][k]).all() and np.array_equal(losses[0][k], losses[1][k]), k
