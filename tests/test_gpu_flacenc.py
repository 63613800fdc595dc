"""Batches encoded as FLAC on the GPU (brever_amd/flac_enc.py, csrc/flacenc/) and datasets written with them
(PoolMixtureMaker.write_dataset, scripts/create_dataset.py). The comparators are never the code under test: the host
decoder brv_flac_decode, the strict host index brv_flacdec_index, the GPU decoder FlacBatchDecoder and the NumPy
restatement of the decision rule (tests/flacenc_ref.py). Every comparison of samples is an equality of integers."""
import io
import os
import subprocess
import sys
import tarfile

import numpy as np
import pytest
import torch

import flacenc_ref
from brever_amd import flac_enc, flac_gpu
from helpers import run_entry_points

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'


@pytest.fixture(scope='module')
def encoder():
    return flac_enc.FlacBatchEncoder(DEV)


@pytest.fixture(scope='module')
def decoder():
    return flac_gpu.FlacBatchDecoder(DEV)


def _resonance(n, seed, freq=3000.0, fs=16000, amp=0.05):
    """Seeded speech-like noise: white noise through an AR(2) resonance at ``freq``."""
    import scipy.signal
    rng = np.random.default_rng(seed)
    r = 0.95
    y = scipy.signal.lfilter([1.0], [1.0, -2*r*np.cos(2*np.pi*freq/fs), r*r], rng.standard_normal(n + 64))
    return (amp*y[64:]).astype(np.float32)


def _two_tones(n=4096):
    t = np.arange(n)
    return (0.4*np.sin(2*np.pi*5000*t/16000) + 0.3*np.sin(2*np.pi*6500*t/16000 + 1)).astype(np.float32)


def _host_decode(data, bps):
    from brever_amd.data import audio_read
    x, rate = audio_read(io.BytesIO(data), 'x.flac')
    x = np.asarray(x, dtype=np.float64)
    x = x[None, :] if x.ndim == 1 else x.T
    return np.round(x*2.0**(bps - 1)).astype(np.int64), rate


def _pad(rows, channels):
    """(tensor (B, C, Lmax) float32 on the device, lengths) of host rows (C, n)."""
    lmax = max(r.shape[1] for r in rows)
    x = np.zeros((len(rows), channels, lmax), dtype=rows[0].dtype)
    for i, r in enumerate(rows):
        x[i, :, :r.shape[1]] = r
    return torch.from_numpy(x).to(DEV), [r.shape[1] for r in rows]


def _check_streams(streams, want, bps, block, decoder, rate=16000):
    """Every stream through the three comparators: exactly the integers of ``want`` (rows (C, n))."""
    for i, (data, pcm) in enumerate(zip(streams, want)):
        info, frames = flac_gpu.index(data, f'row {i}')
        assert (info['sample_rate'], info['channels'], info['bits_per_sample'], info['total_samples']) == \
            (rate, pcm.shape[0], bps, pcm.shape[1]), i
        assert len(frames) == -(-pcm.shape[1]//block), i
        assert frames[:, 3].tolist() == [min(block, pcm.shape[1] - s) for s in range(0, pcm.shape[1], block)]
        assert frames[:, 7].tolist() == list(range(len(frames)))
        # STREAMINFO: the nominal block size twice, the frames' least and largest size
        assert int.from_bytes(data[8:10], 'big') == int.from_bytes(data[10:12], 'big') == block
        assert int.from_bytes(data[12:15], 'big') == frames[:, 1].min()
        assert int.from_bytes(data[15:18], 'big') == frames[:, 1].max()
        assert data[26:42] == bytes(16) and int(frames[-1, 0] + frames[-1, 1]) == len(data)
        got, got_rate = _host_decode(data, bps)
        assert got_rate == rate and np.array_equal(got, pcm), i
    batch = decoder.decode([[s] for s in streams]).check()
    assert batch.lengths == [p.shape[1] for p in want]
    ints = np.round(batch.data[:, 0].double().cpu().numpy()*2.0**(bps - 1)).astype(np.int64)
    for i, pcm in enumerate(want):
        assert np.array_equal(ints[i, :, :pcm.shape[1]], pcm), i


# -- 1. lossless ---------------------------------------------------------------------------------------------------
def _grid_rows(channels, block):
    rows = []
    lengths = [1, 15, 16, 17, 3*block, 3*block + 5]
    for k, n in enumerate(lengths):
        res = np.stack([_resonance(n, seed=10*k + c, freq=3000.0 - 900*c) for c in range(channels)])
        rng = np.random.default_rng(100 + k)
        rows.append(res)                                                   # speech-like noise
        rows.append(np.zeros((channels, n), dtype=np.float32))             # digital silence
        rows.append(np.full((channels, n), 0.25, dtype=np.float32))        # a constant
        rows.append(np.where(rng.random((channels, n)) < 0.5, 1.0, -1.0).astype(np.float32))   # +-1.0: +1.0 clips
        rows.append(rng.uniform(-1, 1, (channels, n)).astype(np.float32))  # full-scale white noise
        if channels == 2:
            rows.append(np.stack([res[0], res[0]]))                        # identical channels
            rows.append(np.stack([res[0], -res[0]]))                       # anti-phase channels
    return rows


@pytest.mark.parametrize('block', [16, 192, 256, 4096])
@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('bps', [16, 24])
def test_lossless_grid(encoder, decoder, bps, channels, block):
    """Lengths 1 (shorter than every predictor order), 15, 16, 17, three blocks, three blocks and 5, each with every
    signal, in one batch; then the same through the int32 PCM entry with both range ends."""
    rows = _grid_rows(channels, block)
    x, lengths = _pad(rows, channels)
    streams = encoder.encode(x, lengths, bits_per_sample=bps, block_size=block)
    want = [flacenc_ref.quantise(r, bps) for r in rows]
    assert any((w == 2**(bps - 1) - 1).any() for w in want) and any((w == -2**(bps - 1)).any() for w in want)
    _check_streams(streams, want, bps, block, decoder)
    # int32 PCM: alternating range ends, random full-range samples, and the quantised resonance
    full = 2**(bps - 1)
    rng = np.random.default_rng(bps + channels + block)
    n = 3*block + 5
    pcm = [np.where((np.arange(n) + np.arange(channels)[:, None]) % 2 == 0, full - 1, -full),
           rng.integers(-full, full, (channels, n)), want[-5 if channels == 1 else -7], np.full((channels, 17), -full)]
    xp, lengths = _pad([p.astype(np.int32) for p in pcm], channels)
    streams = encoder.encode(xp, lengths, bits_per_sample=bps, block_size=block, pcm=True)
    _check_streams(streams, pcm, bps, block, decoder)


def test_a_block_longer_than_the_staged_samples(encoder, decoder):
    """The kernel keeps the first 4096 samples of a coded channel in LDS and reads the rest from the input: a block
    of 5000, stereo, 24 bits, two blocks and 7 samples."""
    n = 2*5000 + 7
    rows = [np.stack([_resonance(n, seed=1), _resonance(n, seed=2, freq=800.0)]), np.stack([_two_tones(n)]*2)]
    x, lengths = _pad(rows, 2)
    streams = encoder.encode(x, lengths, bits_per_sample=24, block_size=5000)
    _check_streams(streams, [flacenc_ref.quantise(r, 24) for r in rows], 24, 5000, decoder)


# -- 2. long streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frames', [130, 2100])
def test_long_streams_code_their_frame_numbers_in_two_and_three_bytes(encoder, decoder, frames):
    n = 16*frames - 3
    rows = [_resonance(n, seed=frames)[None]]
    x, lengths = _pad(rows, 1)
    data = encoder.encode(x, lengths, block_size=16)[0]
    table = flac_gpu.index(data)[1]
    assert len(table) == frames
    # header bytes: 4 + the coded number + the 8-bit block size (16 and 13 have no code of their own) + CRC-8
    assert table[:, 6].tolist() == [4 + flacenc_ref.number_bytes(k) + 1 + 1 for k in range(frames)]
    assert {flacenc_ref.number_bytes(k) for k in range(frames)} == ({1, 2} if frames == 130 else {1, 2, 3})
    _check_streams([data], [flacenc_ref.quantise(rows[0], 16)], 16, 16, decoder)


# -- 3. the choice is the minimum ------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', [16, 64])
@pytest.mark.parametrize('bps', [16, 24])
def test_every_frame_is_the_brute_force_minimum(encoder, decoder, bps, block):
    pcm = np.concatenate(flacenc_ref.decision_blocks(bps, block, seed=bps + block), axis=1)
    rows = [pcm, pcm[:1], pcm[1:]]
    plain, with_lpc = [], []
    for group in ([pcm], [pcm[:1], pcm[1:]]):
        x, lengths = _pad([g.astype(np.int32) for g in group], group[0].shape[0])
        plain += encoder.encode(x, lengths, bits_per_sample=bps, block_size=block, lpc_order=0, pcm=True)
        with_lpc += encoder.encode(x, lengths, bits_per_sample=bps, block_size=block, lpc_order=8, pcm=True)
    kinds, assignments = set(), set()
    for data, lpc_data, row in zip(plain, with_lpc, rows):
        want = flacenc_ref.stream_frame_bytes(row, bps, block)
        frames = flac_gpu.index(data)[1]
        assert frames[:, 1].tolist() == [w[0] for w in want]
        assert frames[:, 4].tolist() == [w[1] for w in want]
        for _, assignment, ks in want:
            assignments.add(assignment)
            kinds.update(ks)
        lpc_frames = flac_gpu.index(lpc_data)[1]
        assert (lpc_frames[:, 1] <= frames[:, 1]).all()
    # each subframe type and each channel assignment wins at least once
    assert assignments == {0, 1, 8, 9, 10}
    assert {'constant', 'verbatim'} <= kinds and len({k for k in kinds if k.startswith('fixed')}) >= 3
    _check_streams(plain[:1] + with_lpc[:1], [pcm, pcm], bps, block, decoder)
    _check_streams(plain[1:] + with_lpc[1:], rows[1:] + rows[1:], bps, block, decoder)


# -- 4. against the host encoder -------------------------------------------------------------------------------------
def test_stream_is_no_larger_than_the_host_encoders(encoder, decoder):
    from brever_amd.data import flac_bytes
    x = _resonance(3*4096 - 100, seed=4)
    host = flac_bytes(x, 16000)
    assert len(flac_gpu.index(host)[1]) == 3
    mine = encoder.encode(torch.from_numpy(x)[None].to(DEV), lpc_order=0)[0]
    with_lpc = encoder.encode(torch.from_numpy(x)[None].to(DEV))[0]
    assert len(with_lpc) <= len(mine) <= len(host)
    _check_streams([mine, with_lpc], [flacenc_ref.quantise(x, 16)[None]]*2, 16, 4096, decoder)
    assert np.array_equal(_host_decode(host, 16)[0], flacenc_ref.quantise(x, 16)[None])


# -- 5. LPC earns its place --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bps', [16, 24])
def test_lpc_codes_two_tones_strictly_smaller(encoder, decoder, bps):
    x = torch.from_numpy(_two_tones())[None].to(DEV)
    plain = encoder.encode(x, bits_per_sample=bps, lpc_order=0)[0]
    lpc = encoder.encode(x, bits_per_sample=bps, lpc_order=8)[0]
    assert len(lpc) < len(plain)
    _check_streams([plain, lpc], [flacenc_ref.quantise(_two_tones(), bps)[None]]*2, bps, 4096, decoder)


def test_lpc_codes_a_resonance_strictly_smaller(encoder):
    x = torch.from_numpy(_resonance(4096, seed=1, amp=0.02))[None].to(DEV)
    assert len(encoder.encode(x, lpc_order=8)[0]) < len(encoder.encode(x, lpc_order=0)[0])


# -- 6. repeatable and batch-independent -------------------------------------------------------------------------------
def test_bytes_are_repeatable_and_do_not_depend_on_the_batch(encoder):
    rows = [np.stack([_resonance(n, seed=n), _resonance(n, seed=n + 1, freq=1200.0)]) for n in (700, 33, 1, 515, 256)]
    x, lengths = _pad(rows, 2)
    first = encoder.encode(x, lengths, block_size=256)
    assert encoder.encode(x, lengths, block_size=256) == first
    assert encoder.encode(x, torch.tensor(lengths), block_size=256) == first
    for i in (0, 2, 3):
        alone = encoder.encode(torch.from_numpy(rows[i])[None].to(DEV), block_size=256)
        assert alone == [first[i]], i
    # two batches in flight, results taken in the other order
    a = encoder.submit(x, lengths, block_size=256)
    b = encoder.submit(x[:2], lengths[:2], block_size=256)
    assert b.result() == first[:2] and a.result() == first
    # (B, L) is mono
    mono = encoder.encode(x[:, 0], lengths, block_size=256)
    assert mono == encoder.encode(x[:, :1], lengths, block_size=256) and flac_gpu.index(mono[0])[0]['channels'] == 1


# -- 7. statuses -----------------------------------------------------------------------------------------------------------
def test_refused_rows_have_a_status_and_the_others_are_correct(encoder, decoder):
    rows = [_resonance(300, seed=k)[None] for k in range(4)]
    bad = [r.copy() for r in rows]
    bad[1][0, 299] = np.nan
    bad[3][0, 0] = np.inf
    x, lengths = _pad(bad, 1)
    with pytest.raises(ValueError, match='row 1 .*non-finite'):
        encoder.encode(x, lengths, block_size=64)
    pending = encoder.submit(x, lengths, block_size=64)
    streams = pending.result(check=False)
    assert pending.status == [0, 1, 0, 1] and streams[1] is None and streams[3] is None
    _check_streams([streams[0], streams[2]], [flacenc_ref.quantise(rows[k], 16) for k in (0, 2)], 16, 64, decoder)
    # int32 PCM one beyond the range, at either end; a length beyond the padded length
    pcm = np.zeros((4, 1, 100), dtype=np.int32)
    pcm[:, 0] = np.arange(100)
    pcm[0, 0, 50], pcm[2, 0, 99] = 32768, -32769
    xp = torch.from_numpy(pcm).to(DEV)
    with pytest.raises(ValueError, match='row 0 .*range'):
        encoder.encode(xp, pcm=True, block_size=16)
    pending = encoder.submit(xp, [100, 100, 100, 101], pcm=True, block_size=16)
    streams = pending.result(check=False)
    assert pending.status == [2, 0, 2, 4] and [s is None for s in streams] == [True, False, True, True]
    assert np.array_equal(_host_decode(streams[1], 16)[0], pcm[1])
    # 24 bits take what 16 bits refuse
    assert encoder.submit(xp, pcm=True, bits_per_sample=24, block_size=16).status == [0, 0, 0, 0]
    with pytest.raises(ValueError, match='float32'):
        encoder.encode(xp)
    with pytest.raises(ValueError, match='block_size'):
        encoder.encode(x, block_size=8)


# -- 8. datasets -----------------------------------------------------------------------------------------------------------
def _pools():
    speech = [_resonance(n, seed=n, amp=0.03) for n in (1900, 2301, 1500)]
    noises = [_resonance(n, seed=n, freq=700.0, amp=0.03) for n in (5000, 4100)]
    rng = np.random.default_rng(11)
    brirs = [[(0.05*rng.standard_normal((t, 2))).astype(np.float32) for t in (300, 257)]]
    for h in brirs[0]:
        h[10, 0], h[14, 1] = 1.0, 0.8
    return dict(speech=speech, noises=noises, brirs=brirs)


def _members(path):
    with tarfile.open(path) as tar:
        return {m.name: tar.extractfile(m).read() for m in tar.getmembers()}


@pytest.mark.parametrize('bps', [16, 24])
def test_write_dataset_round_trips_through_the_dataset(tmp_path, bps):
    import json
    from brever_amd import mixture
    from brever_amd.data import BreverDataset
    sources = ['mixture', 'foreground']
    kw = dict(seed=3, noise_count=(1, 2), batch=2, device=DEV, **_pools())
    maker = mixture.PoolMixtureMaker(None, sources, 5, **kw)
    for name in ('a', 'b'):
        seconds = maker.write_dataset(str(tmp_path/name), epoch=1, bits_per_sample=bps, block_size=1024)
        assert set(seconds) == {'synthesis', 'encode', 'wait', 'copy', 'write'}
    assert (tmp_path/'a'/'audio.tar').read_bytes() == (tmp_path/'b'/'audio.tar').read_bytes()
    assert (tmp_path/'a'/'mixture_info.json').read_bytes() == (tmp_path/'b'/'mixture_info.json').read_bytes()
    members = _members(tmp_path/'a'/'audio.tar')
    assert sorted(members) == sorted(f'audio/{i:05d}_{s}.flac' for i in range(5) for s in sources)
    with open(tmp_path/'a'/'mixture_info.json') as f:
        info = json.load(f)
    assert info == json.loads(json.dumps(maker.draw(1))) and len(info) == 5
    # the directory form holds the same members
    maker.write_dataset(str(tmp_path/'c'), epoch=1, bits_per_sample=bps, tar=False, block_size=1024)
    assert not (tmp_path/'c'/'audio.tar').exists()
    assert {f'audio/{n}': (tmp_path/'c'/'audio'/n).read_bytes() for n in os.listdir(tmp_path/'c'/'audio')} == members
    # the dataset's items against the maker's own
    maker.set_epoch(1)
    host = BreverDataset(str(tmp_path/'a'))
    dev = BreverDataset(str(tmp_path/'a'))
    dev.preload(DEV)                                         # decodes on the GPU
    assert len(host) == 5
    full = 2.0**(bps - 1)
    for i in range(5):
        item = host[i]
        assert torch.equal(dev[i].cpu(), item)
        for k in range(len(sources)):
            want = maker[i][k].T.astype(np.float64)          # (2, frames)
            rounded = np.clip(np.rint(want*full), -full, full - 1)/full
            assert item[k].shape == want.shape
            assert np.array_equal(item[k].double().numpy(), rounded)       # bit equality with the rounded floats
            if bps == 16:
                assert np.abs(item[k].double().numpy() - np.clip(want, -1, 1 - 1/full)).max() <= 2.0**-16
    # another epoch or seed is another archive
    maker.write_dataset(str(tmp_path/'d'), epoch=2, bits_per_sample=bps, block_size=1024)
    assert (tmp_path/'d'/'audio.tar').read_bytes() != (tmp_path/'a'/'audio.tar').read_bytes()


def test_create_dataset_script_feeds_training(tmp_path):
    pools = _pools()
    arrays = {f'speech_{i}': x for i, x in enumerate(pools['speech'])}
    arrays.update({f'noise_{i}': x for i, x in enumerate(pools['noises'])})
    arrays.update({f'brir_0_{a}': h for a, h in enumerate(pools['brirs'][0])})
    np.savez(tmp_path/'pools.npz', **arrays)
    dset = tmp_path/'dset'
    cmd = [sys.executable, 'scripts/create_dataset.py', '--pool', str(tmp_path/'pools.npz'), '--output', str(dset),
           '--size', '5', '--sources', 'mixture', 'foreground', '--seed', '3', '--epoch', '1', '--noise_count', '1', '2',
           '--batch', '2', '--block_size', '1024']
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert '5 mixtures' in out.stdout
    # the maker of the test above with the same options: the same archive
    from brever_amd import mixture
    maker = mixture.PoolMixtureMaker(None, ['mixture', 'foreground'], 5, seed=3, noise_count=(1, 2), batch=2,
                                     device=DEV, **pools)
    maker.write_dataset(str(tmp_path/'direct'), epoch=1, block_size=1024)
    assert (dset/'audio.tar').read_bytes() == (tmp_path/'direct'/'audio.tar').read_bytes()
    again = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert again.returncode != 0 and 'already exists' in again.stderr
    _, losses, scores = run_entry_points(
        tmp_path, 'ffnn', model_args=['--hidden_layers', '64,64'],
        trainer_args=['--epochs', '1', '--val_period', '1', '--batch_size', '4', '--val_metrics', 'snr'],
        train=dset, val=dset, test=dset)
    assert np.isfinite(losses['train_loss']).all() and np.isfinite(scores).all() and scores.shape[0] == 5
