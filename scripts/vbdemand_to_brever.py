"""Import VoiceBank+DEMAND as ``<DATASETS>/{train,val,test}/vbdemand/audio.tar``.

Same command line as the reference (scripts/vbdemand_to_brever.py): ``-f/--force``, ``--vbdemand_path``,
``--val_speakers`` (default ``p226 p287``). Every 48 kHz file is resampled to 16 kHz over the whole signal
(``brever_amd.io.resample_batch``: the reference's ``brever.io.resample`` on the GPU) and stored as mono 16-bit
FLAC: ``audio/NNNNN_mixture.flac`` from ``noisy_*_wav.zip``, ``audio/NNNNN_foreground.flac`` from
``clean_*_wav.zip``; ``train`` and ``val`` share ``*_trainset_28spk_wav.zip`` and are split by the speaker prefix
of the file name, ``test`` is ``*_testset_wav.zip``. Without ``-f`` an existing archive is appended to and members
already present are skipped; an unreadable archive is recreated.

Differences, on purpose: ``--vbdemand_path`` is the public ``DS_10283_2791.zip`` or a directory that holds its
four inner zips; nothing is ever downloaded (without ``--vbdemand_path`` the script says which archive to obtain
and exits); ``--datasets_dir DIR`` overrides ``DATASETS`` of ``config/paths.yaml``; ``--batch N`` files are
decoded, resampled and encoded together; members are written from memory; decoding and encoding run on at most
``min(16, os.cpu_count())`` host threads."""
import argparse
import concurrent.futures
import io
import os
import tarfile
import threading
import time
import zipfile

# read when the HIP runtime loads (torch import): see brever_amd/__init__.py
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

from _common import ROOT  # noqa: E402,F401

FS = 16000
ARCHIVE = 'DS_10283_2791.zip'
SPLITS = (('train', 'trainset_28spk'), ('val', 'trainset_28spk'), ('test', 'testset'))
SOURCES = (('noisy', 'mixture'), ('clean', 'foreground'))


def keep(name, split, val_speakers):
    """Whether member ``name`` of an inner zip belongs to ``split``."""
    if not name.endswith('.wav'):
        return False
    if split == 'test':
        return True
    is_val = any(os.path.basename(name).startswith(spk) for spk in val_speakers)
    return is_val == (split == 'val')


def open_inner(vbdemand_path, zip_name):
    """The inner zip ``zip_name`` of the outer archive, or of a directory that holds the inner zips."""
    if os.path.isdir(vbdemand_path):
        return zipfile.ZipFile(os.path.join(vbdemand_path, zip_name))
    with zipfile.ZipFile(vbdemand_path, 'r') as outer:
        return zipfile.ZipFile(io.BytesIO(outer.read(zip_name)))


def open_archive(path, force):
    if force:
        return tarfile.open(path, 'w')
    try:
        return tarfile.open(path, 'a')
    except tarfile.ReadError:
        print('output archive is corrupted, recreating...')
        return tarfile.open(path, 'w')


def _resample(xs, rates):
    """The batch at 16 kHz, float64 host arrays (the tests replace this with the NumPy restatement)."""
    from brever_amd.io import resample_batch
    return [y.cpu().numpy() for y in resample_batch(xs, rates, FS)]


def _decode(inner, lock, name):
    from brever_amd.data import audio_read
    with lock:                                   # a ZipFile has one file position
        blob = inner.read(name)
    x, fs = audio_read(io.BytesIO(blob), name)
    if x.ndim != 1:
        raise ValueError(f'{name}: {x.shape[1]} channels; the dataset and the FLAC encoder are mono')
    return x, fs


def _encode(y):
    from brever_amd.data import flac_bytes
    return flac_bytes(y, FS)


def convert(args):
    """Write the three archives; returns the seconds spent decoding, resampling and encoding."""
    if args.datasets_dir:
        dsets_dir = args.datasets_dir
    else:
        from brever_amd.config import _resolve, get_config
        dsets_dir = get_config(_resolve('config/paths.yaml')).DATASETS
    shares = dict(decode=0.0, resample=0.0, encode=0.0)
    threads = max(1, min(16, os.cpu_count() or 1))
    lock = threading.Lock()
    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        for split, suffix in SPLITS:
            archive_path = os.path.join(dsets_dir, split, 'vbdemand', 'audio.tar')
            os.makedirs(os.path.dirname(archive_path), exist_ok=True)
            archive = open_archive(archive_path, args.force)
            try:
                present = set(archive.getnames())
                wav_names = []
                for (noisy_or_clean, source), first in zip(SOURCES, (True, False)):
                    zip_name = f'{noisy_or_clean}_{suffix}_wav.zip'
                    print(f'reading {zip_name}...')
                    with open_inner(args.vbdemand_path, zip_name) as inner:
                        names = [n for n in inner.namelist() if keep(n, split, args.val_speakers)]
                        if first:
                            wav_names = names
                        for i, name in enumerate(names):
                            if i >= len(wav_names) or os.path.basename(name) != os.path.basename(wav_names[i]):
                                other = wav_names[i] if i < len(wav_names) else None
                                raise ValueError(f'{zip_name}: member {i} is {name}, the noisy archive has {other}')
                        todo = [(os.path.join('audio', f'{i:05d}_{source}.flac'), name)
                                for i, name in enumerate(names)]
                        todo = [t for t in todo if t[0] not in present]
                        for at in range(0, len(todo), args.batch):
                            chunk = todo[at:at + args.batch]
                            t0 = time.perf_counter()
                            decoded = list(pool.map(lambda t: _decode(inner, lock, t[1]), chunk))
                            t1 = time.perf_counter()
                            ys = _resample([x for x, _ in decoded], [fs for _, fs in decoded])
                            t2 = time.perf_counter()
                            blobs = list(pool.map(_encode, ys))
                            t3 = time.perf_counter()
                            shares['decode'] += t1 - t0
                            shares['resample'] += t2 - t1
                            shares['encode'] += t3 - t2
                            for (arcname, _), blob in zip(chunk, blobs):
                                info = tarfile.TarInfo(arcname)
                                info.size, info.mtime = len(blob), int(time.time())
                                archive.addfile(info, io.BytesIO(blob))
                    print(f'done: {len(todo)} written, {len(names) - len(todo)} already present.')
            finally:
                archive.close()
    return shares


def main(argv=None):
    parser = argparse.ArgumentParser(description='convert VoiceBank+DEMAND to the dataset layout')
    parser.add_argument('-f', '--force', action='store_true')
    parser.add_argument('--vbdemand_path')
    parser.add_argument('--val_speakers', nargs='+', default=['p226', 'p287'])
    parser.add_argument('--datasets_dir', help='(extension) write here instead of paths.DATASETS')
    parser.add_argument('--batch', type=int, default=64, help='(extension) files per batch')
    args = parser.parse_args(argv)
    if args.vbdemand_path is None:
        raise SystemExit(f'--vbdemand_path is required: this build never downloads anything. Obtain {ARCHIVE} '
                         '(VoiceBank+DEMAND, Edinburgh DataShare, DS_10283_2791) and pass its path, or the '
                         'directory that holds its four inner *_wav.zip archives.')
    if args.batch < 1:
        raise SystemExit('--batch must be at least 1')
    shares = convert(args)
    total = sum(shares.values()) or 1.0
    print('host decode {:.2f} s ({:.0%}), resample {:.2f} s ({:.0%}), host encode {:.2f} s ({:.0%})'.format(
        shares['decode'], shares['decode']/total, shares['resample'], shares['resample']/total,
        shares['encode'], shares['encode']/total))


if __name__ == '__main__':
    main()
