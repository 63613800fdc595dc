"""A miniature VoiceBank+DEMAND archive for the tests of scripts/vbdemand_to_brever.py: an outer zip that holds the
four inner zips of 16-bit 48 kHz mono WAVs, noisy = clean + noise, with the directory prefixes, a directory entry
and a stray text member as the public archive has them."""
import io
import struct
import zipfile

import numpy as np

FS = 48000
# (base name, samples): 0.2 - 0.4 s, no length a multiple of 3
TRAIN = [('p226_001', 9601), ('p287_001', 12002), ('p300_001', 14000), ('p300_002', 16001), ('p226_002', 18001),
         ('p300_003', 19199)]
TEST = [('p232_001', 10001), ('p257_001', 11000)]
VAL_SPEAKERS = ('p226', 'p287')


def wav_bytes(pcm, fs=FS, channels=1):
    data = np.asarray(pcm, dtype='<i2').tobytes()
    head = struct.pack('<4sI4s4sIHHIIHH4sI', b'RIFF', 36 + len(data), b'WAVE', b'fmt ', 16, 1, channels, fs,
                       fs*2*channels, 2*channels, 16, b'data', len(data))
    return head + data


def signals(files, seed):
    """{base name: (noisy int16, clean int16)}."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, n in files:
        clean = np.round(0.2*rng.standard_normal(n)*32768)
        noise = np.round(0.05*rng.standard_normal(n)*32768)
        out[name] = ((clean + noise).astype(np.int16), clean.astype(np.int16))
    return out


def inner_zip(folder, items):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w') as z:
        z.writestr(folder + '/', b'')
        z.writestr(folder + '/log.txt', b'not audio')
        for name, pcm in items:
            z.writestr(f'{folder}/{name}.wav', wav_bytes(pcm))
    return buf.getvalue()


def build(path, rename_clean=None, as_directory=False):
    """Write the archive to ``path`` (a zip, or a directory of the inner zips); returns {'train': signals, 'test':
    signals}. ``rename_clean``: (index, new base name) of a clean train member, to break the pairing."""
    import os
    sig = dict(train=signals(TRAIN, 1), test=signals(TEST, 2))
    inner = {}
    for split, suffix, files in (('train', 'trainset_28spk', TRAIN), ('test', 'testset', TEST)):
        for k, kind in enumerate(('noisy', 'clean')):
            items = [(name, sig[split][name][k]) for name, _ in files]
            if kind == 'clean' and split == 'train' and rename_clean is not None:
                items[rename_clean[0]] = (rename_clean[1], items[rename_clean[0]][1])
            inner[f'{kind}_{suffix}_wav.zip'] = inner_zip(f'{kind}_{suffix}_wav', items)
    if as_directory:
        os.makedirs(path, exist_ok=True)
        for name, blob in inner.items():
            with open(os.path.join(path, name), 'wb') as f:
                f.write(blob)
    else:
        with zipfile.ZipFile(path, 'w') as z:
            z.writestr('license_text', b'CC BY 4.0')
            for name, blob in inner.items():
                z.writestr(name, blob)
    return sig


def expected(sig):
    """Per split the list of (base name, noisy int16, clean int16) in member order."""
    is_val = lambda n: n.startswith(VAL_SPEAKERS)                                  # noqa: E731
    train = [(n, *sig['train'][n]) for n, _ in TRAIN if not is_val(n)]
    val = [(n, *sig['train'][n]) for n, _ in TRAIN if is_val(n)]
    test = [(n, *sig['test'][n]) for n, _ in TEST]
    return dict(train=train, val=val, test=test)
