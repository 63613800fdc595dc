"""Throughput of the Fourier resampler (brever_amd/io.py) and of scipy.signal.resample on this machine's CPU.

    python tools/resample_bench.py [--batch 64] [--steps 5] [--warmup 1] [--no-scipy] [--no-shares]

One JSON line per configuration: 64 signals of 4 - 10 s (every length different, as the files of a corpus are) from
48 kHz and from 44.1 kHz to 16 kHz, with a cold chirp cache (every call computes its 2 x batch chirp spectra) and a
warm one; the same signals through ``scipy.signal.resample`` on one CPU thread (what the reference does, one file at
a time); and the three shares of a conversion as scripts/vbdemand_to_brever.py runs it: WAV decoding and FLAC
encoding on at most 16 host threads, resampling on the GPU."""
import argparse
import concurrent.futures
import io as pyio
import json
import os
import struct
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '1')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from brever_amd import io  # noqa: E402


def signals(batch, fs, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(4*fs, 10*fs, size=batch)
    return [np.round(0.1*rng.standard_normal(n)*32768)/32768 for n in lengths]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0)/steps


def wav_bytes(x, fs):
    data = np.round(x*32768).astype('<i2').tobytes()
    return struct.pack('<4sI4s4sIHHIIHH4sI', b'RIFF', 36 + len(data), b'WAVE', b'fmt ', 16, 1, 1, fs, fs*2, 2, 16,
                       b'data', len(data)) + data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-scipy', action='store_true')
    ap.add_argument('--no-shares', action='store_true')
    args = ap.parse_args()
    for fs in (48000, 44100):
        xs = signals(args.batch, fs, fs)
        seconds = sum(len(x) for x in xs)/fs
        dev = [torch.from_numpy(x).cuda() for x in xs]
        common = dict(old_fs=fs, new_fs=16000, batch=args.batch, audio_seconds=round(seconds, 1),
                      classes=sorted({io.plan(len(x), fs, 16000)[1] for x in xs}))
        for cache_state in ('cold', 'warm'):
            cache = io.ChirpCache()

            def run():
                if cache_state == 'cold':
                    cache.clear()
                io.resample_batch(dev, fs, 16000, cache=cache)
            t = timed(run, args.steps, args.warmup)
            print(json.dumps(dict(metric='signals_per_s', value=args.batch/t, ms_per_batch=1e3*t, cache=cache_state,
                                  where='gpu, inputs on the device', **common)), flush=True)
        t = timed(lambda: [y.cpu() for y in io.resample_batch(xs, fs, 16000)], args.steps, args.warmup)
        print(json.dumps(dict(metric='signals_per_s', value=args.batch/t, ms_per_batch=1e3*t, cache='warm',
                              where='gpu, host arrays in and out', **common)), flush=True)
        if not args.no_scipy:
            import scipy.signal
            t0 = time.perf_counter()
            for x in xs:
                scipy.signal.resample(x, io.out_length(len(x), fs, 16000))
            t = time.perf_counter() - t0
            print(json.dumps(dict(metric='signals_per_s', value=args.batch/t, ms_per_batch=1e3*t,
                                  where='scipy.signal.resample, one CPU thread', **common)), flush=True)
        if not args.no_shares and fs == 48000:
            from brever_amd.data import audio_read, flac_bytes
            blobs = [wav_bytes(x, fs) for x in xs]
            threads = max(1, min(16, os.cpu_count() or 1))
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                t0 = time.perf_counter()
                decoded = list(pool.map(lambda b: audio_read(pyio.BytesIO(b), 'a.wav')[0], blobs))
                t1 = time.perf_counter()
                ys = [y.cpu().numpy() for y in io.resample_batch(decoded, fs, 16000)]
                t2 = time.perf_counter()
                flac = list(pool.map(lambda y: flac_bytes(y, 16000), ys))
                t3 = time.perf_counter()
            print(json.dumps(dict(metric='conversion_shares_s', decode=t1 - t0, resample=t2 - t1, encode=t3 - t2,
                                  threads=threads, flac_bytes=sum(len(f) for f in flac), **common)), flush=True)


if __name__ == '__main__':
    main()
