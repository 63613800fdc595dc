"""FLAC decoding, host against GPU, on members written by ``brv_flac_encode16`` (mono, 16 bits,
4096-sample blocks: the project's own format):

    python tools/flac_bench.py [--seconds 4] [--items 16] [--members 4096] [--reps 20] [--warmup 3]

One JSON line per measurement, each the median of ``--reps`` synchronised runs after ``--warmup``:
  host_decode          brv_flac_decode, one process: seconds of audio per second (the parent's path, the yardstick)
  host_index           brv_flacdec_index alone, one process
  gpu_batch            items x 2 members: the two kernels alone (events), the whole decode() call with the tables
                       given (job table, pinned upload, kernels) and with the index included
  gpu_preload          --members members in chunks of the preload byte budget, tables given, upload included
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brever_amd import flac_gpu                                     # noqa: E402
from brever_amd.data import BreverDataset, audio_read, flac_bytes   # noqa: E402


def member(seed, n, fs=16000):
    """A speech-like signal: a modulated harmonic tone plus noise, with a pause."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)/fs
    f0 = 110 + 40*rng.random()
    x = sum(0.25/k*np.sin(2*np.pi*k*f0*t + rng.random()) for k in range(1, 9))
    x = x*(0.5 + 0.5*np.sin(2*np.pi*(2 + rng.random())*t)) + 0.01*rng.standard_normal(n)
    x[n//3:n//3 + n//16] = 0.001*rng.standard_normal(n//16)
    return flac_bytes(0.5*x, fs)


def median_time(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=4.0)
    ap.add_argument('--items', type=int, default=16)
    ap.add_argument('--members', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    n = int(args.seconds*16000)
    pool = [member(s, n) for s in range(8)]
    size = statistics.mean(len(b) for b in pool)

    def line(metric, **kw):
        print(json.dumps(dict(metric=metric, member_seconds=args.seconds, member_bytes=round(size), **kw)), flush=True)

    t = median_time(lambda: [audio_read(io.BytesIO(b), 'm.flac') for b in pool], args.reps, args.warmup, False)
    line('host_decode', audio_s_per_s=len(pool)*args.seconds/t, ms_per_member=1e3*t/len(pool))
    t = median_time(lambda: [flac_gpu.index(b) for b in pool], args.reps, args.warmup, False)
    line('host_index', audio_s_per_s=len(pool)*args.seconds/t, ms_per_member=1e3*t/len(pool))
    if not torch.cuda.is_available():
        return
    dec = flac_gpu.FlacBatchDecoder('cuda')
    members = [[pool[(2*i) % 8], pool[(2*i + 1) % 8]] for i in range(args.items)]
    tables = [[flac_gpu.index(b) for b in row] for row in members]
    audio = 2*args.items*args.seconds
    kernel_ms = []
    for _ in range(args.warmup + args.reps):
        ev = []
        dec.decode(members, tables=tables, events=ev)
        torch.cuda.synchronize()
        kernel_ms.append(ev[0].elapsed_time(ev[1]))
    kernels = statistics.median(kernel_ms[args.warmup:])
    with_upload = median_time(lambda: dec.decode(members, tables=tables), args.reps, args.warmup, True)
    with_index = median_time(lambda: dec.decode(members), args.reps, args.warmup, True)
    dec.decode(members, tables=tables).check()
    line('gpu_batch', items=args.items, frames=int(sum(len(t[1]) for row in tables for t in row)),
         kernels_ms=kernels, decode_call_ms=1e3*with_upload, decode_call_with_index_ms=1e3*with_index,
         audio_s_per_s=audio/with_upload)
    per_chunk = max(1, int(BreverDataset.PRELOAD_BYTE_BUDGET//(2*size)))
    rows = [[pool[(2*i) % 8], pool[(2*i + 1) % 8]] for i in range(args.members//2)]
    row_tables = [[tables[i % args.items][0], tables[i % args.items][1]] for i in range(len(rows))]

    def preload():
        for a in range(0, len(rows), per_chunk):
            dec.decode(rows[a:a + per_chunk], tables=row_tables[a:a + per_chunk]).check()
    t = median_time(preload, max(3, args.reps//5), 1, True)
    line('gpu_preload', members=2*len(rows), chunks=-(-len(rows)//per_chunk), seconds=t,
         audio_s_per_s=2*len(rows)*args.seconds/t)


if __name__ == '__main__':
    main()
