"""FLAC encoding, host against GPU, on seeded speech-like signals (there is no real speech here):

    python tools/flac_enc_bench.py [--seconds 4] [--rows 16] [--chunk 2048] [--mixtures 256] [--reps 20] [--warmup 3]

One JSON line per measurement, each the median of ``--reps`` synchronised runs after ``--warmup``:
  host_encode      brv_flac_encode16 per channel of the same samples, one process, from host arrays, and with the
                   float32 device-to-host copy in front (the GPU-resident case): seconds of audio per second
  gpu_batch        rows x 2 channels x seconds: the kernels alone (events) and the whole encode() call with the
                   download; the same for --chunk rows
  size             compressed bytes per sample, mono 16 bits: brv_flac_encode16, the GPU encoder without and with LPC
  write_dataset    PoolMixtureMaker.write_dataset for --mixtures mixtures of synthetic pools, two sources, with the
                   share of synthesis, encode, wait, copy and tar writing
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brever_amd import flac_enc                                     # noqa: E402
from brever_amd.data import flac_bytes                              # noqa: E402


def signal(seed, n, fs=16000):
    """A speech-like signal: a modulated harmonic tone plus noise, with a pause (tools/flac_bench.py)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)/fs
    f0 = 110 + 40*rng.random()
    x = sum(0.25/k*np.sin(2*np.pi*k*f0*t + rng.random()) for k in range(1, 9))
    x = x*(0.5 + 0.5*np.sin(2*np.pi*(2 + rng.random())*t)) + 0.01*rng.standard_normal(n)
    x[n//3:n//3 + n//16] = 0.001*rng.standard_normal(n//16)
    return (0.5*x).astype(np.float32)


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


def pools(seed=0, fs=16000):
    rng = np.random.default_rng(seed)
    speech = [signal(s, int(fs*(2.0 + 2.0*rng.random()))) for s in range(12)]
    noises = [(0.1*rng.standard_normal(8*fs)).astype(np.float32) for _ in range(4)]
    brirs = [[(0.05*rng.standard_normal((2048, 2))*np.exp(-np.arange(2048)/400.0)[:, None]).astype(np.float32)
              for _ in range(4)] for _ in range(2)]
    for room in brirs:
        for h in room:
            h[10, 0], h[14, 1] = 1.0, 0.8
    return dict(speech=speech, noises=noises, brirs=brirs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=4.0)
    ap.add_argument('--rows', type=int, default=16)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--mixtures', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/flac_enc_bench.py needs a ROCm device: a measurement path has no fallback')
    n = int(args.seconds*16000)
    base = np.stack([np.stack([signal(2*s, n), signal(2*s + 1, n)]) for s in range(8)])       # (8, 2, n)

    def line(metric, **kw):
        print(json.dumps(dict(metric=metric, seconds=args.seconds, **kw)), flush=True)

    enc = flac_enc.FlacBatchEncoder('cuda')
    for rows, reps in ((args.rows, args.reps), (args.chunk, max(3, args.reps//4))):
        host = np.ascontiguousarray(np.tile(base, (-(-rows//8), 1, 1))[:rows])
        x = torch.from_numpy(host).cuda()
        audio = rows*args.seconds                                  # seconds of (stereo) audio
        few = min(rows, 64)                                        # the host's rate does not depend on the batch
        t_host = median_time(lambda: [flac_bytes(ch, 16000) for row in host[:few] for ch in row], min(reps, 5), 1,
                             False)
        t_copy = median_time(lambda: [flac_bytes(ch, 16000) for row in x[:few].cpu().numpy() for ch in row],
                             min(reps, 5), 1, True)
        line('host_encode', rows=few, channels=2, encode_ms=1e3*t_host, with_download_ms=1e3*t_copy,
             audio_s_per_s=few*args.seconds/t_host, audio_s_per_s_with_download=few*args.seconds/t_copy)
        kernel_ms = []
        for _ in range(args.warmup + reps):
            ev = []
            enc.submit(x, events=ev).result()
            torch.cuda.synchronize()
            kernel_ms.append(ev[0].elapsed_time(ev[1]))
        kernels = statistics.median(kernel_ms[args.warmup:])
        call = median_time(lambda: enc.encode(x), reps, args.warmup, True)
        streams = enc.encode(x)
        line('gpu_batch', rows=rows, channels=2, bits=16, block=4096, lpc_order=8, kernels_ms=kernels,
             encode_call_ms=1e3*call, bytes_out=sum(len(s) for s in streams), bytes_float32=int(x.numel()*4),
             audio_s_per_s_kernels=audio/(1e-3*kernels), audio_s_per_s=audio/call)
    mono = torch.from_numpy(np.ascontiguousarray(base[:, 0])).cuda()
    samples = mono.numel()
    line('size', material='synthetic speech-like signals (no real speech on the machine)', samples=samples,
         host_bytes_per_sample=sum(len(flac_bytes(ch, 16000)) for ch in base[:, 0])/samples,
         gpu_fixed_bytes_per_sample=sum(len(s) for s in enc.encode(mono, lpc_order=0))/samples,
         gpu_lpc8_bytes_per_sample=sum(len(s) for s in enc.encode(mono, lpc_order=8))/samples)
    from brever_amd.mixture import PoolMixtureMaker
    maker = PoolMixtureMaker(None, ['mixture', 'foreground'], args.mixtures, noise_count=(1, 3), **pools())
    with tempfile.TemporaryDirectory() as tmp:
        maker.write_dataset(os.path.join(tmp, 'warm'), epoch=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        shares = maker.write_dataset(os.path.join(tmp, 'timed'), epoch=1)
        total = time.perf_counter() - t0
        size = os.path.getsize(os.path.join(tmp, 'timed', 'audio.tar'))
    audio = sum(m['frames'] for m in maker.draw(1))/16000
    line('write_dataset', mixtures=args.mixtures, sources=2, mixture_audio_s=audio, total_s=total, tar_bytes=size,
         audio_s_per_s=audio/total, **{f'{k}_s': v for k, v in shares.items()})


if __name__ == '__main__':
    main()
