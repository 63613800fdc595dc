"""Throughput of the batched mixture engine: one JSON line of mixtures/s.

    python tools/mix_bench.py [--batch 64] [--seconds 4] [--brir-seconds 1] [--noises 3] [--steps 10] [--warmup 2]
                              [--diffuse-color COLOUR] [--ltas-eq] [--decay] [--decay-color COLOUR] [--cold-cache]

The recipe: ``batch`` mixtures of a ``seconds`` long target, ``noises`` directional noises of the same length,
BRIRs of ``brir-seconds``, SNR and RMS jitter set, (mixture, foreground) written. Timed from the first launch
of a batch to the end of its last kernel, descriptors included; the pools are on the device beforehand, as
``PoolMixtureMaker`` keeps them.

``--diffuse-color`` / ``--ltas-eq`` add a diffuse noise over the 8 BRIRs of the room, coloured / matched to the speech
LTAS; ``--decay`` adds a BRIR decay (the reference's default ranges) to the target's and every noise's BRIR.
``--cold-cache`` empties the colouring-filter cache before every batch (every filter is then computed on the host
again); the line then also holds the host time of those misses.

``--cpu-reference DIR`` instead times ``Mixture`` of a checkout of the reference (philgzl/brever) at DIR on the
same recipe, one mixture at a time on this host's CPU (``sofa`` and ``soundfile``, which it imports but does
not use here, may be absent: they are stubbed)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def recipe(args, rng):
    fs = 16000
    n, taps = int(args.seconds*fs), int(args.brir_seconds*fs)
    decay = np.exp(-np.arange(taps)[:, None]/(0.2*taps))
    brirs = [(0.05*rng.standard_normal((taps, 2))*decay).astype(np.float32) for _ in range(8)]
    for h in brirs:
        h[20, 0], h[26, 1] = 1.0, 0.8
    speech = [(0.1*rng.standard_normal(n)).astype(np.float32) for _ in range(16)]
    noises = [(0.1*rng.standard_normal(4*n)).astype(np.float32) for _ in range(8)]
    return speech, noises, brirs


def gpu(args):
    import torch
    from brever_amd import mixture
    rng = np.random.default_rng(0)
    speech, noises, brirs = recipe(args, rng)
    maker = mixture.PoolMixtureMaker(None, ['mixture', 'foreground'], args.batch, speech=speech, noises=noises,
                                     brirs=[brirs], noise_count=(args.noises, args.noises), rms_jitter=(-3.0, 3.0),
                                     batch=args.batch, block=args.block,
                                     diffuse=args.diffuse_color is not None or args.ltas_eq,
                                     diffuse_color=args.diffuse_color or 'white', diffuse_ltas_eq=args.ltas_eq,
                                     decay=args.decay, decay_color=args.decay_color)
    times, miss_ms = [], []
    for step in range(args.warmup + args.steps):
        meta = maker.draw(step)
        if args.cold_cache:
            mixture.color_filters.clear()
        missed = mixture.color_filters.misses, mixture.color_filters.miss_seconds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = maker.synthesize(meta)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        miss_ms.append((mixture.color_filters.misses - missed[0], 1e3*(mixture.color_filters.miss_seconds - missed[1])))
    res.check()
    t = float(np.median(times[args.warmup:]))
    extra = dict(diffuse_color=args.diffuse_color, ltas_eq=args.ltas_eq, decay=args.decay,
                 decay_color=args.decay_color, cold_cache=args.cold_cache, ms_min=1e3*min(times[args.warmup:]),
                 ms_max=1e3*max(times[args.warmup:]), filter_misses=mixture.color_filters.misses)
    # what the cache misses of a batch cost on the host (the cache's own clock), median over the timed batches
    extra.update(filter_misses_per_batch=float(np.median([k for k, _ in miss_ms[args.warmup:]])),
                 host_ms_filter_misses_per_batch=float(np.median([ms for _, ms in miss_ms[args.warmup:]])),
                 peak_gib=torch.cuda.max_memory_allocated()/2**30)
    print(json.dumps(dict(metric='mixtures_per_s', value=args.batch/t, ms_per_batch=1e3*t, batch=args.batch,
                          seconds=args.seconds, brir_seconds=args.brir_seconds, noises=args.noises,
                          block=args.block, steps=args.steps, device=torch.cuda.get_device_name(0), **extra)))


def cpu_reference(args):
    for name in ('sofa', 'soundfile'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, args.cpu_reference)
    from brever.mixture.mixture import Mixture
    rng = np.random.default_rng(0)
    speech, noises, brirs = recipe(args, rng)
    f64 = lambda a: np.asarray(a, dtype=np.float64)                      # noqa: E731
    times = []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        mix = Mixture()
        mix.add_speech(f64(speech[step % len(speech)]), f64(brirs[step % len(brirs)]), 50e-3, 0.0, 16000)
        mix.add_noises([f64(noises[j][:len(mix)]) for j in range(args.noises)],
                       [f64(brirs[(step + j + 1) % len(brirs)]) for j in range(args.noises)])
        mix.set_snr(0.0)
        mix.set_rms(mix.get_rms() + 1.0)
        out = mix.mixture.astype(np.float32), mix.foreground.astype(np.float32)      # noqa: F841
        times.append(time.perf_counter() - t0)
    t = float(np.median(times[args.warmup:]))
    print(json.dumps(dict(metric='mixtures_per_s', value=1/t, ms_per_mixture=1e3*t, seconds=args.seconds,
                          brir_seconds=args.brir_seconds, noises=args.noises, device='cpu reference, one process')))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=4.0)
    ap.add_argument('--brir-seconds', type=float, default=1.0)
    ap.add_argument('--noises', type=int, default=3)
    ap.add_argument('--block', type=int, default=256)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--diffuse-color', default=None, choices=['brown', 'pink', 'white', 'blue', 'violet'])
    ap.add_argument('--ltas-eq', action='store_true')
    ap.add_argument('--decay', action='store_true')
    ap.add_argument('--decay-color', default='white', choices=['brown', 'pink', 'white', 'blue', 'violet'])
    ap.add_argument('--cold-cache', action='store_true')
    ap.add_argument('--cpu-reference', default=None)
    a = ap.parse_args()
    cpu_reference(a) if a.cpu_reference else gpu(a)
