"""Time of the `sdr` criterion (BSS-eval SDR, 512-tap allowed distortion filter; brever_amd/sdr.py).

    python tools/sdr_bench.py [--batch 16] [--seconds 4.0 0.5] [--fs 16000] [--filter-length 512]
                              [--repeats 50] [--warmup-s 1.0]

One JSON line per (length, pass): pass `forward` is the criterion alone, `forward_backward` adds the gradient with
respect to the estimate. A time is a host clock around one call that ends in a device synchronise; after at least
`--warmup-s` seconds of warm-up the median of `--repeats` calls is reported (with the minimum and the 90th
percentile). Each line also carries what the algorithm needs, from the shapes alone: the fp64 FMAs of the
correlations (2 L per sample), of the Levinson recursion (2 L^2 per row) and of the FIR pass (L per sample), and the
bytes each launch must move once, so that a time can be set against the fp64 vector peak and the HBM peak."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from brever_amd import sdr  # noqa: E402
from brever_amd.criterion import init_criterion  # noqa: E402


def algorithmic_work(rows, length, L):
    """fp64 FMAs and bytes read + written once, per launch, from the shapes of `sdr.forward` / `sdr.backward`."""
    chunk = int(sdr.lib().brv_sdr_chunk())
    nchunk = -(-length//chunk)
    partials = 8*rows*nchunk*(2*L + 1)
    return {
        'correlations': dict(fma=2*L*rows*length, bytes=2*4*rows*length + partials),
        'solve': dict(fma=2*L*L*rows, bytes=partials + 8*rows*(L + 3)),
        'fir_backward': dict(fma=L*rows*length, bytes=3*4*rows*length + 8*rows*(L + 3)),
    }


def timed(fn, repeats, warmup_s):
    t_end = time.perf_counter() + warmup_s
    while True:
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            break
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return np.array(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--seconds', type=float, nargs='+', default=[4.0, 0.5])
    ap.add_argument('--fs', type=int, default=16000)
    ap.add_argument('--filter-length', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup-s', type=float, default=1.0)
    args = ap.parse_args()
    if args.repeats < 1:
        ap.error('--repeats must be at least 1')
    dev = torch.device('cuda:0')
    crit = init_criterion('sdr', filter_length=args.filter_length)
    for seconds in args.seconds:
        length = int(round(seconds*args.fs))
        gen = torch.Generator().manual_seed(0)
        y = 0.05*torch.randn(args.batch, 1, length, generator=gen)
        x = (0.8*y + 0.3*y.roll(3, -1) + 0.03*torch.randn(args.batch, 1, length, generator=gen)).to(dev)
        y = y.to(dev)
        x.requires_grad_(True)
        lengths = torch.full((args.batch,), length, device=dev)

        def forward():
            with torch.no_grad():
                crit(x, y, lengths)

        def both():
            x.grad = None
            crit(x, y, lengths).mean().backward()
        for label, fn in (('forward', forward), ('forward_backward', both)):
            times = timed(fn, args.repeats, args.warmup_s)
            line = dict(metric='criterion_ms', criterion='sdr', value=1e3*float(np.median(times)),
                        min_ms=1e3*float(times.min()), p90_ms=1e3*float(np.percentile(times, 90)),
                        repeats=args.repeats, warmup_s=args.warmup_s, shape=[args.batch, 1, length],
                        filter_length=args.filter_length,
                        timing='host clock around one call ending in a device synchronise, median')
            line['pass'] = label
            line['algorithmic_work'] = algorithmic_work(args.batch, length, args.filter_length)
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
