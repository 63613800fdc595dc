"""Time of `bss_eval` (BSS-eval SDR / SIR / SAR, 512-tap allowed distortion filters; brever_amd/bsseval.py).

    python tools/bsseval_bench.py [--batch 16] [--seconds 4.0] [--fs 16000] [--filter-length 512]
                                  [--shapes 2,1 2,2 4,4] [--repeats 20] [--warmup-s 1.0] [--baseline]

One JSON line per (J, S) = (references, estimates): the whole call, as a host clock around one call that ends in a
device synchronise; after at least `--warmup-s` seconds of warm-up the median of `--repeats` calls is reported (with
the minimum and the 90th percentile). Each line carries what the algorithm needs from the shapes alone: the fp64 FMAs
of the lags (2 L per sample and pair, J S + J^2 pairs), of the J S scalar Levinson solves (2 L^2 each) and of the
block recursion (L^2 (2 J^3 + 2 J^2 S) per item). The block solve alone is read from a kernel trace of this tool
(`rocprofv3 --kernel-trace --stats -- python tools/bsseval_bench.py`): `bss_block_kernel`.

`--baseline` adds, per shape, the wall time of the NumPy / SciPy fp64 reference (tests/bsseval_ref.py, formulation
(b): lags, the assembled J L x J L matrix, a dense solve) for ONE item; run it with the BLAS threads limited to one
(`OMP_NUM_THREADS=1`) for a one-core figure."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from brever_amd.bsseval import bss_eval  # noqa: E402


def algorithmic_work(items, J, S, length, L):
    """fp64 FMAs per call, from the shapes."""
    return dict(lags=2*L*(J*S + J*J)*items*length, scalar_solves=2*L*L*J*S*items,
                block_solve=L*L*(2*J**3 + 2*J*J*S)*items)


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


def signals(items, J, S, length):
    gen = torch.Generator().manual_seed(0)
    s = 0.05*torch.randn(items, J, length, generator=gen)
    x = 0.8*s[:, :S] + 0.3*s[:, :S].roll(3, -1) + 0.3*(s.sum(1, keepdim=True) - s[:, :S]) \
        + 0.03*torch.randn(items, S, length, generator=gen)
    return s, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--seconds', type=float, default=4.0)
    ap.add_argument('--fs', type=int, default=16000)
    ap.add_argument('--filter-length', type=int, default=512)
    ap.add_argument('--shapes', nargs='+', default=['2,1', '2,2', '4,4'], help='references,estimates')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup-s', type=float, default=1.0)
    ap.add_argument('--baseline', action='store_true')
    args = ap.parse_args()
    if args.repeats < 1:
        ap.error('--repeats must be at least 1')
    dev = torch.device('cuda:0')
    length, L = int(round(args.seconds*args.fs)), args.filter_length
    for shape in args.shapes:
        J, S = (int(v) for v in shape.split(','))
        s, x = signals(args.batch, J, S, length)
        sg, xg = s.to(dev), x.to(dev)
        lengths = torch.full((args.batch,), length, device=dev)
        times = timed(lambda: bss_eval(xg, sg, lengths, L), args.repeats, args.warmup_s)
        line = dict(metric='bss_eval_ms', value=1e3*float(np.median(times)), min_ms=1e3*float(times.min()),
                    p90_ms=1e3*float(np.percentile(times, 90)), repeats=args.repeats, warmup_s=args.warmup_s,
                    items=args.batch, references=J, estimates=S, length=length, filter_length=L,
                    timing='host clock around one call ending in a device synchronise, median',
                    algorithmic_work=algorithmic_work(args.batch, J, S, length, L))
        if args.baseline:
            sys.path.insert(0, os.path.join(ROOT, 'tests'))
            import bsseval_ref
            t0 = time.perf_counter()
            bsseval_ref.tables_gram(s[0].double().numpy(), x[0].double().numpy(), L, with_cond=False)
            line['numpy_reference_one_item_s'] = time.perf_counter() - t0
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
