"""Time of the STOI / ESTOI training criteria beside `snr` and `multiresyu`.

    python tools/stoi_loss_bench.py [--batch 16] [--length 64000] [--fs 16000] [--repeats 50] [--warmup-s 1.0]

One JSON line per (criterion, pass): pass `forward` is the criterion alone, `forward_backward` adds the gradient
with respect to the estimate. A time is a host clock around one call that ends in a device synchronise; after at
least `--warmup-s` seconds of warm-up the median of `--repeats` calls is reported (with the minimum and the 90th
percentile). The `stoi` / `estoi` lines also give the algorithmic bytes of every launch of the backward (what it
must read and write once, from the shapes), so that a launch time from a kernel trace can be turned into a rate."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from brever_amd import hip, stoi  # noqa: E402
from brever_amd.criterion import init_criterion  # noqa: E402


def algorithmic_bytes(rows, length, fs, ncols):
    """Bytes each new launch reads + writes once (fp32 / int32 elements), from the shapes of `stoi.forward`."""
    n10 = -(-length*stoi.FS//fs)
    nf = max(int(hip.lib().brv_stoi_frames(n10)), 1)
    nseg = max(nf - stoi.SEGMENT + 1, 1)
    comp = stoi.FRAME + nf*stoi.HOP
    tile = stoi.BANDS*stoi.SEGMENT
    out = {
        # both band tensors in (every tile re-reads 30 frames of 15 bands), one tile out per segment
        'brv_sl_segment_backward': 4*rows*nseg*(2*tile + tile),
        # every (band, frame) gathers <= 30 tile entries; the estimate's bands in, band gradient out; then the
        # spectrum in and its gradient out
        'brv_sl_bands_backward': 4*rows*(nseg*tile + 2*stoi.BANDS*nf + 2*nf*ncols + stoi.BANDS*nf),
        'brv_gemm_f32 (frame gradient)': 4*(rows*nf*ncols + stoi.FRAME*ncols + rows*nf*stoi.FRAME),
        'brv_sl_fold_frames': 4*rows*(nf*stoi.FRAME + comp),
        'brv_sl_compact_backward': 4*rows*(comp + nf + n10),
    }
    if fs != stoi.FS:
        out['brv_sl_resample_backward'] = 4*rows*(n10 + length)
    return out


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
    ap.add_argument('--length', type=int, default=64000)
    ap.add_argument('--fs', type=int, default=16000)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup-s', type=float, default=1.0)
    ap.add_argument('--criteria', nargs='+', default=['snr', 'multiresyu', 'stoi', 'estoi'])
    args = ap.parse_args()
    if args.repeats < 1:
        ap.error('--repeats must be at least 1')
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    t = torch.arange(args.length)/args.fs
    env = (torch.sin(2*np.pi*3*t) > -0.3)*(0.5 + 0.5*torch.sin(2*np.pi*1.3*t))          # gaps: frames do get dropped
    y = (0.05*torch.randn(args.batch, 1, args.length, generator=gen)*env).to(dev)
    x = (y.cpu() + 0.03*torch.randn(args.batch, 1, args.length, generator=gen)).to(dev).requires_grad_(True)
    lengths = torch.full((args.batch,), args.length, device=dev)
    for name in args.criteria:
        kwargs = dict(fs=args.fs) if name in ('stoi', 'estoi') else {}
        crit = init_criterion(name, **kwargs)

        def forward():
            with torch.no_grad():
                crit(x, y, lengths)

        def both():
            x.grad = None
            crit(x, y, lengths).mean().backward()
        for label, fn in (('forward', forward), ('forward_backward', both)):
            times = timed(fn, args.repeats, args.warmup_s)
            line = dict(metric='criterion_ms', criterion=name, value=1e3*float(np.median(times)),
                        min_ms=1e3*float(times.min()), p90_ms=1e3*float(np.percentile(times, 90)),
                        repeats=args.repeats, warmup_s=args.warmup_s, shape=[args.batch, 1, args.length],
                        fs=args.fs, timing='host clock around one call ending in a device synchronise, median')
            line['pass'] = label
            if name in ('stoi', 'estoi') and label == 'forward_backward':
                line['backward_algorithmic_bytes'] = algorithmic_bytes(args.batch, args.length, args.fs,
                                                                       stoi.constants(dev, args.fs)['basis'].shape[1])
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
