"""Step time of the streaming Conv-TasNet, DCCRN or FFNN (brever_amd.streaming) on one GPU: one JSON line per
(precision, n streams, F hops per call) with the median and p90 of the synchronised step time, the
real-time factor (step time / audio time of a chunk), the streams one GPU keeps in real time at that
chunk size (n / real-time factor, rounded down) and the launches per step.

    python tools/stream_bench.py [--model {convtasnet,dccrn,ffnn}] [--n 1 16 64 256] [--hops 1 16] [--steps 50]
                                 [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--model', choices=['convtasnet', 'dccrn', 'ffnn'], default='convtasnet')
    p.add_argument('--n', type=int, nargs='+', default=[1, 16, 64, 256])
    p.add_argument('--hops', type=int, nargs='+', default=[1, 16])
    p.add_argument('--amp', type=int, nargs='+', default=[0, 1])
    p.add_argument('--steps', type=int, default=50)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--fs', type=int, default=16000)
    args = p.parse_args()

    import torch
    from brever_amd.models import DCCRN, FFNN, ConvTasNet
    from brever_amd.streaming import ConvTasNetStreamer, DCCRNStreamer, FFNNStreamer

    torch.manual_seed(0)
    channels = ()
    if args.model == 'ffnn':
        model = FFNN().cuda()                       # default widths: 384 -> 1024 -> 1024 -> 64, log-mel, 5 stacks

        def Streamer(model, max_streams, use_amp):  # fp32 only
            return FFNNStreamer(model, max_streams=max_streams)
        args.amp = [0]
        launches = 8 + len(FFNNStreamer._linears(model))
        hop = model.stft.hop_length
        channels = (2,)
    elif args.model == 'dccrn':
        model = DCCRN().cuda()                      # default widths: 16 .. 128 channels, 6 levels, LSTM 2 x 128
        Streamer = DCCRNStreamer
        launches = 5 + 2*len(model.mask_net.encoder) + 2*len(model.mask_net.lstm.lstm.layers)
        hop = model.stft.hop_length
    else:
        model = ConvTasNet(causal=True).cuda()      # default widths: 512/32/128/512/128, 8 x 3 blocks
        Streamer = ConvTasNetStreamer
        cfg = model.cfg
        launches = 5 + 3*cfg.layers*cfg.repeats
        hop = cfg.filter_length//2
    for amp in args.amp:
        for n in args.n:
            s = Streamer(model, max_streams=n, use_amp=bool(amp))
            ids = s.open(n)
            for F in args.hops:
                s.reset(ids)
                x = 0.1*torch.randn(n, *channels, F*hop, device='cuda')
                times = []
                for i in range(args.warmup + args.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    s.process(x, ids)
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        times.append(time.perf_counter() - t0)
                times.sort()
                med = times[len(times)//2]
                p90 = times[min(len(times) - 1, int(0.9*len(times)))]
                audio = F*hop/args.fs
                rtf = med/audio
                print(json.dumps(dict(precision='bf16' if amp else 'fp32', n=n, hops=F, chunk_ms=1e3*audio,
                                      step_ms_median=round(1e3*med, 4), step_ms_p90=round(1e3*p90, 4),
                                      rtf=round(rtf, 4), realtime_streams=int(n/rtf),
                                      launches_per_step=launches)), flush=True)
            del s


if __name__ == '__main__':
    main()
