"""Time of the shoebox image-source simulator (brever_amd/rir.py).

    python tools/rir_bench.py [--shapes 100x19x8000 2x3x800] [--fs 16000] [--seed 0] [--repeats 3]
                              [--bands K] [--ear_model pattern|sphere] [--scratch_bytes N] [--hrir D T_H]

One JSON line per shape ROOMSxANGLESxTAPS: `random_rooms(ROOMS, seed, angles=ANGLES equally spaced, taps=TAPS)`,
two ears per angle. `value` is the median over `--repeats` launches of brv_rir_simulate alone (a host clock around a
launch that ends in a device synchronise, after one warm-up launch); `tables_ms` is the host's table building,
`end_to_end_ms` one whole `simulate_brirs` call (tables, upload, launch, download).

What the model asks for is counted from the tables, not timed: `images` are the images that touch at least one tap,
`window_evaluations` the (image, tap) pairs with |t - tau| < W/2. Both are exact for the first job of every room and
multiplied by the room's jobs (the ears of a room differ by centimetres). A window evaluation needs 7 fp64 vector
operations (a subtraction, two FMAs, two products, a reciprocal, an addition); `share_of_fp64_issue_peak` sets
that against 39.3 T fp64 vector instructions per second (the 78.6 TFLOP/s of the datasheet), and is therefore a
floor's share, not a utilisation: the kernel's reciprocal alone is five instructions, and selects, compares and LDS
reads come on top. `tile_images` gives the median and the largest number of images per tile of the first job,
which is what makes the last tiles of a long response the expensive ones.

With `--bands K` a second line per shape measures the band entry points on the same rooms with
`bands=K` and `--ear_model`, in the same run: `tile_ms` is brv_rir_bands_channels alone and `combine_ms`
brv_rir_bands_combine alone (each the median over `--repeats` launches after a warm-up, summed over the chunks of
jobs whose channel rows fit `--scratch_bytes`), `end_to_end_ms` one whole `simulate_brirs` call.
`tile_over_single_band` is `tile_ms` over the `value` of the first line, to be set against `channels`: the point of
the multi-channel kernel is that C channels cost less than C launches. `combine_share_of_fp64_fma_peak` sets the
`jobs * taps * C * M_f` fused multiply-adds of the filters against 39.3 T per second.

With `--hrir D T_H` two more lines per shape measure the measured-ear entry points on the same rooms
with one coefficient per wall (K = 1) and with `bands=K`, in the same run, for a synthetic set of `D` directions (a
Fibonacci sphere) and `T_H` taps: `channels_ms` is brv_rir_hrir_channels alone (its clearing of the direction scratch
included), `fold_ms` brv_rir_hrir_fold alone and `combine_ms` brv_rir_bands_combine alone, each the median over
`--repeats` launches after a warm-up, summed over the chunks. One job is one (room, angle) and gives both ears.
`fold_fmas` counts `jobs * K * (taps + pad) * D * 2 * n_filter`, what the fold would do if it passed over nothing;
`*_over_bands_*` set a launch against the band line of the same run (`--bands` is required)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from brever_amd import rir  # noqa: E402

FP64_INSTRUCTIONS_PER_SECOND = 39.3e12
INSTRUCTIONS_PER_EVALUATION = 7


def job_inputs(rooms):
    """``geom``, ``shape`` as ``simulate_brirs`` lays them out, and the first job of every room with its job count."""
    geom, shape, first, at = [], [], [], 0
    for room in rooms:
        first.append((len(geom), 2*len(room.angles)))
        ears, side = room.ears(), room.side()
        for angle in room.angles:
            for e in range(2):
                geom.append(rir._geom_row(room.dims, room.beta, room.source(angle), ears[e],
                                          side if e == 0 else -side, room.ear_pattern))
                shape.append((room.taps, at + e, 2))
            at += 2*room.taps
    return np.array(geom), np.array(shape), first


def count_job(rows, ix, opts, tiles=False):
    """``(images, window evaluations, images per tile or None)`` of one job from its tables."""
    fs, c, W = opts
    hdr, nx, ny, nz, taps = (int(v) for v in ix[:5])
    x2, y2, z2 = (rows[a:b, 3] for a, b in ((hdr + 1, hdr + 1 + nx), (hdr + 1 + nx, hdr + 1 + nx + ny),
                                            (hdr + 1 + nx + ny, hdr + 1 + nx + ny + nz)))
    tau = np.sqrt((x2[:, None, None] + y2[None, :, None]) + z2[None, None, :]).ravel()*fs/c
    first = np.maximum(np.floor(tau - W/2) + 1, 0)
    last = np.minimum(np.ceil(tau + W/2) - 1, taps - 1)
    n = np.maximum(last - first + 1, 0)
    hit = n > 0
    per_tile = None
    if tiles:                                           # an image counts in every tile it touches
        first, last = first[hit], last[hit]
        per_tile = np.array([np.count_nonzero((first <= t + rir.TILE - 1) & (last >= t))
                             for t in range(0, taps, rir.TILE)])
    return int(hit.sum()), int(n.sum()), per_tile


def timed(fn, repeats):
    """Median and least seconds of ``repeats`` calls of ``fn`` after one warm-up call, each ending in a synchronise."""
    times = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times[1:])), float(min(times[1:]))


def bench_bands(args, rooms, dev, single_band_seconds):
    """The JSON line of the band entry points for ``rooms`` (all of one group)."""
    room = rooms[0]
    sphere = room.ear_model == 'sphere'
    geom, shape, at = [], [], 0
    for r in rooms:
        ears, side = r.ears(), r.side()
        for angle in r.angles:
            for e in range(2):
                geom.append(rir._band_geom_row(r.dims, r.beta, r.source(angle), r.head if sphere else ears[e],
                                               side if e == 0 else -side, r.ear_pattern))
                shape.append((r.taps, at + e, 2))
            at += 2*r.taps
    geom, shape = np.array(geom), np.array(shape)
    filters, pad = rir.band_filters(args.fs, args.bands, room.ear_model, room.head_radius)
    opts = rir.band_opts(args.fs, args.bands, room.ear_model, room.head_radius, pad=pad)
    channels = rir.channels_of(opts)
    filters_d = torch.tensor(filters, device=dev)
    out = torch.zeros(at, dtype=torch.float32, device=dev)
    chunks = rir.chunk_jobs(shape[:, 0], channels, pad, args.scratch_bytes)
    tile = combine = tile_min = combine_min = tables_s = 0.0
    table_rows = 0
    for first, end in chunks:
        t0 = time.perf_counter()
        rows, index = rir.build_band_tables(geom[first:end], shape[first:end], opts)
        tables_s += time.perf_counter() - t0
        table_rows += len(rows)
        tables, index_d = torch.from_numpy(rows).to(dev), torch.from_numpy(index).to(dev)
        scratch = torch.empty(int(index[-1, 7]) + channels*(int(index[-1, 4]) + pad), dtype=torch.float64, device=dev)
        max_taps = int(index[:, 4].max())
        median, least = timed(lambda: rir.bands_call(
            'brv_rir_bands_channels', tables, index_d, len(index), len(tables), max_taps, opts.ctypes.data, -1,
            scratch, scratch.numel(), rir.hip.stream()), args.repeats)
        tile, tile_min = tile + median, tile_min + least
        median, least = timed(lambda: rir.bands_call(
            'brv_rir_bands_combine', scratch, scratch.numel(), index_d, len(index), max_taps, opts.ctypes.data,
            filters_d, filters.shape[1], out, out.numel(), rir.hip.stream()), args.repeats)
        combine, combine_min = combine + median, combine_min + least
        del tables, index_d, scratch
    t0 = time.perf_counter()
    brirs = rir.simulate_brirs(rooms, fs=args.fs, device=dev, scratch_bytes=args.scratch_bytes)
    end_to_end_ms = 1e3*(time.perf_counter() - t0)
    assert np.array_equal(brirs[0][0].reshape(-1), out[:2*room.taps].cpu().numpy())
    fmas = float(shape[:, 0].sum())*channels*filters.shape[1]
    return dict(metric='rir_bands_ms', value=1e3*(tile + combine), tile_ms=1e3*tile, tile_min_ms=1e3*tile_min,
                combine_ms=1e3*combine, combine_min_ms=1e3*combine_min, end_to_end_ms=end_to_end_ms,
                tables_ms=1e3*tables_s, table_rows=table_rows, repeats=args.repeats, rooms=len(rooms),
                angles=len(room.angles), taps=room.taps, jobs=len(geom), fs=args.fs, window=float(opts[2]),
                bands=args.bands, ear_model=room.ear_model, channels=channels, filter_taps=filters.shape[1],
                pad=pad, chunks=len(chunks), scratch_bytes=args.scratch_bytes,
                single_band_ms=1e3*single_band_seconds, tile_over_single_band=tile/single_band_seconds,
                combine_fmas=fmas, combine_share_of_fp64_fma_peak=fmas/combine/FP64_INSTRUCTIONS_PER_SECOND,
                timing='host clock around one launch ending in a device synchronise, median, summed over chunks')


def synthetic_set(D, taps_h, fs, seed):
    """``D`` directions on a Fibonacci sphere turned by a seeded angle, seeded normal responses under a decaying
    envelope: the cost of the kernels depends on ``D`` and ``taps_h`` only."""
    rng = np.random.default_rng([seed, D, taps_h])
    i = np.arange(D) + 0.5
    z = 1.0 - 2.0*i/D
    phi = i*np.pi*(3.0 - np.sqrt(5.0)) + rng.uniform(0.0, 2.0*np.pi)
    rho = np.sqrt(1.0 - z*z)
    hrirs = rng.standard_normal((D, 2, taps_h))*np.exp(-np.arange(taps_h)/(taps_h/4.0))
    return rir.HrirSet(np.stack([rho*np.cos(phi), rho*np.sin(phi), z], axis=1), hrirs, fs)


def bench_hrir(args, rooms, dev, bands_line):
    """The JSON line of the measured-ear entry points for ``rooms`` (all of one group)."""
    room = rooms[0]
    hrirs, K = room.hrirs, max(room.bands(), 1)
    geom, shape, at = [], [], 0
    for r in rooms:
        for angle in r.angles:
            geom.append(rir._hrir_geom_row(r.dims, r.beta, r.source(angle), r.head, r.front(), r.side()))
            shape.append((r.taps, at, 2, 1))
            at += 2*r.taps
    geom, shape = np.array(geom), np.array(shape)
    filters, pad = rir.band_filters(args.fs, K)
    opts = rir.hrir_opts(args.fs, K, hrirs, pad=pad)
    combine_opts = rir.band_opts(args.fs, K, 'pattern', 0.0, pad=pad)
    D = len(hrirs)
    filters_d = torch.tensor(filters, device=dev)
    directions_d = torch.tensor(hrirs.directions, device=dev)
    responses_d = torch.from_numpy(rir.padded_hrirs(hrirs)).to(dev)
    out = torch.zeros(at, dtype=torch.float32, device=dev)
    chunks = rir.chunk_jobs(shape[:, 0], K*(D + 2), pad, args.scratch_bytes)
    sums = dict(channels=[0.0, 0.0], fold=[0.0, 0.0], combine=[0.0, 0.0])
    tables_s, table_rows = 0.0, 0
    for first, end in chunks:
        t0 = time.perf_counter()
        rows, index, ear_index = rir.build_hrir_tables(geom[first:end], shape[first:end], opts, hrirs.directions)
        tables_s += time.perf_counter() - t0
        table_rows += len(rows)
        tables, index_d, ear_d = (torch.from_numpy(v).to(dev) for v in (rows, index, ear_index))
        last = int(index[-1, 4]) + pad
        dirs = torch.empty(int(index[-1, 5]) + K*D*last, dtype=torch.float64, device=dev)
        fold = torch.empty(int(index[-1, 7]) + 2*K*last, dtype=torch.float64, device=dev)
        max_taps = int(index[:, 4].max())
        launches = dict(
            channels=lambda: rir.hrir_call(
                'brv_rir_hrir_channels', tables, index_d, len(index), len(tables), max_taps, opts.ctypes.data, -1,
                directions_d, dirs, dirs.numel(), rir.hip.stream()),
            fold=lambda: rir.hrir_call(
                'brv_rir_hrir_fold', dirs, dirs.numel(), index_d, len(index), max_taps, opts.ctypes.data, responses_d,
                responses_d.shape[2], fold, fold.numel(), rir.hip.stream()),
            combine=lambda: rir.bands_call(
                'brv_rir_bands_combine', fold, fold.numel(), ear_d, len(ear_d), max_taps, combine_opts.ctypes.data,
                filters_d, filters.shape[1], out, out.numel(), rir.hip.stream()))
        for name, fn in launches.items():
            median, least = timed(fn, args.repeats)
            sums[name][0] += median
            sums[name][1] += least
        del tables, index_d, ear_d, dirs, fold
    t0 = time.perf_counter()
    brirs = rir.simulate_brirs(rooms, fs=args.fs, device=dev, scratch_bytes=args.scratch_bytes)
    end_to_end_ms = 1e3*(time.perf_counter() - t0)
    assert np.array_equal(brirs[0][0].reshape(-1), out[:2*room.taps].cpu().numpy())
    rows_taps = float((shape[:, 0] + pad).sum())
    fold_fmas = rows_taps*K*D*2*responses_d.shape[2]
    combine_fmas = 2.0*float(shape[:, 0].sum())*K*filters.shape[1]
    line = dict(metric='rir_hrir_ms', value=1e3*sum(v[0] for v in sums.values()),
                channels_ms=1e3*sums['channels'][0], channels_min_ms=1e3*sums['channels'][1],
                fold_ms=1e3*sums['fold'][0], fold_min_ms=1e3*sums['fold'][1],
                combine_ms=1e3*sums['combine'][0], combine_min_ms=1e3*sums['combine'][1],
                dominant=max(sums, key=lambda k: sums[k][0]), end_to_end_ms=end_to_end_ms, tables_ms=1e3*tables_s,
                table_rows=table_rows, repeats=args.repeats, rooms=len(rooms), angles=len(room.angles),
                taps=room.taps, jobs=len(geom), fs=args.fs, window=float(opts[2]), bands=K, directions=D,
                hrir_taps=hrirs.taps, hrir_filter_taps=int(responses_d.shape[2]), filter_taps=filters.shape[1],
                pad=pad, chunks=len(chunks), scratch_bytes=args.scratch_bytes,
                direction_scratch_bytes_per_job=8*K*D*(room.taps + pad), fold_fmas=fold_fmas,
                fold_share_of_fp64_fma_peak=fold_fmas/sums['fold'][0]/FP64_INSTRUCTIONS_PER_SECOND,
                combine_fmas=combine_fmas,
                timing='host clock around one launch ending in a device synchronise, median, summed over chunks')
    if bands_line is not None:
        line.update(bands_tile_ms=bands_line['tile_ms'], bands_combine_ms=bands_line['combine_ms'],
                    bands_pair_ms=bands_line['value'],
                    channels_over_bands_tile=line['channels_ms']/bands_line['tile_ms'],
                    fold_over_bands_pair=line['fold_ms']/bands_line['value'],
                    combine_over_bands_combine=line['combine_ms']/bands_line['combine_ms'],
                    value_over_bands_pair=line['value']/bands_line['value'])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['100x19x8000', '2x3x800'])
    ap.add_argument('--fs', type=int, default=16000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--bands', type=int, default=0, help='also measure the band entry points with this many bands')
    ap.add_argument('--ear_model', choices=['pattern', 'sphere'], default='pattern')
    ap.add_argument('--scratch_bytes', type=int, default=1 << 30)
    ap.add_argument('--hrir', type=int, nargs=2, default=None, metavar=('D', 'T_H'),
                    help='also measure the measured-ear entry points with a synthetic set of D directions and T_H taps')
    args = ap.parse_args()
    if args.hrir and not args.bands:
        ap.error('--hrir is measured against the band entry points of the same run: give --bands K as well')
    if not torch.cuda.is_available():
        raise SystemExit('rir_bench needs a ROCm device: a time from anywhere else says nothing')
    dev = torch.device('cuda:0')
    for spec in args.shapes:
        n_rooms, n_angles, taps = (int(v) for v in spec.split('x'))
        angles = np.linspace(-90.0, 90.0, n_angles).tolist() if n_angles > 1 else [0.0]
        rooms = rir.random_rooms(n_rooms, args.seed, angles=angles, taps=taps, fs=args.fs)
        geom, shape, first = job_inputs(rooms)
        t0 = time.perf_counter()
        rows, index, opts = rir.build_tables(geom, shape, args.fs)
        tables_ms = 1e3*(time.perf_counter() - t0)
        images = evaluations = 0
        for j, jobs in first:
            i, e, per_tile = count_job(rows, index[j], opts, tiles=j == 0)
            images, evaluations = images + i*jobs, evaluations + e*jobs
            if j == 0:
                tile_images = dict(median=float(np.median(per_tile)), largest=float(per_tile.max()),
                                   tiles=len(per_tile))
        tables, index_d = torch.from_numpy(rows).to(dev), torch.from_numpy(index).to(dev)
        out = torch.zeros(2*taps*n_rooms*n_angles, dtype=torch.float32, device=dev)
        times = []
        for k in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rir.launch(tables, index_d, opts, -1, taps, out)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        seconds = float(np.median(times[1:]))
        t0 = time.perf_counter()
        brirs = rir.simulate_brirs(rooms, fs=args.fs, device=dev)
        end_to_end_ms = 1e3*(time.perf_counter() - t0)
        assert np.array_equal(brirs[0][0].reshape(-1), out[:2*taps].cpu().numpy())
        line = dict(metric='rir_simulate_ms', value=1e3*seconds, min_ms=1e3*float(min(times[1:])),
                    first_launch_ms=1e3*times[0], repeats=args.repeats, rooms=n_rooms, angles=n_angles, taps=taps,
                    jobs=len(geom), fs=args.fs, window=float(opts[2]), table_rows=len(rows), tables_ms=tables_ms,
                    end_to_end_ms=end_to_end_ms, images=images, window_evaluations=evaluations,
                    images_per_s=images/seconds, window_evaluations_per_s=evaluations/seconds,
                    share_of_fp64_issue_peak=evaluations*INSTRUCTIONS_PER_EVALUATION/seconds /
                    FP64_INSTRUCTIONS_PER_SECOND, tile_images=tile_images,
                    timing='host clock around one launch ending in a device synchronise, median',
                    counts='exact for the first job of every room, times the jobs of the room')
        print(json.dumps(line), flush=True)
        if args.bands:
            del tables, index_d, out
            banded = rir.random_rooms(n_rooms, args.seed, angles=angles, taps=taps, fs=args.fs, bands=args.bands,
                                      ear_model=args.ear_model)
            bands_line = bench_bands(args, banded, dev, seconds)
            print(json.dumps(bands_line), flush=True)
            if args.hrir:
                del banded
                hrirs = synthetic_set(args.hrir[0], args.hrir[1], args.fs, args.seed)
                for bands in (0, args.bands):
                    measured = rir.random_rooms(n_rooms, args.seed, angles=angles, taps=taps, fs=args.fs, bands=bands,
                                                ear_model='hrir', hrirs=hrirs)
                    print(json.dumps(bench_hrir(args, measured, dev, bands_line)), flush=True)


if __name__ == '__main__':
    main()
