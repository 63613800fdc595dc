"""Freeze mixtures synthesised on the GPU as a dataset on disk: ``DIR/audio.tar`` (members
``audio/NNNNN_<source>.flac``) and ``DIR/mixture_info.json``, the layout ``BreverDataset`` and the entry points
(``init_model.py --train_path DIR --val_path DIR``) read.

A thin command line over ``brever_amd.mixture.PoolMixtureMaker.write_dataset``: the mixtures of ``--epoch`` are
drawn from ``--seed``, synthesised batch by batch from the in-memory pools of ``--pool`` (a ``.npz`` with
``speech_<i>``, ``noise_<i>``, ``brir_<room>_<angle>`` arrays) and encoded as stereo FLAC on the device; the same
``(seed, epoch)`` gives byte-identical archives. With ``--simulate_rooms N`` the BRIRs are not read from the pool
but simulated on the device for ``N`` random shoebox rooms (``brever_amd.rir``; ``--room_*``). Like the reference's ``scripts/create_dataset.py`` it refuses a
directory that already holds a ``mixture_info.json`` unless ``-f`` is given, and ``--no_tar`` writes the directory
``DIR/audio/`` instead of the archive.

Differences, on purpose: the reference's script takes a dataset directory whose ``config.yaml`` holds an ``rmm``
section (corpora, rooms, angle ranges, file limits) for ``RandomMixtureMaker``. This script does not read that
configuration: there is no corpus scanning in this build. The pools are given as arrays and
the maker's options by their own names, below."""
import argparse
import os
import time

# read when the HIP runtime loads (torch import): see brever_amd/__init__.py
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

from _common import ROOT  # noqa: E402,F401

COMPONENTS = ('mixture', 'foreground', 'background', 'speech', 'noise', 'early_speech', 'late_speech', 'dir_noise',
              'diffuse')


def parse(argv=None):
    p = argparse.ArgumentParser(description='write a fixed dataset of GPU-synthesised mixtures')
    p.add_argument('--pool', required=True, help='.npz with speech_<i>, noise_<i>, brir_<room>_<angle> arrays')
    p.add_argument('--output', required=True, help='dataset directory to write')
    p.add_argument('--size', type=int, required=True, help='number of mixtures')
    p.add_argument('--sources', nargs='+', default=['mixture', 'foreground'], choices=COMPONENTS)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--epoch', type=int, default=0, help='which epoch of the seed to freeze')
    p.add_argument('--bits', type=int, default=16, choices=(16, 24), help='bits per sample of the FLAC members')
    p.add_argument('--no_tar', action='store_true', help='write the directory audio/ instead of audio.tar')
    p.add_argument('-f', '--force', action='store_true', help='overwrite if already exists')
    p.add_argument('--block_size', type=int, default=4096, help='FLAC block size')
    p.add_argument('--lpc_order', type=int, default=8, help='0 switches the LPC candidates off')
    # the maker's options, by its own names
    p.add_argument('--fs', type=int, default=16000)
    p.add_argument('--padding', type=float, default=0.0)
    p.add_argument('--noise_count', type=int, nargs=2, default=[0, 3])
    p.add_argument('--snr', type=float, nargs=2, default=[-5.0, 10.0])
    p.add_argument('--ndr', type=float, nargs=2, default=[0.0, 30.0])
    p.add_argument('--diffuse', action='store_true')
    p.add_argument('--rms_jitter', type=float, nargs=2, default=[0.0, 0.0])
    p.add_argument('--batch', type=int, default=64, help='mixtures per synthesis batch')
    p.add_argument('--block', type=int, default=256, help='partition size of the convolution')
    p.add_argument('--device', default='cuda')
    p.add_argument('--diffuse_color', default='white')
    p.add_argument('--diffuse_ltas_eq', action='store_true')
    p.add_argument('--decay', action='store_true')
    p.add_argument('--decay_color', default='white')
    p.add_argument('--decay_rt60', type=float, nargs=2, default=[0.1, 5.0])
    p.add_argument('--decay_drr', type=float, nargs=2, default=[5.0, 35.0])
    p.add_argument('--decay_delay', type=float, nargs=2, default=[0.075, 0.100])
    p.add_argument('--synthetic_noises', nargs='*', default=[])
    # BRIRs simulated on the device instead of read from the pool (brever_amd.rir: random_rooms, simulate_brirs)
    p.add_argument('--simulate_rooms', type=int, default=0, metavar='N',
                   help='simulate N shoebox rooms for the BRIRs; --pool then needs speech_<i> / noise_<i> only')
    p.add_argument('--room_seed', type=int, default=0)
    p.add_argument('--room_rt60', type=float, nargs=2, default=[0.2, 0.8], metavar=('LO', 'HI'))
    p.add_argument('--room_distance', type=float, nargs=2, default=[0.5, 3.0], metavar=('LO', 'HI'))
    p.add_argument('--room_angles', type=float, nargs='+', default=list(range(-90, 91, 10)), metavar='A')
    p.add_argument('--room_taps', type=int, default=None, help='taps of every BRIR; default ceil(rt60 fs) per room')
    p.add_argument('--room_bands', type=int, default=0, metavar='K',
                   help='octave bands of the wall coefficients from 125 Hz upwards; 0: one coefficient per wall')
    p.add_argument('--room_band_tilt', type=float, nargs=2, default=[0.0, 0.25], metavar=('LO', 'HI'),
                   help='with --room_bands: rt60 falls by 2^-u per octave, u uniform in this range per room')
    p.add_argument('--room_ear_model', choices=['pattern', 'sphere', 'hrir'], default='pattern',
                   help='an ear is a first-order receiver, a point on a rigid sphere (head shadow, Woodworth delay), '
                        'or the measured pair of --room_hrirs')
    p.add_argument('--room_hrirs', default=None, metavar='FILE',
                   help='with --room_ear_model hrir: the measured HRIR set, a SimpleFreeFieldHRIR .sofa file or the '
                        '.npz of brever_amd.rir.HrirSet.save')
    args = p.parse_args(argv)
    if (args.room_ear_model == 'hrir') != (args.room_hrirs is not None):
        p.error('--room_ear_model hrir and --room_hrirs FILE go together')
    return args


def simulated_pools(args):
    """``speech``, ``noises`` of ``--pool`` and the BRIRs of ``--simulate_rooms`` rooms, as the maker's keywords."""
    from brever_amd import rir
    from brever_amd.mixture import PoolMixtureMaker
    if args.simulate_rooms < 1:
        raise SystemExit('--simulate_rooms must be at least 1')
    speech, noises, _ = PoolMixtureMaker._load(args.pool)
    rooms = rir.random_rooms(args.simulate_rooms, args.room_seed, rt60=args.room_rt60, distance=args.room_distance,
                             angles=args.room_angles, taps=args.room_taps, fs=args.fs, bands=args.room_bands,
                             band_tilt=args.room_band_tilt, ear_model=args.room_ear_model,
                             hrirs=rir.load_hrirs(args.room_hrirs) if args.room_hrirs else None)
    return dict(speech=speech, noises=noises, brirs=rir.simulate_brirs(rooms, fs=args.fs, device=args.device))


def main(argv=None):
    args = parse(argv)
    info = os.path.join(args.output, 'mixture_info.json')
    if os.path.exists(info) and not args.force:
        raise SystemExit(f'{info} already exists: a dataset was written here; pass -f to overwrite it')
    if args.size < 1:
        raise SystemExit('--size must be at least 1')
    from brever_amd.mixture import PoolMixtureMaker
    pools = simulated_pools(args) if args.simulate_rooms else {}
    maker = PoolMixtureMaker(
        args.pool, args.sources, args.size, seed=args.seed, fs=args.fs, padding=args.padding,
        noise_count=args.noise_count, snr=args.snr, ndr=args.ndr, diffuse=args.diffuse, rms_jitter=args.rms_jitter,
        batch=args.batch, block=args.block, device=args.device, diffuse_color=args.diffuse_color,
        diffuse_ltas_eq=args.diffuse_ltas_eq, decay=args.decay, decay_color=args.decay_color,
        decay_rt60=args.decay_rt60, decay_drr=args.decay_drr, decay_delay=args.decay_delay,
        synthetic_noises=args.synthetic_noises, **pools)
    if args.force:                                 # what the other form of an earlier run left
        import shutil
        stale = os.path.join(args.output, 'audio' if not args.no_tar else 'audio.tar')
        if os.path.isdir(stale):
            shutil.rmtree(stale)
        elif os.path.exists(stale):
            os.remove(stale)
    t0 = time.perf_counter()
    seconds = maker.write_dataset(args.output, epoch=args.epoch, bits_per_sample=args.bits, tar=not args.no_tar,
                                  block_size=args.block_size, lpc_order=args.lpc_order)
    total = time.perf_counter() - t0
    audio = sum(maker.draw(args.epoch)[i]['frames'] for i in range(args.size))/args.fs
    print(f'{args.size} mixtures, {audio:.1f} s of audio per source, written in {total:.2f} s: ' +
          ', '.join(f'{k} {v:.2f} s' for k, v in seconds.items()))


if __name__ == '__main__':
    main()
