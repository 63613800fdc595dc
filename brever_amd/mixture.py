"""Batched mixture synthesis on the GPU: ``brever.mixture.mixture.Mixture`` for a batch of ragged mixtures.

The reference builds one mixture at a time on the CPU (``RandomMixtureMaker.make_from_metadata``): add_speech
with the early / late windows of ``split_brir``, add_noises, the diffuse sum, set_ndr, set_snr over
``speech_idx``, set_tmr, ``set_rms(get_rms() + jitter)`` -- six or more long ``oaconvolve`` calls. Here a whole
batch goes through one fixed launch sequence with no host round trip (the gains stay on the device):

    gather signals / BRIRs from pools, split_brir        brv_mix_pack_signals, brv_mix_pack_brirs
    block DFTs of signals and BRIR partitions            brv_dft64_forward   (main library, fp64 matrix pipe)
    per-bin partition multiply-accumulate, both ears     brv_mix_partition_mac
    inverse block DFTs, the valid half only              brv_dft64_synthesis
    energy sums in fp64, gains and labels                brv_mix_energies, brv_mix_gains
    gain-and-sum of the requested components             brv_mix_compose

The convolution is a uniformly partitioned overlap-save product with block ``B``: frames of ``2B`` samples at
hop ``B``; the BRIR partitions are transformed with the first ``B`` columns of the same DFT basis (their zero
padding costs nothing) and only the last ``B`` samples of every output frame are synthesised.

Reference quirks kept: every spatialised signal is truncated to its input length; with ``padding > 0`` the
speech is padded before AND after spatialisation, so a target of L samples gives L + 4 n_pad and ``speech_idx =
(n_pad, n_pad + L)``; energies are those of the channel mean; a zero target or noise energy is a ValueError
(raised by ``MixtureBatch.check``, after the batch has run).

``PoolMixtureMaker`` plugs this into ``BreverDataset(dynamic_mixing=True)`` (``data.set_mixture_maker``).
There is no CPU fallback: without ``libbrever_mix.so`` or a ROCm device the calls raise.
"""
import ctypes
import os

import numpy as np
import torch

from . import hip

COMPONENTS = ('mixture', 'foreground', 'background', 'speech', 'noise', 'early_speech', 'late_speech',
              'dir_noise', 'diffuse')
EN_CHUNK = 2048          # samples per partial energy sum (csrc/mix/mix.hip)
MAX_PARTS = 512          # partitions per impulse response the LDS tile of the product holds

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BRV_MIX_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libbrever_mix.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'brever_mix.h')


def _header_signatures():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f'{HEADER_PATH} is missing: the binding is derived from the C header')
    with open(HEADER_PATH) as f:
        return hip.parse_header(f.read())


# name -> (restype, argtypes) of every brv_mix_* entry point, read from include/brever_mix.h
SIGNATURES = _header_signatures()
_lib = None


def lib():
    """Load ``libbrever_mix.so`` once; fail loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; '
                               'g.build()"` or `make -C brever_amd/csrc` (needs hipcc, targets gfx950). '
                               'The mixture engine has no CPU fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


def call(name, *args):
    """Call the ``brv_mix_*`` entry point ``name``; a non-zero status raises with the library's message."""
    status = getattr(lib(), name)(*args)
    if status:
        msg = lib().brv_mix_last_error()
        raise RuntimeError(f'{name} failed with status {status}: {msg.decode() if msg else ""}')


_tables = {}


def dft_tables(block, device):
    """float64 DFT bases of the overlap-save transform of size ``2*block``, rows (re_k, im_k) interleaved as
    ``brv_dft64_forward`` takes them: ``signal`` (2 bins, 2B) for the signal frames, ``partition`` (2 bins, B) =
    its first B columns (a partition is B taps and B zeros), ``inverse`` (2 bins, B) = the columns of the
    inverse one-sided transform for the last B samples of a frame (the ones overlap-save keeps)."""
    key = (int(block), str(device))
    if key not in _tables:
        n, bins = 2*block, block + 1
        k = np.arange(bins)[:, None]
        m = np.arange(n)[None, :]
        ang = 2*np.pi*((k*m) % n)/n
        fwd = np.empty((2*bins, n))
        fwd[0::2], fwd[1::2] = np.cos(ang), -np.sin(ang)
        w = np.full((bins, 1), 2.0/n)
        w[0] = w[-1] = 1.0/n
        inv = np.empty((2*bins, n))
        inv[0::2], inv[1::2] = w*np.cos(ang), -w*np.sin(ang)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
        _tables[key] = dict(signal=up(fwd), partition=up(fwd[:, :block]), inverse=up(inv[:, block:]))
    return _tables[key]


class MixtureBatch:
    """What one batch gave, all on the device: ``components[name]`` (mixtures, max length, 2) float32 with
    zeros behind each mixture's length, ``lengths`` and ``speech_idx`` (host lists), ``labels`` (mixtures, 3)
    float64 = (tmr, tnr, trr), ``gains`` (mixtures, 8) float64 = the factors of (early, late, dir, diffuse) and
    the reference's (ndr, snr, tmr, rms) gains, ``status`` (mixtures) int32."""

    def __init__(self, components, lengths, speech_idx, labels, gains, status):
        self.components, self.lengths, self.speech_idx = components, lengths, speech_idx
        self.labels, self.gains, self.status = labels, gains, status

    def check(self):
        """Wait for the batch and raise the reference's ValueError for a zero energy."""
        return self.raise_for(self.status.cpu().tolist())

    def raise_for(self, status):
        """The same for status words already on the host."""
        for i, st in enumerate(status):
            if st == 1:
                raise ValueError(f'mixture {i}: cannot scale noise signal if target signal is 0')
            if st == 2:
                raise ValueError(f'mixture {i}: cannot scale noise signal if it equals 0')
        return self

    def item(self, i, name):
        """Component ``name`` of mixture ``i``, (frames, 2)."""
        return self.components[name][i, :self.lengths[i]]


def _nan(v):
    return float('nan') if v is None else float(v)


def synthesize(pools, brir_pool, specs, components=COMPONENTS, padding=0.0, fs=16000, reflection_boundary=50e-3,
               max_itd=1e-3, block=256):
    """Run one batch. ``pools``: list of 1-D float32 device tensors holding signals; ``brir_pool``: 1-D float32
    device tensor holding interleaved (taps, 2) BRIRs. ``specs``: one dict per mixture --

        target=(pool, offset, n)  brir=(offset, taps)
        noises=[((pool, offset, n), (offset, taps)), ...]        directional noises, n = the mixture's length
        diffuse=[((pool, offset, n), (offset, taps)), ...]       diffuse noise signals drawn by the caller
        ndr=, snr=, tmr=, rms_jitter=                             None / absent: step not taken (jitter 0)
        n_pad=                                                    zeros around the speech, else round(padding*fs)

    Only descriptors go to the device; nothing comes back. Returns a ``MixtureBatch``."""
    pools = list(pools)
    hip.require_device(brir_pool, *pools)
    for t in pools + [brir_pool]:
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() < 1:
            raise ValueError('pools are non-empty contiguous 1-D float32 tensors')
    comp_ids = [COMPONENTS.index(c) for c in components]
    if not specs or not comp_ids:
        raise ValueError('needs at least one mixture and one component')
    device, B = brir_pool.device, int(block)
    M = len(specs)
    sig_rows = [[] for _ in pools]      # per pool: (src, n, dst, key)
    hdesc, jobs, slots, mixd, params, lengths, idx = [], [], [], [], [], [], []
    pending = []                        # (slot jobs as (signal key, h job, parts)) resolved once rows are numbered
    for s, spec in enumerate(specs):
        pool, off, n = spec['target']
        n_pad = spec['n_pad'] if spec.get('n_pad') is not None else round(padding*fs)
        T = n + 4*n_pad
        frames = -(-T//B)
        lengths.append(T)
        idx.append((n_pad, n_pad + n))
        mixd.append((T, T - n_pad, n_pad, n_pad + n))
        params.append([_nan(spec.get('ndr')), _nan(spec.get('snr')), _nan(spec.get('tmr')),
                       float(spec.get('rms_jitter') or 0.0)])
        sig_rows[pool].append((off, n, 2*n_pad, (s, 't')))
        groups = [[], [], [], []]
        for mode, g in ((1, 0), (2, 1)):
            boff, taps = spec['brir']
            hdesc.append((boff, taps, mode))
            groups[g].append(((s, 't'), len(hdesc) - 1, min(-(-taps//B), frames)))
        for g, name in ((2, 'noises'), (3, 'diffuse')):
            for j, ((pool, off, n), (boff, taps)) in enumerate(spec.get(name) or []):
                if n != T:
                    raise ValueError(f'mixture {s}: {name}[{j}] has {n} samples, the mixture has {T}')
                sig_rows[pool].append((off, n, 0, (s, name, j)))
                hdesc.append((boff, taps, 0))
                groups[g].append(((s, name, j), len(hdesc) - 1, min(-(-taps//B), frames)))
        pending.append((groups, frames))
    for boff, taps, _ in hdesc:
        if taps < 1 or boff < 0 or boff + 2*taps > brir_pool.numel():
            raise ValueError('a BRIR lies outside brir_pool')
    row_of, r = {}, 0
    for pool, rows in enumerate(sig_rows):
        for off, n, dst, key in rows:
            if n < 1 or off < 0 or off + n > pools[pool].numel():
                raise ValueError(f'a signal lies outside pool {pool}')
            row_of[key] = r
            r += 1
    for groups, frames in pending:
        for g in groups:
            slots.append((len(jobs), len(jobs) + len(g), frames))
            jobs.extend((row_of[key], 2*h, parts) for key, h, parts in g)
    xrows, hjobs = r, len(hdesc)
    Tmax = max(lengths)
    F = -(-Tmax//B)
    Pmax = max(j[2] for j in jobs)
    if Pmax > MAX_PARTS:
        raise ValueError(f'a BRIR spans {Pmax} blocks of {B}; at most {MAX_PARTS}: use a larger block')
    if max(xrows, 2*hjobs, 8*M) > 65535:
        raise ValueError('batch too large: at most 65535 signal rows, BRIR rows and 8 x mixtures')
    bins, st = B + 1, hip.stream()
    tb = dft_tables(B, device)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(device, non_blocking=True)

    f32 = dict(dtype=torch.float32, device=device)
    xs = torch.empty(xrows, Tmax, **f32)
    r = 0
    for pool, rows in enumerate(sig_rows):
        if rows:
            d = up([row[:3] for row in rows], np.int64)
            call('brv_mix_pack_signals', pools[pool], d, xs[r:], pools[pool].numel(), len(rows), Tmax, st)
            r += len(rows)
    hs = torch.empty(2*hjobs, Pmax*B, **f32)
    call('brv_mix_pack_brirs', brir_pool, up(hdesc, np.int64), hs, brir_pool.numel(), hjobs, Pmax*B,
         round(reflection_boundary*fs), max(round(max_itd*fs), 1), st)
    xspec = torch.empty(xrows, bins, F, 2, **f32)
    hip.call('brv_dft64_forward', xs, tb['signal'], xspec, xrows, Tmax, 2*B, B, B, F, bins, 1.0, 1.0, st)
    hspec = torch.empty(2*hjobs, bins, Pmax, 2, **f32)
    hip.call('brv_dft64_forward', hs, tb['partition'], hspec, 2*hjobs, Pmax*B, B, B, 0, Pmax, bins, 1.0, 1.0, st)
    yspec = torch.empty(8*M, bins, F, 2, **f32)
    call('brv_mix_partition_mac', xspec, hspec, yspec, up(slots, np.int32), up(jobs, np.int32), 4*M, len(jobs),
         xrows, F, 2*hjobs, Pmax, bins, F, Pmax, st)
    y = torch.empty(8*M, F*B, **f32)
    hip.call('brv_dft64_synthesis', yspec, tb['inverse'], y, 8*M, F, B, bins, 1.0, 1.0, st)
    chunks = -(-F*B//EN_CHUNK)
    mix_d = up(mixd, np.int32)
    f64 = dict(dtype=torch.float64, device=device)
    partials = torch.empty(M, chunks, 40, **f64)
    call('brv_mix_energies', y, mix_d, partials, M, F*B, chunks, st)
    gains, labels = torch.empty(M, 8, **f64), torch.empty(M, 3, **f64)
    status = torch.empty(M, dtype=torch.int32, device=device)
    call('brv_mix_gains', partials, mix_d, up(params, np.float64), gains, labels, status, M, chunks, st)
    out = torch.empty(len(comp_ids), M, Tmax, 2, **f32)
    call('brv_mix_compose', y, gains, mix_d, up(comp_ids, np.int32), out, len(comp_ids), M, F*B, Tmax, st)
    return MixtureBatch({c: out[k] for k, c in enumerate(components)}, lengths, idx, labels, gains, status)


def mix(targets, brirs, noises=None, noise_brirs=None, diffuse=None, diffuse_brirs=None, ndr=None, snr=None,
        tmr=None, rms_jitter=None, padding=0.0, fs=16000, **kw):
    """``synthesize`` for lists of device tensors, one entry per mixture: ``targets[i]`` (n,), ``brirs[i]``
    (taps, 2), ``noises[i]`` / ``noise_brirs[i]`` and ``diffuse[i]`` / ``diffuse_brirs[i]`` lists of signals of
    the mixture's length and their BRIRs, ``ndr[i]`` ... ``rms_jitter[i]`` numbers or None, ``padding`` one
    number or one per mixture."""
    M = len(targets)
    sig, sig_off, hh, h_off = [], [0], [], [0]

    def add_signal(x):
        x = x.reshape(-1).float()
        sig.append(x)
        sig_off.append(sig_off[-1] + x.numel())
        return (0, sig_off[-2], x.numel())

    def add_brir(h):
        if h.dim() != 2 or h.shape[1] != 2:
            raise ValueError('a BRIR is (taps, 2)')
        hh.append(h.float().reshape(-1))
        h_off.append(h_off[-1] + 2*h.shape[0])
        return (h_off[-2], h.shape[0])

    specs = []
    for i in range(M):
        spec = dict(target=add_signal(targets[i]), brir=add_brir(brirs[i]))
        for name, xs, hs in (('noises', noises, noise_brirs), ('diffuse', diffuse, diffuse_brirs)):
            xi, hi = (xs[i] if xs else []) or [], (hs[i] if hs else []) or []
            if len(xi) != len(hi):
                raise ValueError('xs and brirs must have same number of elements')
            spec[name] = [(add_signal(x), add_brir(h)) for x, h in zip(xi, hi)]
        for name, v in (('ndr', ndr), ('snr', snr), ('tmr', tmr), ('rms_jitter', rms_jitter)):
            spec[name] = None if v is None else v[i]
        spec['n_pad'] = round((padding[i] if isinstance(padding, (list, tuple)) else padding)*fs)
        specs.append(spec)
    return synthesize([torch.cat(sig)], torch.cat(hh), specs, fs=fs, **kw)


class PoolMixtureMaker:
    """Mixture maker in the ``set_mixture_maker`` protocol that synthesises every epoch on the GPU from
    in-memory pools: ``speech`` and ``noises`` lists of 1-D arrays, ``brirs`` a list of rooms, each a list of
    (taps, 2) arrays (one per angle) -- passed in, or loaded from ``path`` (a ``.npz`` with ``speech_<i>``,
    ``noise_<i>``, ``brir_<room>_<angle>`` arrays).

    Per epoch a host RNG seeded with ``(seed, epoch)`` draws, per mixture: target, room, target angle, the
    number of directional noises with their file, start and angle, SNR, NDR (with ``diffuse=True``: one white
    noise per angle of the room, drawn on the device from a seed of the mixture's own) and the RMS jitter. ``set_epoch``
    synthesises the epoch in batches and keeps the requested sources in pinned host memory; the same
    ``(seed, epoch)`` gives bitwise the same mixtures.

    Out of scope: corpus scanning, SOFA / audio file input, ``colored_noise`` other than
    white, ``match_ltas`` and ``BRIRDecay``."""

    def __init__(self, path, sources, size, speech=None, noises=None, brirs=None, seed=0, fs=16000, padding=0.0,
                 noise_count=(0, 3), snr=(-5.0, 10.0), ndr=(0.0, 30.0), diffuse=False, rms_jitter=(0.0, 0.0),
                 batch=64, block=256, device='cuda'):
        if speech is None:
            speech, noises, brirs = self._load(path)
        self.sources, self.size, self.seed, self.fs = list(sources), int(size), int(seed), fs
        for s in self.sources:
            if s not in COMPONENTS:
                raise ValueError(f'unknown source {s!r}; one of {COMPONENTS}')
        self.padding, self.noise_count, self.snr, self.ndr = padding, tuple(noise_count), tuple(snr), tuple(ndr)
        self.diffuse, self.rms_jitter, self.batch, self.block = bool(diffuse), tuple(rms_jitter), int(batch), block
        self.device = device
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)                    # noqa: E731
        self._speech = [f32(x).reshape(-1) for x in speech]
        self._noises = [f32(x).reshape(-1) for x in (noises or [])]
        self._brirs = [[f32(h) for h in room] for room in brirs]
        if not self._speech or not self._brirs or any(not room for room in self._brirs):
            raise ValueError('needs at least one speech signal and one room with one BRIR')
        if any(h.ndim != 2 or h.shape[1] != 2 for room in self._brirs for h in room):
            raise ValueError('a BRIR is (taps, 2)')
        # offsets of every pooled array in the two flat device tensors (uploaded on first use)
        self._sig_off = np.cumsum([0] + [len(x) for x in self._speech + self._noises]).tolist()
        flat = [h for room in self._brirs for h in room]
        off = np.cumsum([0] + [h.size for h in flat]).tolist()
        self._brir_ref, k = [], 0
        for room in self._brirs:
            self._brir_ref.append([(off[k + a], room[a].shape[0]) for a in range(len(room))])
            k += len(room)
        self._pools = None
        self._epoch, self._meta, self._items = 0, self.draw(0), None

    @staticmethod
    def _load(path):
        with np.load(path) as z:
            def numbered(prefix):
                keys = sorted((k for k in z.files if k.startswith(prefix)), key=lambda k: int(k[len(prefix):]))
                return [z[k] for k in keys]
            rooms = {}
            for k in z.files:
                if k.startswith('brir_'):
                    room, angle = (int(v) for v in k[5:].split('_'))
                    rooms.setdefault(room, {})[angle] = z[k]
            brirs = [[rooms[r][a] for a in sorted(rooms[r])] for r in sorted(rooms)]
            return numbered('speech_'), numbered('noise_'), brirs

    # -- the epoch's draws (host only) ------------------------------------------------------------------------
    def draw(self, epoch):
        """The metadata of every mixture of ``epoch``: a list of dicts, a function of ``(seed, epoch)`` only."""
        rng = np.random.default_rng([self.seed, int(epoch)])
        n_pad = round(self.padding*self.fs)
        meta = []
        for _ in range(self.size):
            t = int(rng.integers(len(self._speech)))
            room = int(rng.integers(len(self._brirs)))
            angles = len(self._brirs[room])
            m = dict(target=t, room=room, angle=int(rng.integers(angles)), frames=len(self._speech[t]) + 4*n_pad)
            fits = [i for i, x in enumerate(self._noises) if len(x) >= m['frames']]
            count = int(rng.integers(self.noise_count[0], self.noise_count[1] + 1)) if fits else 0
            m['noises'] = []
            for _ in range(count):
                f = fits[int(rng.integers(len(fits)))]
                m['noises'].append(dict(file=f, i_start=int(rng.integers(len(self._noises[f]) - m['frames'] + 1)),
                                        angle=int(rng.integers(angles))))
            m['diffuse'] = self.diffuse
            # the white noises of a mixture come from a generator of its own: no function of the batch it is in
            m['diffuse_seed'] = int(rng.integers(2**62)) if self.diffuse else None
            m['snr'] = float(rng.uniform(*self.snr)) if (count or self.diffuse) else None
            m['ndr'] = float(rng.uniform(*self.ndr)) if (count and self.diffuse) else None
            m['rms_jitter'] = float(rng.uniform(*self.rms_jitter))
            meta.append(m)
        return meta

    @property
    def file_lengths(self):
        return [m['frames'] for m in self._meta]

    # -- synthesis ------------------------------------------------------------------------------------------------
    def _spec(self, m, diffuse_refs):
        ns = len(self._speech)
        spec = dict(target=(0, self._sig_off[m['target']], len(self._speech[m['target']])),
                    brir=self._brir_ref[m['room']][m['angle']], snr=m['snr'], ndr=m['ndr'],
                    rms_jitter=m['rms_jitter'])
        spec['noises'] = [((0, self._sig_off[ns + n['file']] + n['i_start'], m['frames']),
                           self._brir_ref[m['room']][n['angle']]) for n in m['noises']]
        spec['diffuse'] = list(zip(diffuse_refs, self._brir_ref[m['room']])) if m['diffuse'] else []
        return spec

    def synthesize(self, meta):
        """One batch of drawn mixtures on the device (``MixtureBatch`` of ``self.sources``)."""
        if self._pools is None:
            dev = torch.device(self.device)
            self._pools = (torch.from_numpy(np.concatenate(self._speech + self._noises)).to(dev),
                           torch.from_numpy(np.concatenate([h.reshape(-1) for room in self._brirs for h in room])).to(dev))
        signals, brir_pool = self._pools
        refs, drawn, total = [], [], 0
        for m in meta:
            k = len(self._brirs[m['room']]) if m['diffuse'] else 0
            refs.append([(1, total + a*m['frames'], m['frames']) for a in range(k)])
            if k:
                g = torch.Generator(device=signals.device).manual_seed(m['diffuse_seed'])
                drawn.append(torch.randn(k*m['frames'], generator=g, device=signals.device, dtype=torch.float32))
            total += k*m['frames']
        pools = [signals] + ([torch.cat(drawn)] if drawn else [])
        specs = [self._spec(m, r) for m, r in zip(meta, refs)]
        return synthesize(pools, brir_pool, specs, components=self.sources, padding=self.padding, fs=self.fs,
                          block=self.block)

    def set_epoch(self, epoch):
        self._epoch, self._meta = int(epoch), self.draw(epoch)
        self._items, queue = [None]*self.size, []

        def finish(res, host, start, status, event):   # wait for ONE batch; only its pinned copies stay alive
            event.synchronize()
            res.raise_for(status.tolist())
            for j, T in enumerate(res.lengths):
                self._items[start + j] = [host[name][j, :T].numpy() for name in self.sources]

        for start in range(0, self.size, self.batch):
            res = self.synthesize(self._meta[start:start + self.batch])
            host = {}
            for name in self.sources:
                dev = res.components[name]
                host[name] = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
                host[name].copy_(dev, non_blocking=True)
            status = torch.empty(res.status.shape, dtype=res.status.dtype, pin_memory=True)
            status.copy_(res.status, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            queue.append((res, host, start, status, event))
            if len(queue) > 2:                 # two batches stay queued behind the one being waited for
                finish(*queue.pop(0))
        while queue:
            finish(*queue.pop(0))

    def __getitem__(self, i):
        if self._items is None:
            self.set_epoch(self._epoch)
        return self._items[i]
