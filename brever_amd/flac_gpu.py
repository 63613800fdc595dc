"""FLAC dataset members decoded on the GPU (``libbrever_flac.so``, include/brever_flac.h).

``index(blob)`` is host work: STREAMINFO and the table of the stream's frames, found without entropy decoding and
accepted only with matching CRC-8, running number and CRC-16. ``FlacBatchDecoder.decode`` turns the frames that
overlap each item's window into jobs, makes ONE pinned upload of the concatenated members and the job table on the
current stream and launches the two kernels of ``brv_flacdec_decode``: no host synchronisation. The per-job status
is reduced on the device and read once by ``FlacBatch.check`` (the ``MixtureBatch.check`` pattern), which raises a
``ValueError`` naming the member.

The host decoder of ``csrc/flac.hip`` stays the path of DataLoader worker processes and of the members the index
declines (more than 24 bits per sample): those are decoded on the host and copied in, logged once per decoder.
There is no other fallback: without the library or a ROCm device the calls raise.
"""
import ctypes
import logging

import numpy as np
import torch

from . import hip

# in place of an ``index`` result: the index declined the member (``NOT_TAKEN``), the host decoder reads it
HOST_MEMBER = 'host'
INFO_FIELDS = ('sample_rate', 'channels', 'bits_per_sample', 'total_samples', 'min_block', 'max_block',
               'first_frame', 'variable')


# the brv_flacdec_* entry points of include/brever_flac.h
_LIB = hip.Library('brever_flac.h', 'libbrever_flac.so', 'BRV_FLAC_LIB_PATH', 'The GPU FLAC decoder has no fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, last_error = _LIB.lib, _LIB.call, _LIB.last_error
# the header's BRV_FLACDEC_* constants: table widths in words, index statuses, job statuses
INFO_WORDS, FRAME_WORDS, JOB_WORDS, NOT_TAKEN, NOT_FLAC, BAD_HEADER, BAD_CRC16, BAD_NUMBER, TRUNCATED = (
    _LIB.constants['BRV_FLACDEC_' + name] for name in (
        'INFO_WORDS', 'FRAME_WORDS', 'JOB_WORDS', 'NOT_TAKEN', 'NOT_FLAC', 'BAD_HEADER', 'BAD_CRC16', 'BAD_NUMBER',
        'TRUNCATED'))
JOB_MESSAGES = {_LIB.constants['BRV_FLACDEC_JOB_' + name]: text for name, text in (
    ('BAD_FIELDS', 'job fields outside the extents of the call'),
    ('RESERVED', 'reserved or invalid field in a subframe'), ('OVERRUN', "the frame's bits ran out"),
    ('LENGTH', 'the frame does not end where the index says'))}


class FlacIndexError(ValueError):
    """A stream ``index`` does not take; ``code`` is the library's (``NOT_TAKEN`` ... ``TRUNCATED``)."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


def index(blob, name='<bytes>'):
    """``(info, frames)`` of the FLAC stream ``blob``: ``info`` a dict of ``INFO_FIELDS``, ``frames`` an int64
    array (n, 8) = (byte offset, byte length, first sample, block size, channel assignment, sample size, header
    bytes, coded number). Host work only. Raises ``FlacIndexError``."""
    blob = bytes(blob)
    info = np.zeros(INFO_WORDS, dtype=np.int64)
    # a first guess from the stream's own block size (STREAMINFO's, bytes 10-11); the count comes back either way
    capacity = 64
    if len(blob) >= 26:
        total = int.from_bytes(blob[21:26], 'big') & ((1 << 36) - 1)
        capacity = max(capacity, total//max(int.from_bytes(blob[8:10], 'big'), 1) + 2)
    capacity = min(capacity, max(len(blob)//8, 64))
    while True:
        frames = np.zeros((capacity, FRAME_WORDS), dtype=np.int64)
        n = lib().brv_flacdec_index(blob, len(blob), info.ctypes.data_as(ctypes.c_void_p),
                                    frames.ctypes.data_as(ctypes.c_void_p), capacity)
        if n < 0:
            raise FlacIndexError(int(n), f'{name}: {last_error()} (status {n})')
        if n <= capacity:
            return dict(zip(INFO_FIELDS, info.tolist())), frames[:n]
        capacity = int(n)


class FlacBatch:
    """What ``FlacBatchDecoder.decode`` gave: ``data`` (items, sources, channels, L_max) float32 on the device
    with zeros behind each item's length, ``lengths`` (a host list), ``sample_rates`` per item, ``status`` (jobs)
    int32 on the device."""

    def __init__(self, data, lengths, sample_rates, status, job_names):
        self.data, self.lengths, self.sample_rates, self.status = data, lengths, sample_rates, status
        self._job_names = job_names
        # reduced on the device now, read once in check(): (number of failed jobs, the first of them, its status)
        if status is None:
            self.summary = None
        else:
            bad = status.ne(0)
            first = bad.to(torch.int32).argmax()
            self.summary = torch.stack([bad.sum(), first, status[first].to(torch.int64)])

    def check(self):
        """Wait for the batch and raise ``ValueError`` naming the member of the first frame that did not decode."""
        if self.summary is not None:
            n_bad, first, st = self.summary.tolist()
            if n_bad:
                member, frame = self._job_names(first)
                raise ValueError(f'{member}: FLAC frame {frame} did not decode on the GPU: '
                                 f'{JOB_MESSAGES.get(st, st)} ({n_bad} frame(s) failed)')
        return self


class FlacBatchDecoder:
    """Decodes batches of FLAC members on ``device``. One instance per consumer: it keeps reusable pinned staging
    buffers, so two batches in flight need two decoders, or a ``slot`` each (``DevicePrefetcher`` does that)."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError(f'the GPU FLAC decoder runs on a ROCm device only; got {self.device} '
                               '(brv_flac_decode is the host decoder)')
        lib()
        self._pinned, self._fences = {}, {}
        self._logged_host = False

    def _pin(self, key, nbytes):
        buf = self._pinned.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
            self._pinned[key] = buf
        return buf

    def _host_decode(self, blob, name):
        import io
        from .data import audio_read
        if not self._logged_host:
            logging.info(f'{name}: not taken by the GPU FLAC decoder; such members are decoded on the host')
            self._logged_host = True
        x, rate = audio_read(io.BytesIO(blob), name if name.lower().endswith('.flac') else name + '.flac')
        x = np.asarray(x, dtype=np.float32)
        x = x[None, :] if x.ndim == 1 else np.ascontiguousarray(x.T)
        return x, rate                                       # (channels, frames)

    def decode(self, members, windows=None, names=None, tables=None, slot=0, pad_offsets=None, events=None):
        """``members[item][source]``: the bytes of a FLAC stream. ``windows[item]``: ``(start, end)`` in samples,
        ``None`` for the whole member; a window may end beyond the member (zeros). ``names`` (same nesting) go
        into error messages, ``tables[item][source]`` are ``index`` results the caller already has (``HOST_MEMBER``
        where it declined the member).
        ``pad_offsets``: bytes of padding in front of each member in the upload (a test's way to place members
        at any alignment). ``events``: a list that gets a pair of ``torch.cuda.Event`` around the two kernels
        (tools/flac_bench.py). Returns a ``FlacBatch``; nothing here waits for the device."""
        n_items = len(members)
        if n_items == 0:
            raise ValueError('empty batch')
        n_src = len(members[0])
        flat, metas, host = [], [], []                       # host: (item, source, channels x frames array)
        for i, row in enumerate(members):
            if len(row) != n_src:
                raise ValueError(f'item {i} has {len(row)} sources, item 0 has {n_src}')
            first = None
            for s, blob in enumerate(row):
                name = names[i][s] if names is not None else f'item {i} source {s}'
                table = tables[i][s] if tables is not None else None
                if table is None:
                    try:
                        table = index(blob, name)
                    except FlacIndexError as e:
                        if e.code != NOT_TAKEN:
                            raise
                        table = HOST_MEMBER
                if isinstance(table, str) and table == HOST_MEMBER:
                    x, rate = self._host_decode(bytes(blob), name)
                    table = (dict(sample_rate=rate, channels=x.shape[0], total_samples=x.shape[1], max_block=0), None)
                    host.append((i, s, x))
                info = table[0]
                key = (info['sample_rate'], info['channels'])
                if first is None:
                    first = key
                elif key != first:
                    raise ValueError(f'{name}: sample rate / channels {key} differ from {first} of the same item')
                flat.append((i, s, name, bytes(blob) if table[1] is not None else b'', table))
            metas.append(first)
        channels = max(m[1] for m in metas)
        if any(m[1] != channels for m in metas):
            raise ValueError(f'items of one batch differ in channel count: {sorted(set(m[1] for m in metas))}')
        # windows and lengths
        lengths, wins = [], []
        for i in range(n_items):
            totals = [t[4][0]['total_samples'] for t in flat if t[0] == i]
            if windows is None or windows[i] is None:
                if any(n != totals[0] for n in totals):
                    raise ValueError(f'item {i}: sources do not all have the same length: {totals}')
                wins.append((0, totals[0]))
            else:
                start, end = int(windows[i][0]), int(windows[i][1])
                if start < 0 or end < start:
                    raise ValueError(f'item {i}: window ({start}, {end}) is not 0 <= start <= end')
                wins.append((start, end))
            lengths.append(wins[-1][1] - wins[-1][0])
        l_max = max(max(lengths), 1)
        out = torch.zeros((n_items, n_src, channels, l_max), dtype=torch.float32, device=self.device)
        # jobs: the frames that overlap the window
        parts, offsets, job_rows, job_member = [], [], [], []
        cursor, max_block = 0, 1
        for m, (i, s, name, blob, table) in enumerate(flat):
            frames = table[1]
            if frames is None or len(frames) == 0:
                offsets.append(None)
                continue
            start, end = wins[i]
            f0, bs = frames[:, 2], frames[:, 3]
            lo = np.maximum(start, f0) - f0
            hi = np.minimum(end, f0 + bs) - f0
            keep = np.nonzero(lo < hi)[0]
            if len(keep) == 0:
                offsets.append(None)
                continue
            cursor += int(pad_offsets[m]) if pad_offsets is not None else 0
            # only the bytes of the frames that are decoded travel
            b0 = int(frames[keep[0], 0])
            b1 = int(frames[keep[-1], 0] + frames[keep[-1], 1])
            parts.append((cursor, blob[b0:b1]))
            rows = np.zeros((len(keep), JOB_WORDS), dtype=np.int64)
            fk = frames[keep]
            rows[:, 0] = fk[:, 0] - b0 + cursor
            rows[:, 1] = fk[:, 1]
            rows[:, 2] = fk[:, 3]
            rows[:, 3] = fk[:, 4]
            rows[:, 4] = fk[:, 5]
            rows[:, 5] = fk[:, 6]
            rows[:, 6] = lo[keep]
            rows[:, 7] = hi[keep]
            rows[:, 8] = ((i*n_src + s)*channels)*l_max + (fk[:, 2] + lo[keep] - start)
            rows[:, 9] = l_max
            rows[:, 10] = m
            rows[:, 11] = keep
            job_rows.append(rows)
            max_block = max(max_block, int(fk[:, 3].max()))
            cursor += b1 - b0
        status = None
        jobs_np = None
        if job_rows:
            jobs_np = np.concatenate(job_rows)
            n_jobs = len(jobs_np)
            nbytes = (cursor + 3)//4*4
            job_bytes = jobs_np.size*8
            # one pinned buffer, one upload: the job table (8-byte aligned) first, the members' bytes behind it
            if slot in self._fences:
                self._fences[slot].synchronize()             # the upload that last used this slot's buffer is done
            stage = self._pin(slot, job_bytes + nbytes)
            view = stage.numpy()
            view[:job_bytes] = jobs_np.reshape(-1).view(np.uint8)
            view[job_bytes + cursor:job_bytes + nbytes] = 0
            for off, chunk in parts:
                view[job_bytes + off:job_bytes + off + len(chunk)] = np.frombuffer(chunk, dtype=np.uint8)
            dev = torch.empty(job_bytes + nbytes, dtype=torch.uint8, device=self.device)
            dev.copy_(stage[:job_bytes + nbytes], non_blocking=True)
            fence = torch.cuda.Event()
            fence.record()
            self._fences[slot] = fence
            need = int(lib().brv_flacdec_scratch_elems(n_jobs, channels, max_block))
            if need < 0:
                raise RuntimeError(f'brv_flacdec_scratch_elems failed with status {need}: {last_error()}')
            scratch = torch.empty(need, dtype=torch.int32, device=self.device)
            status = torch.empty(n_jobs, dtype=torch.int32, device=self.device)
            if events is not None:
                events.append(torch.cuda.Event(enable_timing=True))
                events[-1].record()
            call('brv_flacdec_decode', dev[job_bytes:], nbytes, dev, n_jobs, channels, max_block, scratch, need, out,
                 out.numel(), status, hip.stream())
            if events is not None:
                events.append(torch.cuda.Event(enable_timing=True))
                events[-1].record()
        for i, s, x in host:                                 # the members the index declined
            start, end = wins[i]
            piece = x[:, start:min(end, x.shape[1])]
            if piece.shape[1]:
                out[i, s, :, :piece.shape[1]] = torch.from_numpy(np.ascontiguousarray(piece)).to(self.device)
        names_of = [t[2] for t in flat]

        def job_names(j):
            return names_of[int(jobs_np[j, 10])], int(jobs_np[j, 11])
        return FlacBatch(out, lengths, [m[0] for m in metas], status, job_names)
