"""Batches of signals encoded as FLAC on the GPU (``libbrever_flacenc.so``, include/brever_flacenc.h):
the counterpart of ``flac_gpu.FlacBatchDecoder``.

``FlacBatchEncoder.encode`` takes a padded device batch ``(B, C, L)`` (or ``(B, L)``) with per-row lengths and
returns one complete FLAC stream of RFC 9639 per row as ``bytes``: mono or stereo, 16 or 24 bits, CONSTANT / VERBATIM
/ FIXED / LPC subframes chosen by exact coded size, partitioned Rice residuals, all four stereo decorrelations. The
samples never travel to the host as float32; what is downloaded is the offset table (a few words per row) and then
the compressed bytes in one copy. ``submit`` is the same without waiting: it queues the kernels and the table's copy
on the current stream and returns a ``PendingStreams`` whose ``result()`` waits for that batch only and downloads
the bytes on a side stream, so that a writer can overlap it with whatever it queued in between.

``brv_flac_encode16`` of the main library (mono, 16 bits, FIXED predictors; ``data.flac_bytes``) is untouched.
There is no fallback: without the library or a ROCm device the calls raise.
"""
import torch

from . import hip

# the brv_flacenc_* entry points of include/brever_flacenc.h
_LIB = hip.Library('brever_flacenc.h', 'libbrever_flacenc.so', 'BRV_FLACENC_LIB_PATH',
                   'The GPU FLAC encoder has no fallback.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, call, last_error = _LIB.lib, _LIB.call, _LIB.last_error
# the header's BRV_FLACENC_* constants: the bits of a row's status, the limits of a call
ROW_MESSAGES = {_LIB.constants['BRV_FLACENC_ROW_' + name]: text for name, text in (
    ('NONFINITE', 'a non-finite sample'), ('RANGE', 'a PCM sample outside the range of the bit depth'),
    ('LENGTH', 'a length outside 1 ... the padded length'), ('INTERNAL', 'a frame did not fit its image'))}
MAX_ROWS, MAX_LPC_ORDER = _LIB.constants['BRV_FLACENC_MAX_ROWS'], _LIB.constants['BRV_FLACENC_MAX_LPC_ORDER']


def query(name, *args):
    """A size query of the library; a negative answer is the caller's ``ValueError`` with the library's message, its
    arguments named (``Library.query`` raises ``RuntimeError``)."""
    n = int(getattr(lib(), name)(*args))
    if n < 0:
        raise ValueError(f'{name}{args}: {last_error()}')
    return n


def status_message(status):
    return ', '.join(text for bit, text in ROW_MESSAGES.items() if status & bit) or f'status {status}'


class PendingStreams:
    """A batch that ``FlacBatchEncoder.submit`` queued. ``result()`` gives the ``list[bytes]``."""

    def __init__(self, encoder, out, table_dev, table_host, event, rows, keep):
        self._encoder, self._out, self._table_dev, self._table = encoder, out, table_dev, table_host
        self._event, self._rows, self._keep = event, rows, keep
        self._streams = None
        self.seconds = {}                                      # wait / copy, filled by result()

    def result(self, check=True):
        """Wait for this batch, download its bytes in one copy on the encoder's side stream and cut them into
        rows. A row with a non-zero status raises ``ValueError`` naming the row (``check=False``: gives ``None``
        in its place)."""
        import time
        if self._streams is None:
            t0 = time.perf_counter()
            self._event.synchronize()
            t1 = time.perf_counter()
            rows = self._rows
            table = self._table.tolist()
            offsets, sizes, status = table[:rows + 1], table[rows + 1:2*rows + 1], table[2*rows + 1:]
            total = offsets[rows]
            data = b''
            if total:
                enc = self._encoder
                host = enc._pin('bytes', total)
                with torch.cuda.stream(enc._side):
                    host[:total].copy_(self._out[:total], non_blocking=True)
                enc._side.synchronize()
                data = host[:total].numpy().tobytes()
            self._streams = [None if status[r] else data[offsets[r]:offsets[r] + sizes[r]] for r in range(rows)]
            self._status = status
            self._out = self._table_dev = self._keep = None    # the device buffers are free again
            self.seconds = dict(wait=t1 - t0, copy=time.perf_counter() - t1)
        if check:
            for r, st in enumerate(self._status):
                if st:
                    raise ValueError(f'row {r} was not encoded: {status_message(st)} (status {st})')
        return self._streams

    @property
    def status(self):
        self.result(check=False)
        return list(self._status)


class FlacBatchEncoder:
    """Encodes batches on ``device``. It owns the pinned staging of the downloads; the scratch and the output buffer
    of a batch belong to that batch until its ``result()`` was taken, so several batches may be in flight."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError(f'the GPU FLAC encoder runs on a ROCm device only; got {self.device} '
                               '(brv_flac_encode16 is the host encoder)')
        lib()
        self._pinned = {}
        self._side = torch.cuda.Stream(device=self.device)

    def _pin(self, key, nbytes):
        buf = self._pinned.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
            self._pinned[key] = buf
        return buf

    def submit(self, x, lengths=None, fs=16000, bits_per_sample=16, block_size=4096, lpc_order=8, pcm=False,
               events=None):
        """Queue the encode of ``x`` on the current stream; nothing here waits for the device. ``x``: ``(B, C, L)``
        or ``(B, L)`` on the device, float32 (quantised as ``clip(rint(x 2^(bits-1)), -2^(bits-1), 2^(bits-1) - 1)``)
        or, with ``pcm=True``, int32 already in that range. ``lengths``: per row, a sequence or a tensor; ``None``
        for ``L`` everywhere. ``events``: a list that gets a pair of ``torch.cuda.Event`` around the kernels
        (tools/flac_enc_bench.py)."""
        if x.device != self.device and not (x.is_cuda and self.device.index is None):
            raise ValueError(f'x is on {x.device}, the encoder on {self.device}')
        if x.dim() == 2:
            x = x.unsqueeze(1)
        if x.dim() != 3:
            raise ValueError(f'x is (B, C, L) or (B, L), got {tuple(x.shape)}')
        want = torch.int32 if pcm else torch.float32
        if x.dtype != want:
            raise ValueError(f'x must be {want} with pcm={pcm}, got {x.dtype}')
        x = x.contiguous()
        rows, channels, max_len = x.shape
        if lengths is None:
            lengths = torch.full((rows,), max_len, dtype=torch.int64, device=x.device)
        elif isinstance(lengths, torch.Tensor):
            lengths = lengths.to(device=x.device, dtype=torch.int64).contiguous()
        else:
            lengths = torch.tensor([int(n) for n in lengths], dtype=torch.int64).to(x.device, non_blocking=True)
        if lengths.shape != (rows,):
            raise ValueError(f'lengths has shape {tuple(lengths.shape)}, the batch {rows} rows')
        extents = (rows, channels, max_len, int(bits_per_sample), int(block_size))
        scratch_elems = query('brv_flacenc_scratch_elems', *extents)
        capacity = query('brv_flacenc_out_capacity', *extents)
        scratch = torch.empty(scratch_elems, dtype=torch.int32, device=x.device)
        out = torch.empty(capacity, dtype=torch.uint8, device=x.device)
        table = torch.empty(3*rows + 1, dtype=torch.int64, device=x.device)
        if events is not None:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()
        call('brv_flacenc_encode', x, 1 if pcm else 0, lengths, rows, channels, max_len, int(fs), int(bits_per_sample),
             int(block_size), int(lpc_order), scratch, scratch_elems, out, capacity, table, hip.stream())
        if events is not None:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()
        host = torch.empty(3*rows + 1, dtype=torch.int64).pin_memory()
        host.copy_(table, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return PendingStreams(self, out, table, host, event, rows, (x, lengths, scratch))

    def encode(self, x, lengths=None, fs=16000, bits_per_sample=16, block_size=4096, lpc_order=8, pcm=False):
        """``submit(...).result()``: the streams of the batch as ``list[bytes]``; a row with a non-zero status raises
        ``ValueError`` naming the row."""
        return self.submit(x, lengths, fs, bits_per_sample, block_size, lpc_order, pcm).result()
