"""Stateful streaming inference of the causal Conv-TasNet (C ABI ``brv_ctn_stream_*``,
``csrc/ctn_stream.hip``).

A :class:`ConvTasNetStreamer` keeps up to ``max_streams`` concurrent streams in one HBM state buffer;
each :meth:`~ConvTasNetStreamer.process` call advances any subset of them by a chunk of whole hops
(``hop = filter_length // 2`` samples). A stream's output lags its input by exactly one hop: the first
hop it returns is zeros. Concatenating every chunk's output and the :meth:`~ConvTasNetStreamer.flush`
of the last partial hop, then dropping the first hop, gives ``model.enhance`` of the whole signal (up to
the summation order of the layer-norm statistics).

The kernels read the model's flat fp32 parameters at every step, as the offline fp32 path does, so an
optimizer step, ``load_state_dict`` or ``mark_params_changed`` takes effect at the next ``process``.
Streams that are already open keep the state they computed with the old parameters.
"""
import ctypes

import torch

from . import hip


class ConvTasNetStreamer:
    """Many concurrent streams of one causal :class:`~brever_amd.models.ConvTasNet` on its device.

    ``use_amp=False``: fp32 products (the precision of ``enhance(x, use_amp=False)``);
    ``use_amp=True``: bf16 operands with fp32 accumulation and state."""

    def __init__(self, model, max_streams=64, use_amp=False):
        from .models.convtasnet import ConvTasNet
        if not isinstance(model, ConvTasNet):
            raise ValueError(f'streaming needs a ConvTasNet, got {type(model).__name__}')
        if not model.cfg.causal:
            raise ValueError('streaming needs a causal ConvTasNet: the global layer norm of the '
                             'non-causal model needs the whole signal')
        if model.cfg.filter_length % 2:
            raise ValueError('streaming needs an even filter_length (hop = filter_length // 2)')
        if int(max_streams) < 1:
            raise ValueError(f'max_streams must be >= 1, got {max_streams}')
        hip.require_device(model.flat_params())
        self.model = model
        self.use_amp = bool(use_amp)
        self.max_streams = int(max_streams)
        self.hop = model.cfg.filter_length//2
        self.sources = model.output_sources
        nbytes = hip.lib().brv_ctn_stream_state_bytes(model._cfg_ptr())
        if nbytes < 0:
            hip.check(int(nbytes), 'brv_ctn_stream_state_bytes')
        self.state_bytes = int(nbytes)
        self._state = torch.zeros(self.max_streams*self.state_bytes, dtype=torch.uint8,
                                  device=model.flat_params().device)
        self._open = [False]*self.max_streams
        self._ws = None
        self._ids_cache = None

    @property
    def device(self):
        return self._state.device

    # ---- slots ----------------------------------------------------------------------------------
    def open(self, n=1):
        """Open ``n`` new streams; returns their slot ids (lowest free slots first)."""
        free = [i for i, used in enumerate(self._open) if not used]
        if n < 1 or n > len(free):
            raise RuntimeError(f'cannot open {n} streams: {len(free)} of {self.max_streams} slots are free')
        ids = free[:n]
        self._reset(ids)
        for i in ids:
            self._open[i] = True
        return ids

    def close(self, ids):
        """Free the slots ``ids``; a later ``open`` may hand them out again."""
        for i in self._check_ids(ids):
            self._open[i] = False

    def reset(self, ids):
        """Restart the open streams ``ids`` at sample 0."""
        self._reset(self._check_ids(ids))

    def _check_ids(self, ids):
        if isinstance(ids, torch.Tensor):
            ids = ids.tolist()
        elif isinstance(ids, int):
            ids = [ids]
        ids = [int(i) for i in ids]
        if not ids:
            raise ValueError('no stream ids given')
        for i in ids:
            if not 0 <= i < self.max_streams or not self._open[i]:
                raise ValueError(f'stream id {i} is not open')
        if len(set(ids)) != len(ids):
            raise ValueError(f'stream ids must be distinct, got {ids}')
        return ids

    def _ids_tensor(self, ids):
        # the id list of the last call stays on the device: a server steps the same set chunk after chunk
        key = tuple(ids)
        if self._ids_cache is None or self._ids_cache[0] != key:
            self._ids_cache = (key, torch.tensor(ids, dtype=torch.int32).to(self.device))
        return self._ids_cache[1]

    def _reset(self, ids):
        t = self._ids_tensor(ids)
        hip.check(hip.lib().brv_ctn_stream_reset(self.model._cfg_ptr(), hip.ptr(self._state), hip.ptr(t),
                                                 len(ids), hip.stream()), 'brv_ctn_stream_reset')

    def _mono(self, x, n):
        hip.require_device(x)
        if x.dim() == 3:
            x = x.mean(axis=-2)          # channels averaged, as enhance does
        if x.dim() != 2 or x.shape[0] != n:
            raise ValueError(f'input must be (n, samples) or (n, channels, samples) with n = {n} streams, '
                             f'got {tuple(x.shape)}')
        return x.float().contiguous()

    # ---- compute --------------------------------------------------------------------------------
    def process(self, x, ids):
        """Advance the streams ``ids`` by the chunk ``x`` (``(n, k hop)`` or ``(n, channels, k hop)``):
        returns ``(n, sources, k hop)``, one hop behind the input."""
        ids = self._check_ids(ids)
        n = len(ids)
        x = self._mono(x, n)
        L = x.shape[1]
        if L == 0 or L % self.hop:
            raise ValueError(f'a chunk must be a positive multiple of hop = {self.hop} samples, got {L}')
        hops = L//self.hop
        model = self.model
        model._check_layout()
        flat = model.flat_params()
        hip.require_device(flat)
        if flat.device != self.device:
            raise RuntimeError(f'the model moved to {flat.device}; the streams live on {self.device}')
        lib = hip.lib()
        cfg = model._cfg_ptr()
        nbytes = lib.brv_ctn_stream_workspace_bytes(cfg, n, hops, int(self.use_amp))
        if nbytes < 0:
            hip.check(int(nbytes), 'brv_ctn_stream_workspace_bytes')
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        y = torch.empty(n, self.sources, L, dtype=torch.float32, device=self.device)
        t = self._ids_tensor(ids)
        hip.check(lib.brv_ctn_stream_step(
            cfg, hip.ptr(flat), hip.ptr(self._state), hip.ptr(t), n, hip.ptr(x), hops, hip.ptr(y),
            int(self.use_amp), hip.ptr(self._ws), self._ws.numel(), None, hip.stream()), 'brv_ctn_stream_step')
        return y

    def flush(self, ids, rest=None):
        """End the streams ``ids``: ``rest`` is their last ``r < hop`` input samples (``(n, r)`` or
        ``(n, channels, r)``, or None), zero-padded to a frame as the offline encoder pads. Returns the
        ``(n, sources, hop + r)`` output samples still owed. Reset or close the streams afterwards."""
        ids = self._check_ids(ids)
        n = len(ids)
        out = []
        r = 0
        if rest is not None:
            rest = self._mono(rest, n)
            r = rest.shape[1]
            if r >= self.hop:
                raise ValueError(f'rest must be shorter than hop = {self.hop} samples, got {r}; '
                                 'process the whole hops first')
        if r:
            x = torch.zeros(n, self.hop, dtype=torch.float32, device=self.device)
            x[:, :r] = rest
            out.append(self.process(x, ids))
        tail = torch.empty(n, self.sources, self.hop, dtype=torch.float32, device=self.device)
        t = self._ids_tensor(ids)
        hip.check(hip.lib().brv_ctn_stream_tail(self.model._cfg_ptr(), hip.ptr(self._state), hip.ptr(t), n,
                                                hip.ptr(tail), hip.stream()), 'brv_ctn_stream_tail')
        out.append(tail[..., :r] if r else tail)
        return torch.cat(out, dim=-1)


def enhance_streaming(model, x, chunk_samples, use_amp=False):
    """``model.enhance(x, use_amp)`` computed chunk by chunk through a :class:`ConvTasNetStreamer`
    (same shapes: ``(channels, L)`` -> ``(S, L)``, ``(B, channels, L)`` -> ``(B, S, L)``).
    ``chunk_samples`` is rounded down to whole hops (at least one)."""
    if x.ndim == 2:
        return enhance_streaming(model, x.unsqueeze(0), chunk_samples, use_amp).squeeze(0)
    if x.ndim != 3:
        raise ValueError(f'input must be 2 or 3 dimensional, got {x.ndim}')
    B, L = x.shape[0], x.shape[-1]
    s = ConvTasNetStreamer(model, max_streams=B, use_amp=use_amp)
    hip.require_device(x)
    hop = s.hop
    chunk = max(1, int(chunk_samples)//hop)*hop
    mono = x.float().mean(axis=-2)
    ids = s.open(B)
    whole = L//hop*hop
    outs = [s.process(mono[:, i:i + chunk], ids) if i + chunk <= whole else
            s.process(mono[:, i:whole], ids) for i in range(0, whole, chunk)]
    outs.append(s.flush(ids, mono[:, whole:] if L > whole else None))
    return torch.cat(outs, dim=-1)[..., hop:]
