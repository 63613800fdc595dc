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

A :class:`DCCRNStreamer` does the same for :class:`~brever_amd.models.DCCRN` (C ABI ``brv_dccrn_stream_*``,
``csrc/dccrn_stream.hip``) at the model's own latency: its output lags the input by
``lag = model.latency - hop`` samples, and the concatenated output minus the first ``lag`` samples is
``enhance`` of the model in eval mode.
"""
import ctypes

import torch

from . import hip


class _StreamSlots:
    """Slot bookkeeping shared by the streamers: ``max_streams`` slots of ``state_bytes`` in one HBM buffer."""

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

    def _mono(self, x, n):
        hip.require_device(x)
        if x.dim() == 3:
            x = x.mean(axis=-2)          # channels averaged, as enhance does
        if x.dim() != 2 or x.shape[0] != n:
            raise ValueError(f'input must be (n, samples) or (n, channels, samples) with n = {n} streams, '
                             f'got {tuple(x.shape)}')
        return x.float().contiguous()


class ConvTasNetStreamer(_StreamSlots):
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
        self.lag = self.hop               # the output lags the input by one hop
        self.sources = model.output_sources
        self.state_bytes = int(hip.query('brv_ctn_stream_state_bytes', model._cfg_ptr()))
        self._state = torch.zeros(self.max_streams*self.state_bytes, dtype=torch.uint8,
                                  device=model.flat_params().device)
        self._open = [False]*self.max_streams
        self._ws = None
        self._ids_cache = None

    def _reset(self, ids):
        t = self._ids_tensor(ids)
        hip.call('brv_ctn_stream_reset', self.model._cfg_ptr(), self._state, t, len(ids), hip.stream())

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
        cfg = model._cfg_ptr()
        nbytes = hip.query('brv_ctn_stream_workspace_bytes', cfg, n, hops, int(self.use_amp))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        y = torch.empty(n, self.sources, L, dtype=torch.float32, device=self.device)
        t = self._ids_tensor(ids)
        hip.call('brv_ctn_stream_step', cfg, flat, self._state, t, n, x, hops, y, int(self.use_amp), self._ws,
                 self._ws.numel(), None, hip.stream())
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
        hip.call('brv_ctn_stream_tail', self.model._cfg_ptr(), self._state, t, n, tail, hip.stream())
        out.append(tail[..., :r] if r else tail)
        return torch.cat(out, dim=-1)


class DCCRNStreamer(_StreamSlots):
    """Many concurrent streams of one :class:`~brever_amd.models.DCCRN` on its device, at the model's own
    latency: the output lags the input by ``lag = model.latency - hop`` samples (the first ``lag`` are
    zeros). Batch norms always use their running statistics (the model in eval mode, whatever
    ``model.training`` says); the flat parameters and the running buffers are read where they live at
    every call.

    ``use_amp=False``: fp32 products (the precision of ``enhance(x, use_amp=False)``);
    ``use_amp=True``: bf16 operands with fp32 accumulation, activations and state."""

    def __init__(self, model, max_streams=64, use_amp=False):
        self.lag = self.lag_for(model)           # (validates the model)
        if int(max_streams) < 1:
            raise ValueError(f'max_streams must be >= 1, got {max_streams}')
        try:
            nbytes = hip.query('brv_dccrn_stream_state_bytes', ctypes.byref(self._geometry(model)))
        except RuntimeError:
            raise ValueError(f'this DCCRN cannot stream: {hip.lib().brv_last_error().decode()}') from None
        hip.require_device(model.flat_params())
        self.model = model
        self.use_amp = bool(use_amp)
        self.max_streams = int(max_streams)
        self.hop = model.stft.hop_length
        self.state_bytes = int(nbytes)
        self._state = torch.zeros(self.max_streams*self.state_bytes, dtype=torch.uint8,
                                  device=model.flat_params().device)
        self._open = [False]*self.max_streams
        self._hops = [0]*self.max_streams          # hops received per slot
        self._ended = [False]*self.max_streams     # flushed: reset or close before the next process
        self._ws = None
        self._ids_cache = None
        self._offsets = None

    # ---- configuration --------------------------------------------------------------------------
    @staticmethod
    def lag_for(model):
        """Output lag of a DCCRN stream in samples (``model.latency - hop``); ``ValueError`` for a model
        the streaming kernels do not take."""
        from .models.dccrn import DCCRN
        if not isinstance(model, DCCRN):
            raise ValueError(f'streaming needs a DCCRN, got {type(model).__name__}')
        (kf, kt), (sf, st), (pf, pt), (opf, opt) = model.mask_net.geom
        if st != 1 or pt != 0 or opt != 0:
            raise ValueError('DCCRN streaming needs time stride 1, time padding 0 and time output padding 0 '
                             f'(got stride {st}, padding {pt}, output padding {opt})')
        stft = model.stft
        if stft.n_fft != stft.frame_length:
            raise ValueError(f'DCCRN streaming needs n_fft == frame_length, got {stft.n_fft} and {stft.frame_length}')
        if stft.frame_length % (2*stft.hop_length):
            raise ValueError('DCCRN streaming needs frame_length to be a multiple of 2 hop (the centre padding '
                             f'in whole hops), got {stft.frame_length} and hop {stft.hop_length}')
        if not (stft.center and stft.pad_mode == 'constant' and stft.normalized and stft.onesided
                and stft.compression_factor == 1 and stft.scale_factor == 1):
            raise ValueError('DCCRN streaming needs the STFT settings DCCRN builds')
        net = model.mask_net
        for blk in list(net.encoder) + list(net.decoder):
            if blk.norm is not None and (not getattr(blk.norm, 'track_running_stats', True)
                                         or getattr(blk.norm, 'running_mean', None) is None):
                raise ValueError('DCCRN streaming needs batch norms that track running statistics')
        if model.flat_params() is None:
            raise ValueError('DCCRN streaming reads the flat parameter buffer; this model keeps separate '
                             'parameters (optimizer other than Adam)')
        return model.latency - stft.hop_length

    @staticmethod
    def _geometry(model):
        """``brv_dccrn_stream_config`` with the geometry only (offsets and buffer addresses unset)."""
        from .models.dccrn import ComplexBatchNorm2d
        net = model.mask_net
        (kf, kt), (sf, st), (pf, pt), (opf, opt) = net.geom
        cfg = hip.DccrnStreamConfig()
        cfg.n_fft, cfg.hop, cfg.levels = model.stft.n_fft, model.stft.hop_length, len(net.encoder)
        cfg.kf, cfg.kt, cfg.sf, cfg.pf, cfg.opf, cfg.st, cfg.pt, cfg.opt = kf, kt, sf, pf, opf, st, pt, opt
        cfg.complex_bn = int(isinstance(net.encoder[0].norm, ComplexBatchNorm2d))
        if len(net.encoder) > hip.DCCRN_STREAM_MAX_LEVELS:
            cfg.levels = hip.DCCRN_STREAM_MAX_LEVELS + 1       # (refused by the library, with its message)
        for i, blk in enumerate(list(net.encoder)[:hip.DCCRN_STREAM_MAX_LEVELS]):
            cfg.channels[i] = blk.conv.module_real.out_channels
        lstm = net.lstm.lstm.layers
        cfg.lstm_hidden, cfg.lstm_layers = lstm[0].module_real.hidden_size, len(lstm)
        return cfg

    def _config(self):
        """The full config of one call: geometry, flat offsets, eps and the running buffers' current addresses."""
        model = self.model
        net = model.mask_net
        flat = model.flat_params()
        key = (flat.data_ptr(), flat.numel())
        if self._offsets is None or self._offsets[0] != key:
            self._offsets = (key, {id(p): off for p, off in model.param_offsets()})
        offs = self._offsets[1]
        cfg = self._geometry(model)

        def off(p):
            return offs[id(p)] if p is not None else -1
        blocks = list(net.encoder) + list(net.decoder)
        for b, blk in enumerate(blocks):
            mr, mi = blk.conv.module_real, blk.conv.module_imag
            norm, act = blk.norm, blk.activation
            cfg.off_block[b][:] = [off(mr.weight), off(mr.bias), off(mi.weight), off(mi.bias),
                                   off(norm.weight) if norm is not None else -1,
                                   off(norm.bias) if norm is not None else -1,
                                   off(act.weight) if act is not None else -1]
            if norm is not None:
                hip.require_device(norm.running_mean, norm.running_var)
                cfg.eps[b] = float(norm.eps)
                cfg.run_mean[b] = norm.running_mean.data_ptr()
                cfg.run_var[b] = norm.running_var.data_ptr()
        for li, layer in enumerate(net.lstm.lstm.layers):
            for m, mod in enumerate((layer.module_real, layer.module_imag)):
                cfg.off_lstm[li][m][:] = [off(mod.weight_ih_l0), off(mod.weight_hh_l0), off(mod.bias_ih_l0),
                                          off(mod.bias_hh_l0)]
        lr, li_ = net.lstm.linear_r, net.lstm.linear_i
        cfg.off_linear[:] = [off(lr.weight), off(lr.bias), off(li_.weight), off(li_.bias)]
        for b, blk in enumerate(blocks):
            norm = blk.norm
            if norm is not None and (not norm.running_mean.is_contiguous() or not norm.running_var.is_contiguous()
                                     or norm.running_mean.dtype != torch.float32):
                raise RuntimeError('the running buffers must be contiguous fp32 tensors')
        return cfg

    def _reset(self, ids):
        t = self._ids_tensor(ids)
        cfg = self._geometry(self.model)
        hip.call('brv_dccrn_stream_reset', ctypes.byref(cfg), self._state, t, len(ids), hip.stream())
        for i in ids:
            self._hops[i] = 0
            self._ended[i] = False

    def _call(self, ids, n, hops):
        """What every launch of a call needs: params, tables, config, workspace."""
        model = self.model
        flat = model.flat_params()
        hip.require_device(flat)
        if flat.device != self.device:
            raise RuntimeError(f'the model moved to {flat.device}; the streams live on {self.device}')
        cfg = self._config()
        nbytes = hip.query('brv_dccrn_stream_workspace_bytes', ctypes.byref(cfg), n, hops, int(self.use_amp))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        tb = model.stft._tables(self.device)
        return cfg, flat, tb

    # ---- compute --------------------------------------------------------------------------------
    def process(self, x, ids):
        """Advance the streams ``ids`` by the chunk ``x`` (``(n, k hop)`` or ``(n, channels, k hop)``):
        returns ``(n, k hop)``, ``lag`` samples behind the input."""
        ids = self._check_ids(ids)
        n = len(ids)
        x = self._mono(x, n)
        L = x.shape[1]
        if L == 0 or L % self.hop:
            raise ValueError(f'a chunk must be a positive multiple of hop = {self.hop} samples, got {L}')
        for i in ids:
            if self._ended[i]:
                raise ValueError(f'stream {i} was flushed; reset or close it first')
        hops = L//self.hop
        cfg, flat, tb = self._call(ids, n, hops)
        y = torch.empty(n, L, dtype=torch.float32, device=self.device)
        t = self._ids_tensor(ids)
        hip.call('brv_dccrn_stream_step', ctypes.byref(cfg), flat, tb['window'], tb['basis'], tb['synthesis'],
                 self._state, t, n, x, hops, y, int(self.use_amp), self._ws, self._ws.numel(), None, hip.stream())
        for i in ids:
            self._hops[i] += hops
        return y

    def flush(self, ids, rest=None):
        """End the streams ``ids``: ``rest`` is their last ``r < hop`` input samples (``(n, r)`` or
        ``(n, channels, r)``, or None). Runs the frames of the zero-padded end and returns the ``(n, lag + r)``
        output samples still owed. Reset or close the streams afterwards."""
        ids = self._check_ids(ids)
        n = len(ids)
        r = 0
        if rest is not None:
            rest = self._mono(rest, n)
            r = rest.shape[1]
            if r >= self.hop:
                raise ValueError(f'rest must be shorter than hop = {self.hop} samples, got {r}; '
                                 'process the whole hops first')
        stft = self.model.stft
        (_, kt), _, _, _ = self.model.mask_net.geom
        need = 1 + len(self.model.mask_net.encoder)*(kt - 1)     # STFT frames the offline model needs
        for i in ids:
            if self._ended[i]:
                raise ValueError(f'stream {i} was flushed already; reset or close it first')
            length = self._hops[i]*self.hop + r
            frames = stft.frame_count(length) + stft.n_fft//self.hop
            if frames < need:
                raise ValueError(f'stream {i} has {length} samples: DCCRN needs at least {need} STFT frames '
                                 f'({frames} here)')
        hops = self.lag//self.hop + (1 if r else 0)
        cfg, flat, tb = self._call(ids, n, hops)
        y = torch.empty(n, self.lag + r, dtype=torch.float32, device=self.device)
        t = self._ids_tensor(ids)
        hip.call('brv_dccrn_stream_tail', ctypes.byref(cfg), flat, tb['window'], tb['basis'], tb['synthesis'],
                 self._state, t, n, rest if r else None, r, y, int(self.use_amp), self._ws, self._ws.numel(), None,
                 hip.stream())
        for i in ids:
            self._ended[i] = True
        return y


def enhance_streaming(model, x, chunk_samples, use_amp=False):
    """``model.enhance(x, use_amp)`` computed chunk by chunk through a :class:`ConvTasNetStreamer` or, for a
    DCCRN, a :class:`DCCRNStreamer` (same shapes as ``model.enhance``). ``chunk_samples`` is rounded down to
    whole hops (at least one)."""
    if x.ndim == 2:
        return enhance_streaming(model, x.unsqueeze(0), chunk_samples, use_amp).squeeze(0)
    if x.ndim != 3:
        raise ValueError(f'input must be 2 or 3 dimensional, got {x.ndim}')
    B, L = x.shape[0], x.shape[-1]
    from .models.dccrn import DCCRN
    cls = DCCRNStreamer if isinstance(model, DCCRN) else ConvTasNetStreamer
    s = cls(model, max_streams=B, use_amp=use_amp)
    hip.require_device(x)
    hop = s.hop
    chunk = max(1, int(chunk_samples)//hop)*hop
    mono = x.float().mean(axis=-2)
    ids = s.open(B)
    whole = L//hop*hop
    outs = [s.process(mono[:, i:i + chunk], ids) if i + chunk <= whole else
            s.process(mono[:, i:whole], ids) for i in range(0, whole, chunk)]
    outs.append(s.flush(ids, mono[:, whole:] if L > whole else None))
    return torch.cat(outs, dim=-1)[..., s.lag:]
