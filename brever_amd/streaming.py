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
    """What the streamers share: ``max_streams`` slots of ``state_bytes`` in one HBM buffer, the grow-only workspace,
    the checks of a chunk, a rest and the model's device and, for a streamer that asks for it, how many hops each
    slot received and whether it was flushed. A streamer gives ``_launch_reset(t, n)``."""

    def __init__(self, max_streams):
        if int(max_streams) < 1:
            raise ValueError(f'max_streams must be >= 1, got {max_streams}')
        self.max_streams = int(max_streams)

    def _allocate(self, state_bytes, device, track_end=False):
        self.state_bytes = int(state_bytes)
        self._state = torch.zeros(self.max_streams*self.state_bytes, dtype=torch.uint8, device=device)
        self._open = [False]*self.max_streams
        self._hops = [0]*self.max_streams if track_end else None        # hops received per slot
        self._ended = [False]*self.max_streams if track_end else None   # flushed: reset or close it next
        self._ws = self._ids_cache = None

    @property
    def device(self):
        return self._state.device

    def _reset(self, ids):
        self._launch_reset(self._ids_tensor(ids), len(ids))
        if self._ended is not None:
            for i in ids:
                self._hops[i] = 0
                self._ended[i] = False

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    def _whole_hops(self, L):
        if L == 0 or L % self.hop:
            raise ValueError(f'a chunk must be a positive multiple of hop = {self.hop} samples, got {L}')
        return L//self.hop

    def _rest(self, rest, n):
        """``(rest, r)`` of a flush: the last ``r < hop`` samples as ``_input`` shapes them, or ``(None, 0)``."""
        if rest is None:
            return None, 0
        rest = self._input(rest, n, 'rest')
        if rest.shape[-1] >= self.hop:
            raise ValueError(f'rest must be shorter than hop = {self.hop} samples, got {rest.shape[-1]}; '
                             'process the whole hops first')
        return rest, rest.shape[-1]

    def _check_device(self, t):
        hip.require_device(t)
        if t.device != self.device:
            raise RuntimeError(f'the model moved to {t.device}; the streams live on {self.device}')

    def _check_live(self, ids, already=''):
        for i in ids:
            if self._ended[i]:
                raise ValueError(f'stream {i} was flushed{already}; reset or close it first')

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

    def _input(self, x, n, what='input'):
        """The mono (n, samples) fp32 input of a call (the FFNN streamer keeps the channels instead)."""
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
        super().__init__(max_streams)
        hip.require_device(model.flat_params())
        self.model = model
        self.use_amp = bool(use_amp)
        self.hop = model.cfg.filter_length//2
        self.lag = self.hop               # the output lags the input by one hop
        self.sources = model.output_sources
        self._allocate(hip.query('brv_ctn_stream_state_bytes', model._cfg_ptr()), model.flat_params().device)

    def _launch_reset(self, t, n):
        hip.call('brv_ctn_stream_reset', self.model._cfg_ptr(), self._state, t, n, hip.stream())

    # ---- compute --------------------------------------------------------------------------------
    def process(self, x, ids):
        """Advance the streams ``ids`` by the chunk ``x`` (``(n, k hop)`` or ``(n, channels, k hop)``):
        returns ``(n, sources, k hop)``, one hop behind the input."""
        ids = self._check_ids(ids)
        n = len(ids)
        x = self._input(x, n)
        L = x.shape[1]
        hops = self._whole_hops(L)
        model = self.model
        model._check_layout()
        flat = model.flat_params()
        self._check_device(flat)
        cfg = model._cfg_ptr()
        ws = self._workspace(hip.query('brv_ctn_stream_workspace_bytes', cfg, n, hops, int(self.use_amp)))
        y = torch.empty(n, self.sources, L, dtype=torch.float32, device=self.device)
        t = self._ids_tensor(ids)
        hip.call('brv_ctn_stream_step', cfg, flat, self._state, t, n, x, hops, y, int(self.use_amp), ws, ws.numel(),
                 None, hip.stream())
        return y

    def flush(self, ids, rest=None):
        """End the streams ``ids``: ``rest`` is their last ``r < hop`` input samples (``(n, r)`` or
        ``(n, channels, r)``, or None), zero-padded to a frame as the offline encoder pads. Returns the
        ``(n, sources, hop + r)`` output samples still owed. Reset or close the streams afterwards."""
        ids = self._check_ids(ids)
        n = len(ids)
        out = []
        rest, r = self._rest(rest, n)
        if r:
            x = torch.zeros(n, self.hop, dtype=torch.float32, device=self.device)
            x[:, :r] = rest
            out.append(self.process(x, ids))
        tail = torch.empty(n, self.sources, self.hop, dtype=torch.float32, device=self.device)
        t = self._ids_tensor(ids)
        hip.call('brv_ctn_stream_tail', self.model._cfg_ptr(), self._state, t, n, tail, hip.stream())
        out.append(tail[..., :r] if r else tail)
        return torch.cat(out, dim=-1)


def _check_stft(stft, name):
    """The STFT settings the DCCRN and FFNN streaming kernels take; ``ValueError`` in the streamer's own words."""
    if stft.frame_length % (2*stft.hop_length):
        raise ValueError(f'{name} streaming needs frame_length to be a multiple of 2 hop (the centre padding '
                         f'in whole hops), got {stft.frame_length} and hop {stft.hop_length}')
    if not (stft.n_fft == stft.frame_length and stft.center and stft.pad_mode == 'constant' and stft.normalized
            and stft.onesided and stft.compression_factor == 1 and stft.scale_factor == 1):
        raise ValueError(f'{name} streaming needs the STFT settings {name} builds')


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
        super().__init__(max_streams)
        try:
            nbytes = hip.query('brv_dccrn_stream_state_bytes', ctypes.byref(self._geometry(model)))
        except RuntimeError:
            raise ValueError(f'this DCCRN cannot stream: {hip.last_error()}') from None
        hip.require_device(model.flat_params())
        self.model = model
        self.use_amp = bool(use_amp)
        self.hop = model.stft.hop_length
        self._allocate(nbytes, model.flat_params().device, track_end=True)
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
        _check_stft(stft, 'DCCRN')
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

    def _launch_reset(self, t, n):
        cfg = self._geometry(self.model)
        hip.call('brv_dccrn_stream_reset', ctypes.byref(cfg), self._state, t, n, hip.stream())

    def _call(self, ids, n, hops):
        """What every launch of a call needs: config, params, tables, the ids on the device (and the workspace)."""
        model = self.model
        flat = model.flat_params()
        self._check_device(flat)
        cfg = self._config()
        self._workspace(hip.query('brv_dccrn_stream_workspace_bytes', ctypes.byref(cfg), n, hops, int(self.use_amp)))
        tb = model.stft._tables(self.device)
        return cfg, flat, tb, self._ids_tensor(ids)

    # ---- compute --------------------------------------------------------------------------------
    def process(self, x, ids):
        """Advance the streams ``ids`` by the chunk ``x`` (``(n, k hop)`` or ``(n, channels, k hop)``):
        returns ``(n, k hop)``, ``lag`` samples behind the input."""
        ids = self._check_ids(ids)
        n = len(ids)
        x = self._input(x, n)
        L = x.shape[1]
        hops = self._whole_hops(L)
        self._check_live(ids)
        cfg, flat, tb, t = self._call(ids, n, hops)
        y = torch.empty(n, L, dtype=torch.float32, device=self.device)
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
        rest, r = self._rest(rest, n)
        stft = self.model.stft
        (_, kt), _, _, _ = self.model.mask_net.geom
        need = 1 + len(self.model.mask_net.encoder)*(kt - 1)     # STFT frames the offline model needs
        for i in ids:
            self._check_live([i], ' already')
            length = self._hops[i]*self.hop + r
            frames = stft.frame_count(length) + stft.n_fft//self.hop
            if frames < need:
                raise ValueError(f'stream {i} has {length} samples: DCCRN needs at least {need} STFT frames '
                                 f'({frames} here)')
        hops = self.lag//self.hop + (1 if r else 0)
        cfg, flat, tb, t = self._call(ids, n, hops)
        y = torch.empty(n, self.lag + r, dtype=torch.float32, device=self.device)
        hip.call('brv_dccrn_stream_tail', ctypes.byref(cfg), flat, tb['window'], tb['basis'], tb['synthesis'],
                 self._state, t, n, rest if r else None, r, y, int(self.use_amp), self._ws, self._ws.numel(), None,
                 hip.stream())
        for i in ids:
            self._ended[i] = True
        return y


class FFNNStreamer(_StreamSlots):
    """Many concurrent streams of one :class:`~brever_amd.models.FFNN` on its device, at the model's own latency:
    the output lags the input by ``lag = frame_length - hop_length`` samples (the first ``lag`` are zeros), the
    look-ahead of the centred STFT. A stream keeps all its ``channels``: the features are the channel mean of
    the power, the mask is applied to the channel-mean spectrum. Dropout is never applied (the model in eval
    mode, whatever ``model.training`` says). Weights, biases and the static normaliser's ``mean`` / ``std`` are
    read where they live at every call. fp32 only, as the offline model."""

    def __init__(self, model, max_streams=64, channels=2):
        from . import ffnn_stream as ffs
        self.lag = self.lag_for(model)           # (validates the model)
        super().__init__(max_streams)
        if int(channels) < 1:
            raise ValueError(f'channels must be >= 1, got {channels}')
        self._ffs = ffs
        self.model = model
        self.channels = int(channels)
        try:
            nbytes = ffs.query('brv_ffs_state_bytes', ctypes.byref(self._geometry(model, self.channels)))
        except RuntimeError:
            raise ValueError(f'this FFNN cannot stream: {ffs.last_error()}') from None
        hip.require_device(next(model.parameters()))
        self.hop = model.stft.hop_length
        self._allocate(nbytes, next(model.parameters()).device, track_end=True)
        self._mel = None
        self._bufs = {}

    # ---- configuration --------------------------------------------------------------------------
    @staticmethod
    def lag_for(model):
        """Output lag of an FFNN stream in samples (``frame_length - hop_length``); ``ValueError`` naming the
        cause for a model the streaming kernels do not take."""
        from .models.ffnn import FFNN
        from .modules.features import FeatureExtractor
        if not isinstance(model, FFNN):
            raise ValueError(f'streaming needs an FFNN, got {type(model).__name__}')
        family = FeatureExtractor._fbe_family
        for f in model.feature_extractor.features:
            if f in ('ild', 'ipd', 'ic'):
                raise ValueError(f"FFNN streaming does not take the binaural cue feature '{f}'")
            if family[f][2]:
                raise ValueError(f"FFNN streaming does not take the DCT feature '{f}': its delta rows are "
                                 'differences along the frames')
        stft = model.stft
        _check_stft(stft, 'FFNN')
        hidden = sum(isinstance(m, torch.nn.Linear) for m in model.ffnn.module_list) - 1
        from .ffnn_stream import MAX_HIDDEN
        if hidden > MAX_HIDDEN:
            raise ValueError(f'FFNN streaming takes at most {MAX_HIDDEN} hidden layers, got {hidden}')
        return stft.frame_length - stft.hop_length

    @staticmethod
    def _linears(model):
        return [m for m in model.ffnn.module_list if isinstance(m, torch.nn.Linear)]

    @staticmethod
    def _geometry(model, channels=2):
        """``brv_ffs_config`` with the geometry only (addresses unset)."""
        from . import ffnn_stream as ffs
        from .models.ffnn import CumulativeNormalizer
        from .modules.features import FeatureExtractor, eps
        stft, fe = model.stft, model.feature_extractor
        cfg = ffs.FfsConfig()
        cfg.n_fft, cfg.frame_length, cfg.hop, cfg.channels = stft.n_fft, stft.frame_length, stft.hop_length, channels
        cfg.center, cfg.pad_constant = int(bool(stft.center)), int(stft.pad_mode == 'constant')
        cfg.normalized, cfg.onesided = int(bool(stft.normalized)), int(bool(stft.onesided))
        cfg.compression, cfg.scale = float(stft.compression_factor), float(stft.scale_factor)
        cfg.mel, cfg.stacks, cfg.features = model.mel_fb.n_filters, model.stacks, len(fe.features)
        for i, f in enumerate(fe.features[:ffs.MAX_FEATURES]):
            cfg.feat_norm[i], cfg.feat_comp[i], _ = (int(v) for v in FeatureExtractor._fbe_family[f])
        cumulative = isinstance(model.normalization, CumulativeNormalizer)
        cfg.norm = int(cumulative)
        cfg.eps_feat = float(eps)
        cfg.eps_norm = float(model.normalization.eps) if cumulative else 0.0
        linears = FFNNStreamer._linears(model)
        cfg.hidden = len(linears) - 1
        for i, lin in enumerate(linears[:ffs.MAX_HIDDEN + 1]):
            cfg.widths[i] = lin.out_features
        return cfg

    def _config(self):
        """The config of one call: geometry and the current addresses of every value the kernels read."""
        model = self.model
        cfg = self._geometry(model, self.channels)
        tensors = []
        for i, lin in enumerate(self._linears(model)):
            cfg.weight[i], cfg.bias[i] = lin.weight.data_ptr(), lin.bias.data_ptr()
            tensors += [lin.weight, lin.bias]
        if not cfg.norm:
            norm = model.normalization
            cfg.mean, cfg.std = norm.mean.data_ptr(), norm.std.data_ptr()
            tensors += [norm.mean, norm.std]
        for t in tensors:
            self._check_device(t)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError('the weights, biases and statistics must be contiguous fp32 tensors')
        if self._mel is None:
            fb = model.mel_fb
            self._mel = (fb.filters.float().to(self.device).contiguous(),
                         fb.inverse_filters.float().to(self.device).contiguous())
        cfg.mel_fwd, cfg.mel_inv = self._mel[0].data_ptr(), self._mel[1].data_ptr()
        return cfg

    def _launch_reset(self, t, n):
        cfg = self._geometry(self.model, self.channels)
        self._ffs.call('brv_ffs_reset', ctypes.byref(cfg), self._state, self.max_streams, t, n, hip.stream())

    def _input(self, x, n, what='input'):
        hip.require_device(x)
        if x.dim() == 2:
            raise ValueError(f'FFNN needs its channels: {what} must be (n, channels, samples) with '
                             f'{self.channels} channels, got {tuple(x.shape)} (the features are the channel mean of '
                             'the power, so the channels cannot be averaged first)')
        if x.dim() != 3 or x.shape[0] != n or x.shape[1] != self.channels:
            raise ValueError(f'{what} must be (n, channels, samples) with n = {n} streams and {self.channels} '
                             f'channels, got {tuple(x.shape)}')
        return x.float().contiguous()

    def _run(self, ids, n, x, hops, rest, y):
        """The launch sequence of one call: frames, DFT, network, synthesis, overlap-add + commit."""
        ffs, stft = self._ffs, self.model.stft
        cfg = self._config()
        c = ctypes.byref(cfg)
        ws = self._workspace(ffs.query('brv_ffs_workspace_bytes', c, n, hops))
        C, N, hop, bins = self.channels, stft.n_fft, self.hop, stft.bins
        if (n, hops) not in self._bufs:
            if len(self._bufs) >= 16:
                self._bufs.clear()
            f32 = dict(dtype=torch.float32, device=self.device)
            self._bufs[(n, hops)] = (torch.empty(n*C, self.lag + hops*hop, **f32),
                                     torch.empty(n*C, bins, hops, 2, **f32), torch.empty(n, bins, hops, 2, **f32),
                                     torch.empty(n, hops, N, **f32))
        xin, spec, mspec, frames = self._bufs[(n, hops)]
        tb = stft._tables(self.device)
        t, st = self._ids_tensor(ids), hip.stream()
        ffs.call('brv_ffs_step_frames', c, self._state, self.max_streams, t, n, x, hops, rest, xin, st)
        hip.call('brv_dft64_forward', xin, tb['basis'], spec, n*C, self.lag + hops*hop, N, hop, 0, hops, bins, 1.0,
                 1.0, st)
        ffs.call('brv_ffs_step_net', c, self._state, self.max_streams, t, n, hops, rest, spec, mspec, ws, ws.numel(),
                 st)
        hip.call('brv_dft64_synthesis', mspec, tb['synthesis'], frames, n, hops, N, bins, 1.0, 1.0, st)
        ffs.call('brv_ffs_step_emit', c, tb['window'], self._state, self.max_streams, t, n, hops, rest, xin, frames,
                 y, ws, ws.numel(), st)

    # ---- compute --------------------------------------------------------------------------------
    def process(self, x, ids):
        """Advance the streams ``ids`` by the chunk ``x`` (``(n, channels, k hop)``): returns ``(n, k hop)``,
        ``lag`` samples behind the input."""
        ids = self._check_ids(ids)
        n = len(ids)
        x = self._input(x, n)
        L = x.shape[-1]
        hops = self._whole_hops(L)
        self._check_live(ids)
        y = torch.empty(n, L, dtype=torch.float32, device=self.device)
        self._run(ids, n, x, hops, -1, y)
        for i in ids:
            self._hops[i] += hops
        return y

    def flush(self, ids, rest=None):
        """End the streams ``ids``: ``rest`` is their last ``r < hop`` input samples (``(n, channels, r)``, or
        None). Runs the frames of the zero-padded end and returns the ``(n, lag + r)`` output samples still
        owed. Reset or close the streams afterwards."""
        ids = self._check_ids(ids)
        n = len(ids)
        rest, r = self._rest(rest, n)
        self._check_live(ids, ' already')
        y = torch.empty(n, self.lag + r, dtype=torch.float32, device=self.device)
        self._run(ids, n, rest if r else None, self.model.stft.n_fft//self.hop, r, y)
        for i in ids:
            self._ended[i] = True
        return y


def enhance_streaming(model, x, chunk_samples, use_amp=False):
    """``model.enhance(x, use_amp)`` computed chunk by chunk through a :class:`ConvTasNetStreamer`, for a DCCRN a
    :class:`DCCRNStreamer`, for an FFNN an :class:`FFNNStreamer` (same shapes as ``model.enhance``).
    ``chunk_samples`` is rounded down to whole hops (at least one). An FFNN is fed every channel of ``x`` and, as
    its ``enhance``, has no reduced-precision mode: ``use_amp`` changes nothing for it."""
    if x.ndim == 2:
        return enhance_streaming(model, x.unsqueeze(0), chunk_samples, use_amp).squeeze(0)
    if x.ndim != 3:
        raise ValueError(f'input must be 2 or 3 dimensional, got {x.ndim}')
    B, L = x.shape[0], x.shape[-1]
    from .models.dccrn import DCCRN
    from .models.ffnn import FFNN
    if isinstance(model, FFNN):
        s = FFNNStreamer(model, max_streams=B, channels=x.shape[-2])
        hip.require_device(x)
        feed = x.float()
    else:
        cls = DCCRNStreamer if isinstance(model, DCCRN) else ConvTasNetStreamer
        s = cls(model, max_streams=B, use_amp=use_amp)
        hip.require_device(x)
        feed = x.float().mean(axis=-2)
    hop = s.hop
    chunk = max(1, int(chunk_samples)//hop)*hop
    ids = s.open(B)
    whole = L//hop*hop
    outs = [s.process(feed[..., i:i + chunk], ids) if i + chunk <= whole else
            s.process(feed[..., i:whole], ids) for i in range(0, whole, chunk)]
    outs.append(s.flush(ids, feed[..., whole:] if L > whole else None))
    return torch.cat(outs, dim=-1)[..., s.lag:]
