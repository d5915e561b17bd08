"""`HipEngine`: Python owner of one `tts_hip_engine` handle (one GPU, one HIP stream).

Inputs may be numpy arrays (host buffers: the library stages them over PCIe) or torch CUDA tensors (device buffers:
passed by pointer, results returned as torch tensors on the same device).  PyTorch is only used to host device memory.
Every call that takes arrays goes through `HipEngine._call`, which holds the host / device / stream rules.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import HipLibraryError, MelConfigC, MEM_DEVICE, MEM_HOST

# field order of the reference's namedtuple (architectures/tacotron2_arch.py:52-56)
Tacotron2InferenceOutput = namedtuple(
    'Tacotron2InferenceOutput', ['decoder_output', 'mel', 'stop_tokens', 'attention_weights', 'lengths'])

# what Tacotron2.call returns (tacotron2_arch.py:849) plus the alignments, which `call` drops
Tacotron2ForwardOutput = namedtuple('Tacotron2ForwardOutput', ['decoder_output', 'mel', 'stop_tokens', 'attention_weights'])

KERNEL_WN_IN, KERNEL_WN_RES_SKIP, KERNEL_DECODER_STEP = 0, 1, 2
_INT32 = (-2 ** 31, 2 ** 31 - 1)        # the range of a row table whose entries only the C side checks


def _is_torch_cuda(x) -> bool:
    return hasattr(x, 'data_ptr') and hasattr(x, 'is_cuda') and bool(x.is_cuda)


def _u64(v):
    return ctypes.c_uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


def _dims(x):
    """The shape of an array, a tensor or a nested sequence as a tuple of ints."""
    return tuple(int(n) for n in np.shape(x))


def attention_window(win_len, offset):
    """(win_len, win_off) as the ints the C API takes; `None` / 0 window -> (0, 0) (no window).  The offset is in positions
    here: a fraction of the window (the reference's default 0.5) is resolved by `HipRuntime.tacotron2_infer`."""
    if win_len is None or win_len == 0:
        return 0, 0
    if win_len != int(win_len) or win_len < 0:
        raise ValueError(f'attn_mask_win_len must be a non-negative integer, got {win_len!r}')
    if offset is None:
        offset = 0
    if offset != int(offset):
        raise ValueError(f'attn_mask_offset must be a whole number of positions at this level, got {offset!r}: '
                         'HipRuntime.tacotron2_infer resolves a fraction of the window')
    return int(win_len), int(offset)


class MelFn:
    """A mel plan of one engine (tts_hip_mel_fn; `HipEngine.mel_fn`).  It is freed when the engine closes."""

    def __init__(self, handle, cfg):
        self.handle = handle
        self.n_mel = int(cfg.n_mel_channels)
        self.geometry = {name: getattr(cfg, name) for name, _ in cfg._fields_}


class EncodedBatch:
    """Encoder output of one token batch, resident on the GPU (tts_hip_encoded).  Freed by `close()`, the garbage collector
    or the engine's own teardown order (an engine must outlive its encoded batches)."""

    def __init__(self, engine, handle, B, Tin, keep=(), on_device=False):
        self.engine, self.handle, self.B, self.Tin, self.on_device = engine, handle, B, Tin, on_device
        self._keep = keep                       # inputs of the still-running asynchronous encoder

    def close(self):
        if self.handle is not None and getattr(self.engine, '_h', None):
            self.engine._lib.tts_hip_encoded_free(self.engine._h, self.handle)
        self.handle = None
        self._keep = ()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipEngine:
    def __init__(self, device: int = 0):
        self._lib = _lib.load_library()
        self._h = ctypes.c_void_p()
        rc = self._lib.tts_hip_create(int(device), ctypes.byref(self._h))
        if rc != 0:
            self._h = None
            raise HipLibraryError(f'tts_hip_create(device={device}) failed with code {rc} (no usable MI355X GPU?)')
        self.device = int(device)

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, '_h', None):
            self._lib.tts_hip_destroy(self._h)          # frees the mel plans with the rest
            self._h = None
            getattr(self, '_mel_fns', {}).clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.tts_hip_last_error(self._h)
            raise HipLibraryError(f'{what} failed ({rc}): {msg.decode("utf-8", "replace") if msg else ""}')

    def _torch(self):
        import torch
        return torch

    def _check_device(self, *tensors):
        """Device tensors are passed by pointer: they must live on this engine's GPU (a pointer into another GPU's memory
        would be read as garbage or fault)."""
        for t in tensors:
            if t is not None and _is_torch_cuda(t) and t.device.index != self.device:
                raise ValueError(f'tensor on {t.device} passed to an engine on cuda:{self.device}')

    @staticmethod
    def _ptr(x):
        """NULL, a device tensor's or a host array's address."""
        if x is None:
            return None
        return ctypes.c_void_p(x.data_ptr()) if hasattr(x, 'data_ptr') else x.ctypes.data_as(ctypes.c_void_p)

    def _call(self, name, inputs, make_outputs, args, stream=None, device=None, twin=True):
        """tts_hip_<name> on host arrays or on CUDA tensors, synchronously or on a caller's stream -> the outputs.

        `inputs`: (array-like or None, shape or None, dtype name) each; an input becomes a contiguous array of that dtype and
        shape (None: its own).  `make_outputs(new)` returns the outputs as a tuple (None allowed), allocating with
        new(shape, dtype='float32', zeros=False) or handing on a caller's `out=` tensor.  `args(ins, outs, (mem, stream
        pointer))` returns what the C function takes after the handle; arrays and tensors in it are turned into their
        addresses here, so a host table (lengths, keys, a bias ...) put into it stays referenced until the C call has returned.
        `twin`: the entry point ends in the mem kind and has an _async twin that ends in the stream (appended here); not
        `twin`: one entry point, and `args` places the mem kind and the stream pointer itself.

        `device` (default: whether the first input is a CUDA tensor) decides between
          * a host call: numpy inputs and outputs, TTS_HIP_MEM_HOST; a `stream` is refused before any library call;
          * a device call: the other inputs are moved to this engine's GPU, every tensor must live there (`_check_device`), the
            outputs are CUDA tensors.  stream=None: inputs are converted and outputs allocated on torch's current stream,
            which is then drained (the engine runs on a stream of its own and returns after that drained), and the call takes
            TTS_HIP_MEM_DEVICE.  A torch.cuda.Stream: it first waits for what torch's current stream has queued (the inputs may
            still be in flight there), conversion and allocation happen with it as torch's current stream, and the caller's
            inputs and every prepared tensor are marked as used on it -- the caching allocator must not hand out a temporary
            freed when this method returns while the kernels still read it; the work is enqueued there and not waited for."""
        if device is None:
            device = _is_torch_cuda(inputs[0][0])
        if not device:
            if stream is not None:
                raise ValueError('stream= needs device tensors')
            def host(x, shape, dt):
                a = np.asarray(x.detach().cpu() if hasattr(x, 'detach') else x, dtype=dt)
                return np.ascontiguousarray(a if shape is None else a.reshape(shape))

            ins = [None if x is None else host(x, shape, dt) for x, shape, dt in inputs]
            outs = make_outputs(lambda shape, dtype='float32', zeros=False: (np.zeros if zeros else np.empty)(shape, dtype=dtype))
            mem, sp = MEM_HOST, None
        else:
            torch = self._torch()
            gpu = torch.device('cuda', self.device)
            self._check_device(*(x for x, _, _ in inputs))
            given = [x if x is None or _is_torch_cuda(x) else torch.as_tensor(np.asarray(x, dtype=dt), device=gpu)
                     for x, _, dt in inputs]

            def prepare():
                ins = [None if x is None else (x.to(getattr(torch, dt)) if shape is None else x.to(getattr(torch, dt)).reshape(shape)).contiguous()
                       for x, (_, shape, dt) in zip(given, inputs)]
                outs = make_outputs(lambda shape, dtype='float32', zeros=False:
                                    (torch.zeros if zeros else torch.empty)(shape, dtype=getattr(torch, dtype), device=gpu))
                self._check_device(*outs)
                return ins, outs

            current = torch.cuda.current_stream(self.device)
            mem, sp = MEM_DEVICE, None
            if stream is None:
                ins, outs = prepare()
                current.synchronize()
            else:
                stream.wait_stream(current)
                with torch.cuda.stream(stream):
                    ins, outs = prepare()
                for t in (*given, *ins, *outs):
                    if t is not None:
                        t.record_stream(stream)
                sp = ctypes.c_void_p(int(stream.cuda_stream))
                if twin:
                    name += '_async'
        argv = tuple(args(ins, outs, (mem, sp)))
        if twin:
            argv += (mem if stream is None else sp,)
        self._check(getattr(self._lib, 'tts_hip_' + name)(
            self._h, *(self._ptr(a) if isinstance(a, np.ndarray) or hasattr(a, 'data_ptr') else a for a in argv)), name)
        return outs

    @staticmethod
    def _row_table(values, B, lo, hi, what, name):
        """`values` (any int sequence / array / tensor), the `name` argument of call `what`, as a contiguous host int32 [B] with
        every entry in [lo, hi].  Raises before any GPU call."""
        if hasattr(values, 'detach'):
            values = values.detach().cpu().numpy()
        arr = np.atleast_1d(np.asarray(values))
        who = f'{what}: {name}' if what else name
        if arr.shape != (B,):
            raise ValueError(f'{who} must hold one value per row, shape ({B},), got {arr.shape}')
        if arr.dtype.kind not in 'iu':
            raise ValueError(f'{who} must be integers, got dtype {arr.dtype}')
        if int(arr.min()) < lo or int(arr.max()) > hi:
            raise ValueError(f'{who} must lie in [{lo}, {hi}], got {arr.tolist()}')
        return np.ascontiguousarray(arr, dtype=np.int32)

    @staticmethod
    def _frame_lengths(lengths, B, T):
        """`lengths` (any int sequence / array / tensor) as a contiguous host int32 [B] with every entry in [0, T]."""
        return HipEngine._row_table(lengths, B, 0, T, '', 'lengths')

    @staticmethod
    def _batched(x, rank):
        """The dims of `x`, [B, ...] of `rank` axes or one row of it without the batch axis (B = 1); None for any other rank."""
        shape = _dims(x)
        return (1, *shape) if len(shape) == rank - 1 else shape if len(shape) == rank else None

    # ------------------------------------------------------------------ device-side sampling
    def random_normal(self, shape, seed: int, offset: int = 0, stream=None):
        """N(0, 1) float32 tensor of `shape` on this engine's GPU, drawn on the device (Philox4x32-10 + Box-Muller,
        tts_hip_random_fill); the same (seed, offset) always gives the same values."""
        return self._random(0, shape, seed, offset, stream)

    def random_prenet_masks(self, B: int, max_len: int, seed: int, offset: int = 0, stream=None):
        """Prenet dropout masks [B, max_len, 2, 256] (2.0 with probability 0.5, else 0.0) drawn on the device."""
        return self._random(1, (int(B), int(max_len), 2, 256), seed, offset, stream)

    def _random(self, kind, shape, seed, offset, stream):
        out, = self._call('random_fill', [], lambda new: (new(tuple(shape)),),
                          lambda ins, outs, where: (kind, _u64(seed), _u64(offset), outs[0], outs[0].numel(), where[1]),
                          stream, device=True, twin=False)
        if stream is None:                      # the fill ran on the engine's own stream
            self.synchronize()
        return out

    @staticmethod
    def _row_tables(row_seeds, B=None, what='row_seeds'):
        """(keys, offsets) -> two contiguous host uint64 [B] arrays (offsets None or a scalar: that value for every row)."""
        if not isinstance(row_seeds, (tuple, list)) or len(row_seeds) != 2:
            raise ValueError(f'{what} must be (keys, offsets), one entry per row')
        keys, offsets = row_seeds
        as_u64 = lambda seq: np.ascontiguousarray([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.atleast_1d(np.asarray(seq, dtype=object))],
                                                  dtype=np.uint64)
        keys = as_u64(keys)
        offsets = as_u64([0] * len(keys) if offsets is None else
                         [offsets] * len(keys) if np.ndim(offsets) == 0 else offsets)
        if len(keys) == 0 or len(keys) != len(offsets) or (B is not None and len(keys) != B):
            raise ValueError(f'{what}: need one key and one offset per row'
                             + (f' ({B} rows)' if B is not None else '') + f', got {len(keys)} and {len(offsets)}')
        return keys, offsets

    def random_normal_rows(self, row_stride: int, keys, offsets=None, counts=None, stream=None, out=None):
        """N(0, 1) float32 [B, row_stride] on this engine's GPU with one Philox stream per row (tts_hip_random_fill_rows):
        row b, element i = element i of `random_normal` under (keys[b], offsets[b]) for i < counts[b] (default row_stride).
        Elements at i >= counts[b] are not written: they keep what `out` (a float32 CUDA tensor of B * row_stride elements to
        fill in place) held, or the zeros of a fresh tensor."""
        return self._random_rows(0, row_stride, keys, offsets, counts, stream, out)

    def random_prenet_masks_rows(self, row_stride: int, keys, offsets=None, counts=None, stream=None, out=None):
        """Prenet dropout mask values (2.0 with probability 0.5, else 0.0) [B, row_stride], one Philox stream per row, as
        `random_normal_rows`.  With row_stride = max_len * 512, `.view(B, max_len, 2, 256)` is what
        `tacotron2_decode(row_mask_seeds=(keys, offsets))` multiplies the prenet by."""
        return self._random_rows(1, row_stride, keys, offsets, counts, stream, out)

    def _random_rows(self, kind, row_stride, keys, offsets, counts, stream, out):
        keys, offsets = self._row_tables((keys, offsets))
        B, row_stride = len(keys), int(row_stride)
        if row_stride < 0:
            raise ValueError('row_stride must not be negative')
        cnt = None
        if counts is not None:                                   # int64, unlike the other row tables
            cnt = np.ascontiguousarray(np.asarray(counts, dtype=np.int64))
            if cnt.shape != (B,) or (B and (int(cnt.min()) < 0 or int(cnt.max()) > row_stride)):
                raise ValueError(f'counts must hold one value in [0, row_stride = {row_stride}] per row, got {cnt.tolist()}')
        if out is not None and (not _is_torch_cuda(out) or out.dtype != self._torch().float32 or not out.is_contiguous()
                                or out.numel() != B * row_stride):
            raise ValueError(f'out must be a contiguous float32 CUDA tensor of {B} x {row_stride} elements')
        out, = self._call('random_fill_rows', [], lambda new: (new((B, row_stride), zeros=True) if out is None else out,),
                          lambda ins, outs, where: (kind, keys, offsets, B, row_stride, cnt, outs[0], where[1]),
                          stream, device=True, twin=False)
        if stream is None:
            self.synchronize()
        return out

    # ------------------------------------------------------------------ weights
    def set_tensor(self, name: str, array) -> None:
        a = np.ascontiguousarray(array, dtype=np.float32)
        dims = (ctypes.c_int64 * a.ndim)(*a.shape)
        self._check(self._lib.tts_hip_set_tensor(self._h, name.encode(), self._ptr(a), dims, a.ndim), f'set_tensor({name})')

    def load_state(self, tensors) -> None:
        for k, v in tensors.items():
            self.set_tensor(k, v)

    def load_weights(self, path: str) -> None:
        self._check(self._lib.tts_hip_load_weights(self._h, str(path).encode()), f'load_weights({path})')

    def finalize(self) -> None:
        self._check(self._lib.tts_hip_finalize(self._h), 'finalize')

    def has_model(self, model: str) -> bool:
        return bool(self._lib.tts_hip_has_model(self._h, model.encode()))

    # ------------------------------------------------------------------ WaveGlow
    _WG_PRECISIONS = {'f32': 0, 'f16': 1, 'f16x3': 2}
    # (noise, rows) -> entry point, without the tts_hip_ prefix and the _async suffix of a call on a caller's stream
    _WG_ENTRY = {('z', 'plain'): 'waveglow_infer', ('z', 'ragged'): 'waveglow_infer_ragged', ('z', 'packed'): 'waveglow_infer_packed',
                 ('seed', 'plain'): 'waveglow_infer_seeded', ('rows', 'plain'): 'waveglow_infer_rows_seeded',
                 ('rows', 'ragged'): 'waveglow_infer_rows_seeded', ('rows', 'packed'): 'waveglow_infer_rows_seeded'}

    def _wg_inputs(self, mel, z=None, audio=None, lengths=None):
        """(B, T, int32 lengths or None) of a WaveGlow call on mel [B, T, 80], z [B, T*32, 8] and / or audio [B, T*256]."""
        shape = _dims(mel)
        if len(shape) != 3 or shape[2] != 80:
            raise ValueError(f'mel must be [B, T, 80], got {shape}')
        B, T = shape[:2]
        if z is not None and _dims(z) != (B, T * 32, 8):
            raise ValueError(f'z must be [B, T*32, 8] = {(B, T * 32, 8)}, got {_dims(z)}')
        if audio is not None and _dims(audio) != (B, T * 256):
            raise ValueError(f'audio must be [B, T*256] = {(B, T * 256)}, got {_dims(audio)}')
        return B, T, None if lengths is None else self._frame_lengths(lengths, B, T)

    def waveglow_infer(self, mel, z=None, sigma: float = 1.0, precision: str = 'f32', stream=None, seed=None, offset: int = 0,
                       lengths=None, packed: bool = False, row_seeds=None):
        """mel [B, T, 80] (+ optional z [B, T*32, 8]) -> audio [B, T*256].  precision: 'f32' (exact fp32 MFMA), 'f16x3'
        (split fp16: fp32-class accuracy, ~3x faster) or 'f16' (fp16 operands).  `seed` (with z=None): the noise is drawn
        on the device from (seed, offset) -- the reference's default `z=None, deterministic=False`
        (waveglow_arch.py:272-274,299-302) without a host-made tensor crossing PCIe; z=None and seed=None: zeros
        (`deterministic=True`).  `stream` (a torch.cuda.Stream, device tensors only): enqueue on that stream and return
        without waiting (tts_hip_waveglow_infer_async).
        `lengths` [B] (ints in [0, T]; brought to host int32): a batch of unequal rows (tts_hip_waveglow_infer_ragged) --
        audio[b, :lengths[b] * 256] is what row b's own frames give in a call of their own, audio[b, lengths[b] * 256:] is 0,
        and mel / z beyond a row's length are never read (they may be uninitialised).  With `seed` the noise is drawn in the
        batch layout [B, T*32, 8] as without lengths.
        `packed=True` (needs `lengths`): the same results computed as ONE packed row (tts_hip_waveglow_infer_packed) -- the real
        frames of all rows one after another, 4 zero gap frames between two rows -- so the work follows sum(lengths), not
        B * T.  The noise of `seed` is still drawn in the batch layout: a row gets the values the ragged call gives it.
        `row_seeds=(keys, offsets)` (one pair per row; excludes `z` and `seed`): row b's noise z[b, p, c] is normal element
        p * 8 + c of its own Philox stream (keys[b], offsets[b]), drawn inside the engine (tts_hip_waveglow_infer_rows_seeded)
        -- the values `random_normal_rows` gives -- whatever batch the row sits in.  With `lengths` (ragged or packed) a row's
        arithmetic is its own too, so its audio is that of a one-row call with its key up to fp32 re-association; without
        `lengths` the batch is a padded one and a row still hears its padding."""
        if packed and lengths is None:
            raise ValueError('packed=True needs lengths (one frame count per row)')
        if row_seeds is not None and (z is not None or seed is not None):
            raise ValueError('row_seeds excludes z and seed')
        if z is not None and seed is not None:
            raise ValueError('pass either z or seed, not both')
        if precision not in self._WG_PRECISIONS:
            raise ValueError(f"precision must be one of {tuple(self._WG_PRECISIONS)}, got {precision!r}")
        B, T, lens = self._wg_inputs(mel, z=z, lengths=lengths)
        keys, offsets = (None, None) if row_seeds is None else self._row_tables(row_seeds, B)
        # A batch seed has an entry point of its own for plain synchronous calls only; everywhere else the call is
        # `random_fill` into a device z, then the z entry point.  Host mel with lengths: the noise lives on the device, so
        # the mel joins it there (80 floats a frame against the noise's 256) and the audio comes back.
        fill = seed is not None and (lens is not None or stream is not None)
        via_device = fill and stream is None and not _is_torch_cuda(mel)
        # the entry point and its arguments: (h, mel, B, T, <rows and noise>, sigma, audio, precision, ..., mem | stream)
        noise = 'rows' if row_seeds is not None else 'seed' if seed is not None and not fill else 'z'
        name = self._WG_ENTRY[noise, 'packed' if packed else 'ragged' if lens is not None else 'plain']
        pcode = (self._WG_PRECISIONS[precision],)
        if name == 'waveglow_infer' and stream is None:          # the synchronous plain call has one symbol per precision
            name, pcode = name + {'f32': '', 'f16': '_f16', 'f16x3': '_f16x3'}[precision], ()

        def args(ins, outs, where):
            m, zz = ins
            if fill:                                             # on the stream of the call that reads it, ahead of it
                zz = outs[1]
                self._check(self._lib.tts_hip_random_fill(self._h, 0, _u64(seed), _u64(offset), self._ptr(zz), zz.numel(), where[1]),
                            'random_fill')
            if noise == 'rows':
                mid, last = (lens, keys, offsets), (1 if packed else 0,)
            elif noise == 'seed':
                mid, last = (_u64(seed), _u64(offset)), ()
            else:
                mid, last = ((zz,) if lens is None else (lens, zz)), ()
            return (m, B, T, *mid, float(sigma), outs[0], *pcode, *last)

        out = self._call(name, [(mel, None, 'float32'), (z, None, 'float32')],
                         lambda new: (new((B, T * 256)), new((B, T * 32, 8)) if fill else None), args, stream,
                         device=True if via_device else None)[0]
        return out.cpu().numpy() if via_device else out

    def waveglow_encode(self, audio, mel, lengths=None, stream=None):
        """The forward flow, audio [B, T*256] + mel [B, T, 80] -> (z [B, T*32, 8], stats float32 [3, B]), fp32
        (tts_hip_waveglow_encode): z in the layout `waveglow_infer` consumes, so `waveglow_infer(mel, z=z, sigma=1)` returns the
        audio; stats[0] = sum z^2, stats[1] = sum of the couplings' s, stats[2] = frames * 32 * sum_k log|det kernel_k| per row,
        over its real positions -- the row's log-likelihood under N(0, sigma^2) is -(stats[0] / (2 sigma^2)) + stats[1] +
        stats[2] up to the constant.  `lengths` [B] (ints in [0, T]): a batch of unequal rows -- audio and mel beyond a row's
        length are never read, z is 0 there and the row gets what a call on its own frames gives it.  numpy in gives numpy out,
        CUDA tensors in give tensors out; `stream` (a torch.cuda.Stream, device tensors only): enqueue there and return without
        waiting (tts_hip_waveglow_encode_async).  B * T is limited to one run (31 744 frames)."""
        if _is_torch_cuda(mel) != _is_torch_cuda(audio):
            raise ValueError('audio and mel must both be host arrays or both be CUDA tensors')
        B, T, lens = self._wg_inputs(mel, audio=audio, lengths=lengths)
        return self._call('waveglow_encode', [(audio, None, 'float32'), (mel, None, 'float32')],
                          lambda new: (new((B, T * 32, 8)), new((3, B))),
                          lambda ins, outs, where: (ins[0], ins[1], B, T, lens, outs[0], outs[1]), stream)

    def waveglow_encode_probe(self, audio, mel, lengths=None, flow: int = 11, what: str = 'state'):
        """Test hook (tts_hip_waveglow_encode_probe): run `waveglow_encode` on host arrays up to the end of flow `flow` (0 .. 11;
        -1: the init step audio @ kernel_0 only) and return either the flow state as stored (what='state': [B, T*32, n], what
        flow `flow` + 1 reads -- early channels gone, its matrix applied; n = 8, 6, 4 for flows -1 .. 2, 3 .. 6, 7 .. 10; after
        flow 11 z's channels 0 .. 3) or the per-position sum of s through that flow (what='slog': [B, T*32])."""
        whats = {'state': 0, 'slog': 1}
        if what not in whats:
            raise ValueError(f'what must be one of {tuple(whats)}')
        B, T, lens = self._wg_inputs(mel, audio=audio, lengths=lengths)
        flow = int(flow)
        shape = (B, T * 32) if what == 'slog' else (B, T * 32, 8 if flow <= 2 else 6 if flow <= 6 else 4)
        return self._call('waveglow_encode_probe', [(audio, None, 'float32'), (mel, None, 'float32')], lambda new: (new(shape),),
                          lambda ins, outs, where: (ins[0], ins[1], B, T, lens, flow, whats[what], outs[0]))[0]

    def waveglow_probe(self, mel, z=None, sigma: float = 1.0, precision: str = 'f32', flow: int = 11, what: str = 'acts',
                       layer: int = 0, lengths=None, packed: bool = False):
        """Test hook (tts_hip_waveglow_probe): run `waveglow_infer` in `precision` up to flow `flow` and return either the gated
        activations [B, T*32, C] (C = `waveglow_channels`) of its WN layer `layer` (what='acts') or the flow state [B, T*32, n] right after the flow,
        early output included (what='state'; the reference's audio after that flow), or the conditioning plane [B, T*32, 1024]
        of that layer -- sum_q V_q mel[t - q] + b, columns in the gate-interleaved order of the engine's weights -- that the
        fp32 Winograd form builds (what='cond'; layers 1 - 7 of calls of 144 frames or more, 512-channel models only).
        `lengths` [B] (tts_hip_waveglow_probe_rows): the one run of `waveglow_infer(.., lengths=)` stopped there, same shapes; the
        state is 0 behind a row's length, activations and planes are not specified there.  `packed=True` (needs `lengths`):
        the packed row of `waveglow_infer(.., lengths=, packed=True)` stopped there, in the packed row's OWN layout [F*32, width]
        (F frames: the rows that hold frames one after another, 4 gap frames between two; no scatter), state 0 on gap frames."""
        whats = {'acts': 0, 'state': 1, 'cond': 2}
        if precision not in self._WG_PRECISIONS or what not in whats:
            raise ValueError(f'precision must be one of {tuple(self._WG_PRECISIONS)} and what one of {tuple(whats)}')
        if packed and lengths is None:
            raise ValueError('packed=True needs lengths (one frame count per row)')
        B, T, lens = self._wg_inputs(mel, z=z, lengths=lengths)
        C = self.waveglow_channels
        width = C if what == 'acts' else 2 * C if what == 'cond' else (4 if flow >= 8 else 6 if flow >= 4 else 8) + (2 if flow in (4, 8) else 0)
        if lens is None:
            return self._call('waveglow_probe', [(mel, None, 'float32'), (z, None, 'float32')], lambda new: (new((B, T * 32, width)),),
                              lambda ins, outs, where: (ins[0], B, T, ins[1], float(sigma), self._WG_PRECISIONS[precision], int(flow),
                                                        whats[what], int(layer), outs[0]))[0]
        if packed:                                               # wg_packed_frames (csrc/wg_call.h)
            rows = int((lens > 0).sum())
            shape = ((int(lens.sum()) + 4 * max(rows - 1, 0)) * 32, width)
        else:
            shape = (B, T * 32, width)
        return self._call('waveglow_probe_rows', [(mel, None, 'float32'), (z, None, 'float32')], lambda new: (new(shape),),
                          lambda ins, outs, where: (ins[0], B, T, lens, 1 if packed else 0, ins[1], float(sigma),
                                                    self._WG_PRECISIONS[precision], int(flow), whats[what], int(layer), outs[0]))[0]

    def waveglow_probe_acts(self, mel, z=None, sigma: float = 1.0, flow: int = 11, layer: int = 1):
        """Test hook (tts_hip_waveglow_probe_acts): the gated activations [B, T*32, C] (C = `waveglow_channels`) of WN layer `layer` of flow `flow` on
        the fp32 path, in the form `set_waveglow_form` selects -- the values before the res/skip and `end` convolutions."""
        B, T, _ = self._wg_inputs(mel, z=z)
        C = self.waveglow_channels
        return self._call('waveglow_probe_acts', [(mel, None, 'float32'), (z, None, 'float32')], lambda new: (new((B, T * 32, C)),),
                          lambda ins, outs, where: (ins[0], B, T, ins[1], float(sigma), int(flow), int(layer), outs[0]))[0]

    def set_waveglow_form(self, form: str) -> None:
        """How the fp32 vocoder evaluates the dilated convolutions of WN layers 1 - 7: 'winograd' (default: minimal filtering
        along the tap axis, F(4,3), for calls of 144 frames or more) or 'direct' (always three taps).  Both are fp32; they differ by rounding only.
        The Winograd form exists for 512-channel models: with a 256-channel one (`waveglow_channels`) the call is accepted and
        every fp32 call still takes the direct form."""
        # 'winograd-3pass' / 'winograd-prepass': the two earlier stages of the Winograd form (pre-pass + per-product GEMM + combine
        # pass; fused GEMM behind the pre-pass), kept for measurement and as bit-identical cross-checks of the default kernel
        forms = {'direct': 0, 'winograd': 1, 'winograd-3pass': 2, 'winograd-prepass': 3}
        if form not in forms:
            raise ValueError(f'form must be one of {tuple(forms)}, got {form!r}')
        self._check(self._lib.tts_hip_set_waveglow_form(self._h, forms[form]), 'set_waveglow_form')

    @property
    def last_waveglow_form(self) -> str:
        """'winograd' or 'direct' for the last `waveglow_infer` call on this handle ('none' before the first)."""
        return {1: 'winograd', 0: 'direct'}.get(self._lib.tts_hip_last_waveglow_form(self._h), 'none')

    @property
    def waveglow_channels(self) -> int:
        """n_channels of this handle's WaveGlow (tts_hip_waveglow_channels): 512 or 256, fixed by the tensors present at
        `finalize`; 0 while no WaveGlow is finalized."""
        return int(self._lib.tts_hip_waveglow_channels(self._h))

    @property
    def last_waveglow_tiles(self) -> str:
        """WN GEMM tile family of the last `waveglow_infer` (or probe) call: '64-row', '128x64', '128-row' or '256-row'
        ('none' before the first)."""
        return {3: '64-row', 2: '128x64', 1: '128-row', 0: '256-row'}.get(self._lib.tts_hip_last_waveglow_tiles(self._h), 'none')

    # ------------------------------------------------------------------ Tacotron2
    _TACO_PRECISIONS = {'f32': 0, 'f16': 1}
    # mask source -> (decode entry point without the tts_hip_ prefix, what the call passes where `tacotron2_decode` takes the
    # masks, from src = the staged masks | (seed, offset) | the host tables (keys, offsets))
    _TACO_DECODE = {'tensor': ('tacotron2_decode', lambda src: (src,)),
                    'seed': ('tacotron2_decode_seeded', lambda src: (_u64(src[0]), _u64(src[1]))),
                    'rows': ('tacotron2_decode_rows_seeded', lambda src: tuple(src))}

    def _taco_precision(self, precision):
        if precision not in self._TACO_PRECISIONS:
            raise ValueError(f"precision must be 'f32' or 'f16', got {precision!r}")
        return self._TACO_PRECISIONS[precision]

    def _check_encoded(self, encoded):
        if encoded.engine is not self or encoded.handle is None:
            raise ValueError('this EncodedBatch belongs to another engine or was freed')

    @staticmethod
    def _token_dims(tokens):
        """(B, Tin) of tokens [B, Tin]."""
        shape = _dims(tokens)
        if len(shape) != 2:
            raise ValueError(f'tokens must be [B, Tin], got {shape}')
        return shape

    @staticmethod
    def _check_masks(masks, B, T, axis):
        """Prenet masks (or None) must be [B, T, 2, 256]; `axis` names T in the message."""
        if masks is not None and _dims(masks) != (B, T, 2, 256):
            raise ValueError(f'prenet_masks must be [B, {axis}, 2, 256] = {(B, T, 2, 256)}, got {_dims(masks)}')

    @staticmethod
    def _taco_outputs(new, B, T, Tin, want_attention=True, want_lengths=True):
        """Zero-filled (mel [B, T, 80], dec [B, T, 80], stop [B, T], attn [B, T, Tin] | None, lengths int32 [B] | None)."""
        return (new((B, T, 80), zeros=True), new((B, T, 80), zeros=True), new((B, T), zeros=True),
                new((B, T, Tin), zeros=True) if want_attention else None, new((B,), 'int32', zeros=True) if want_lengths else None)

    def tacotron2_infer(self, tokens, speaker=None, max_len: int = 1000, early_stopping: bool = True,
                        prenet_masks=None, attn_mask_win_len=None, attn_mask_offset: int = 0, want_attention=True,
                        precision: str = 'f32', row_mask_seeds=None):
        """tokens int32 [B, Tin] -> Tacotron2InferenceOutput of numpy arrays (or torch tensors for CUDA tokens).
        precision 'f16': decoder LSTM weights in fp16 (fp32 accumulate and state).
        `attn_mask_win_len` / `attn_mask_offset`: the attention window, both in positions (`attention_window`).
        `row_mask_seeds=(keys, offsets)` (excludes `prenet_masks`): the prenet dropout masks are drawn on the device, row b
        from its own stream (encode + `tacotron2_decode(row_mask_seeds=...)`)."""
        pcode = self._taco_precision(precision)
        if row_mask_seeds is not None:
            if prenet_masks is not None:
                raise ValueError('pass either prenet_masks or row_mask_seeds, not both')
            enc = self.tacotron2_encode(tokens, speaker=speaker)
            try:
                return self.tacotron2_decode(enc, max_len=max_len, early_stopping=early_stopping,
                                             attn_mask_win_len=attn_mask_win_len, attn_mask_offset=attn_mask_offset,
                                             want_attention=want_attention, precision=precision, row_mask_seeds=row_mask_seeds)
            finally:
                enc.close()
        win_len, win_off = attention_window(attn_mask_win_len, attn_mask_offset)
        max_len = int(max_len)
        if max_len <= 0:
            raise ValueError('max_len must be positive')
        B, Tin = self._token_dims(tokens)
        self._check_masks(prenet_masks, B, max_len, 'max_len')
        steps = ctypes.c_int32(0)
        mel, dec, stop, attn, lengths = self._call(
            'tacotron2_infer' + ('_f16' if pcode else ''),                 # one symbol per precision
            [(tokens, None, 'int32'), (speaker, None, 'float32'), (prenet_masks, None, 'float32')],
            lambda new: self._taco_outputs(new, B, max_len, Tin, want_attention),
            lambda ins, outs, where: (ins[0], B, Tin, ins[1], max_len, 1 if early_stopping else 0, ins[2], win_len, win_off, *outs,
                                      ctypes.cast(ctypes.byref(steps), ctypes.c_void_p)))
        self.last_steps = int(steps.value)
        return Tacotron2InferenceOutput(decoder_output=dec, mel=mel, stop_tokens=stop, attention_weights=attn, lengths=lengths)

    # ------------------------------------------------------------------ Tacotron2 in two calls
    def tacotron2_encode(self, tokens, speaker=None, stream=None, into=None):
        """tokens int32 [B, Tin] (+ speaker [B, E]) -> `EncodedBatch` (the encoder's output, kept on the GPU).  Asynchronous:
        the encoder is only enqueued (on `stream`, a torch.cuda.Stream, or on the engine's own stream).  `into`: an
        `EncodedBatch` of this engine to overwrite (tts_hip_tacotron2_reencode: no allocation, the decoder's cached graphs
        stay valid); it is returned."""
        B, Tin = self._token_dims(tokens)
        if into is not None and (into.engine is not self or into.handle is None):
            raise ValueError('`into` belongs to another engine or was freed')
        h, keep = ctypes.c_void_p(), []

        def args(ins, outs, where):
            keep.extend(ins)
            if into is not None:
                return (into.handle, ins[0], B, Tin, ins[1], *where)
            return (ins[0], B, Tin, ins[1], *where, ctypes.byref(h))

        self._call('tacotron2_encode' if into is None else 'tacotron2_reencode', [(tokens, None, 'int32'), (speaker, None, 'float32')],
                   lambda new: (), args, stream, twin=False)
        if into is None:
            return EncodedBatch(self, h, B, Tin, keep=tuple(keep), on_device=_is_torch_cuda(tokens))
        into.B, into.Tin, into.on_device, into._keep = B, Tin, _is_torch_cuda(tokens), tuple(keep)
        return into

    def tacotron2_decode(self, encoded, max_len: int = 1000, early_stopping: bool = True, prenet_masks=None,
                         attn_mask_win_len=None, attn_mask_offset: int = 0, want_attention=True, precision: str = 'f32',
                         stream=None, mask_seed=None, row_mask_seeds=None):
        """Decoder loop + postnet on an `EncodedBatch`; may be called repeatedly (new dropout masks, other `max_len`).
        `mask_seed` = (seed, offset): the prenet dropout masks are drawn on the device (tts_hip_tacotron2_decode_seeded)
        instead of being passed in.  Returns after `stream` (or the engine's stream) has drained: the loop's length is
        decided on the GPU.  (`stream` only matters for a batch encoded from device tensors.)
        `row_mask_seeds` = (keys, offsets), one pair per row: row b's masks [max_len, 2, 256] are mask elements
        0 .. max_len * 512 of its own stream (tts_hip_tacotron2_decode_rows_seeded; `random_prenet_masks_rows` returns the same
        values), so a row draws the same dropout whichever rows it is decoded with and whatever `max_len` they impose."""
        given = [k for k, v in (('tensor', prenet_masks), ('seed', mask_seed), ('rows', row_mask_seeds)) if v is not None]
        if len(given) > 1:
            raise ValueError('pass only one of prenet_masks, mask_seed and row_mask_seeds')
        source = given[0] if given else 'tensor'
        row_tables = None if row_mask_seeds is None else self._row_tables(row_mask_seeds, encoded.B, 'row_mask_seeds')
        pcode = self._taco_precision(precision)
        win_len, win_off = attention_window(attn_mask_win_len, attn_mask_offset)
        self._check_encoded(encoded)
        B, Tin, dev = encoded.B, encoded.Tin, encoded.on_device
        max_len = int(max_len)
        if max_len <= 0:
            raise ValueError('max_len must be positive')
        self._check_masks(prenet_masks, B, max_len, 'max_len')
        steps = ctypes.c_int32(0)
        name, mid = self._TACO_DECODE[source]
        mel, dec, stop, attn, lengths = self._call(
            name, [(prenet_masks, None, 'float32')], lambda new: self._taco_outputs(new, B, max_len, Tin, want_attention),
            lambda ins, outs, where: (encoded.handle, max_len, 1 if early_stopping else 0,
                                      *mid({'tensor': ins[0], 'seed': mask_seed, 'rows': row_tables}[source]),
                                      win_len, win_off, pcode, *outs, ctypes.cast(ctypes.byref(steps), ctypes.c_void_p), *where),
            stream if dev else None, device=dev, twin=False)
        self.last_steps = int(steps.value)
        return Tacotron2InferenceOutput(decoder_output=dec, mel=mel, stop_tokens=stop, attention_weights=attn, lengths=lengths)

    def tacotron2_forward(self, tokens, mel_input, mel_lengths=None, speaker=None, prenet_masks=None, seed=None,
                          offset: int = 0, precision: str = 'f32', stream=None):
        """Teacher-forced pass (Tacotron2.call; tts_hip_tacotron2_forward): step t of the decoder reads `mel_input[:, t]`
        instead of its own previous output, every row runs all T steps.  `tokens`: int32 [B, Tin] (0 = pad; with `speaker`
        [B, E] for a multi-speaker model) or an `EncodedBatch`.  `mel_input` float32 [B, T, 80] is ALREADY SHIFTED: frame 0 is
        the zero go-frame, frame t is target frame t - 1.  `mel_lengths` [B] (default: T for every row), each in 1 .. T:
        decoder_output and mel are zero / masked where t > mel_lengths[b]; stop tokens and attention are not masked.
        Dropout: `prenet_masks` [B, T, 2, 256], or `seed` (the masks of `random_prenet_masks(B, T, seed, offset)`), or
        neither (deterministic).  numpy in gives numpy out; CUDA tensors in give CUDA tensors out.
        Repeated calls: pass an `EncodedBatch` (`tacotron2_encode`, re-filled with `into=`) -- the chunk graphs are cached per
        encoded batch and replayed; a call made from tokens encodes into a fresh buffer, which empties the handle's graph
        cache (decode graphs included), so it captures its graph anew every time.
        Returns Tacotron2ForwardOutput(decoder_output [B, T, 80], mel [B, T, 80], stop_tokens [B, T],
        attention_weights [B, T, Tin]) after `stream` (or the engine's stream) has drained."""
        pcode = self._taco_precision(precision)
        if seed is not None and prenet_masks is not None:
            raise ValueError('pass either prenet_masks or seed, not both')
        dev = _is_torch_cuda(mel_input)
        if stream is not None and not dev:
            raise ValueError('stream= needs device tensors')
        own = not isinstance(tokens, EncodedBatch)
        if own:
            if _is_torch_cuda(tokens) != dev:
                raise ValueError('tokens and mel_input must both be numpy arrays or both CUDA tensors')
            encoded = self.tacotron2_encode(tokens, speaker=speaker, stream=stream)
        else:
            encoded = tokens
            self._check_encoded(encoded)
        try:
            B, Tin = encoded.B, encoded.Tin
            shape = _dims(mel_input)
            if len(shape) != 3 or shape[0] != B or shape[2] != 80:
                raise ValueError(f'mel_input must be [B = {B}, T, 80], got {shape}')
            T = shape[1]
            lens = np.full((B,), T, np.int32) if mel_lengths is None else self._row_table(mel_lengths, B, *_INT32, '', 'mel_lengths')
            if seed is not None:
                prenet_masks = self.random_prenet_masks(B, T, seed, offset, stream=stream)
                if not dev:
                    prenet_masks = prenet_masks.cpu().numpy()
            self._check_masks(prenet_masks, B, T, 'T')
            mel, dec, stop, attn, _ = self._call(
                'tacotron2_forward', [(mel_input, None, 'float32'), (prenet_masks, None, 'float32')],
                lambda new: self._taco_outputs(new, B, T, Tin, want_lengths=False),
                lambda ins, outs, where: (encoded.handle, ins[0], T, lens, ins[1], pcode, *outs[:4], *where), stream, twin=False)
        finally:
            if own:
                encoded.close()
        return Tacotron2ForwardOutput(decoder_output=dec, mel=mel, stop_tokens=stop, attention_weights=attn)

    def tacotron2_loss(self, mel_target, gate_target, decoder_output, mel, stop_tokens, *, mel_loss='mse', mask_mel_padding=True,
                       from_logits=False, finish_weight=1., not_finish_weight=1., stream=None):
        """The reference's TacotronLoss per sample (tts_hip_tacotron2_loss; the math is pinned in include/tts_hip.h):
        `mel_target`, `decoder_output`, `mel` [B, T, 80] and `gate_target`, `stop_tokens` [B, T] -> float32 [K, B], K = 2 + 2 x
        the number of `mel_loss` kinds, rows in the order of `losses.loss_output_names(mel_loss)`: loss, <kind>_mel_loss ...,
        <kind>_mel_postnet_loss ..., gate_loss.  `mel_loss`: one of 'mse', 'mae', 'weighted_mse', 'weighted_mae' or a list of
        1 to 4 distinct ones.  `stop_tokens` are probabilities (what `tacotron2_forward` returns) unless `from_logits`.
        numpy in gives numpy out.  If any input is a CUDA tensor the rest are moved to the GPU and a CUDA tensor comes back:
        the outputs of `tacotron2_forward` go in as they are, on `stream` (a torch.cuda.Stream) if one is given.  Specified for
        finite inputs only: the padding mask multiplies the error, so a non-finite value in a masked frame propagates.
        Returns after `stream` (or the engine's stream) has drained.  Needs no weights."""
        from .losses import MEL_LOSS_KINDS, mel_loss_kinds
        kinds = np.asarray([MEL_LOSS_KINDS[k] for k in mel_loss_kinds(mel_loss)], dtype=np.int32)
        inputs = (mel_target, gate_target, decoder_output, mel, stop_tokens)
        shape = _dims(mel_target)
        if len(shape) != 3 or shape[2] != 80:
            raise ValueError(f'mel_target must be [B, T, 80], got {shape}')
        B, T = shape[:2]
        for name, x, want in (('gate_target', gate_target, (B, T)), ('decoder_output', decoder_output, shape), ('mel', mel, shape),
                              ('stop_tokens', stop_tokens, (B, T))):
            if _dims(x) != want:
                raise ValueError(f'{name} must be {want} beside mel_target {shape}, got {_dims(x)}')
        return self._call('tacotron2_loss', [(x, None, 'float32') for x in inputs], lambda new: (new((len(kinds) * 2 + 2, B)),),
                          lambda ins, outs, where: (*ins, B, T, kinds, len(kinds), 1 if mask_mel_padding else 0, 1 if from_logits else 0,
                                                    float(finish_weight), float(not_finish_weight), outs[0], *where),
                          stream, device=any(_is_torch_cuda(x) for x in inputs), twin=False)[0]

    # ------------------------------------------------------------------ MCD along a DTW path
    DTW_ALIGN, DTW_C0 = 1, 2                        # TTS_HIP_DTW_*
    DTW_STAGES = {'cepstra_a': 0, 'cepstra_b': 1, 'distance': 2, 'cost': 3, 'step': 4}

    def _dtw_request(self, who, a, b, lengths_a, lengths_b, n_cep, include_c0, align):
        """The checked arguments of a `mel_dtw` / `mel_dtw_probe` call -> (B, Ta, Tb, n_mel, len_a, len_b, n_cep, flags)."""
        sa, sb = self._batched(a, 3) if len(_dims(a)) == len(_dims(b)) else None, self._batched(b, 3)
        if sa is None or sb is None or sa[0] != sb[0] or sa[2] != sb[2] or min(sa + sb) < 1:
            raise ValueError(f'{who}: a and b must be [B, Ta, n_mel] and [B, Tb, n_mel] (or one row of each), got {_dims(a)} and {_dims(b)}')
        (B, Ta, n_mel), Tb = sa, sb[1]
        if not 2 <= n_mel <= 128:
            raise ValueError(f'{who}: n_mel = {n_mel} is outside [2, 128]')
        if n_cep != int(n_cep) or not 1 <= int(n_cep) <= n_mel - 1:
            raise ValueError(f'{who}: n_cep = {n_cep!r} is outside [1, n_mel - 1 = {n_mel - 1}]')
        la = None if lengths_a is None else self._row_table(lengths_a, B, 1, Ta, who, 'lengths_a')
        lb = None if lengths_b is None else self._row_table(lengths_b, B, 1, Tb, who, 'lengths_b')
        flags = (self.DTW_ALIGN if align else 0) | (self.DTW_C0 if include_c0 else 0)
        return B, Ta, Tb, n_mel, la, lb, int(n_cep), flags

    def mel_dtw(self, a, b, lengths_a=None, lengths_b=None, *, n_cep=13, include_c0=False, align=True, return_path=False,
                stream=None):
        """Mel-cepstral distortion of log-mels `a` [B, Ta, n_mel] against `b` [B, Tb, n_mel] along their dynamic-time-warping
        path, per row (tts_hip_mel_dtw; the math is pinned in include/tts_hip.h).  `lengths_a` / `lengths_b` [B], each in
        1 .. Ta / 1 .. Tb (default: full): nothing at or behind a row's length is read.  The cepstra are rows 1 .. n_cep of the
        orthonormal DCT-II of a frame (0 .. n_cep with `include_c0`).  `align=False`: no warping, the frames (t, t) below the
        shorter length.  Returns float32 [3, B] = cost, path length, MCD in dB; with `return_path` also int32
        [B, Ta + Tb - 1, 2], the pairs (i, j) from (0, 0) onwards and -1 behind the path's end.  One row of each operand
        without the batch axis is taken as B = 1.  numpy in gives numpy out; if either operand is a CUDA tensor the other is
        moved to the GPU and CUDA tensors come back, on `stream` (a torch.cuda.Stream) if one is given.  Returns after
        `stream` (or the engine's stream) has drained.  Needs no weights."""
        B, Ta, Tb, n_mel, la, lb, n_cep, flags = self._dtw_request('mel_dtw', a, b, lengths_a, lengths_b, n_cep, include_c0, align)
        outs = self._call('mel_dtw', [(a, (B, Ta, n_mel), 'float32'), (b, (B, Tb, n_mel), 'float32')],
                          lambda new: (new((3, B)), new((B, Ta + Tb - 1, 2), 'int32') if return_path else None),
                          lambda ins, outs, where: (*ins, B, Ta, Tb, n_mel, la, lb, n_cep, flags, *outs, *where),
                          stream, device=_is_torch_cuda(a) or _is_torch_cuda(b), twin=False)
        return outs if return_path else outs[0]

    def mel_dtw_probe(self, a, b, lengths_a=None, lengths_b=None, *, n_cep=13, include_c0=False, what='cost'):
        """Test hook (tts_hip_mel_dtw_probe): the aligned programme of `mel_dtw` up to one stage, returned dense with zeros at
        and behind the lengths: what='cepstra_a' [B, Ta, R] / 'cepstra_b' [B, Tb, R] (R = n_cep, + 1 with `include_c0`),
        'distance', 'cost', 'step' [B, Ta, Tb] (the step codes 0 diagonal, 1 from (i-1, j), 2 from (i, j-1) as float32)."""
        if what not in self.DTW_STAGES:
            raise ValueError(f'what must be one of {tuple(self.DTW_STAGES)}, got {what!r}')
        B, Ta, Tb, n_mel, la, lb, n_cep, flags = self._dtw_request('mel_dtw_probe', a, b, lengths_a, lengths_b, n_cep, include_c0, True)
        R = n_cep + (1 if include_c0 else 0)
        shape = (B, Ta, R) if what == 'cepstra_a' else (B, Tb, R) if what == 'cepstra_b' else (B, Ta, Tb)
        return self._call('mel_dtw_probe', [(a, (B, Ta, n_mel), 'float32'), (b, (B, Tb, n_mel), 'float32')], lambda new: (new(shape),),
                          lambda ins, outs, where: (*ins, B, Ta, Tb, n_mel, la, lb, n_cep, flags, self.DTW_STAGES[what], outs[0], *where),
                          device=_is_torch_cuda(a) or _is_torch_cuda(b), twin=False)[0]

    # ------------------------------------------------------------------ pitch tracks (YIN) and their comparison
    PITCH_STAGES = {'difference': 0, 'cmnd': 1, 'pick': 2}      # TTS_HIP_PITCH_*
    PITCH_MAX_WIN, PITCH_MAX_LAG = 2048, 1024
    GROSS_CENTS = 1200.0 * float(np.log2(1.2))                  # a gross pitch error: more than 20 % off

    def _pitch_request(self, who, audio, lengths, rate, hop, win, fmin, fmax, threshold):
        """The checked arguments of a `pitch` / `pitch_probe` call -> (B, N, F, lengths, rate, hop, win, tau_min, tau_max,
        threshold).  Raises before any library call."""
        from .pitch import hz_to_lags
        shape = self._batched(audio, 2)
        if shape is None or min(shape) < 1:
            raise ValueError(f'{who}: audio must be [B, N] (or one row [N]), got {_dims(audio)}')
        B, N = shape
        for name, v in (('rate', rate), ('hop', hop), ('win', win)):
            if v != int(v) or int(v) < 1:
                raise ValueError(f'{who}: {name} = {v!r} must be a positive integer')
        rate, hop, win = int(rate), int(hop), int(win)
        if not 2 <= win <= self.PITCH_MAX_WIN:
            raise ValueError(f'{who}: win = {win} is outside [2, {self.PITCH_MAX_WIN}]')
        if hop > win:
            raise ValueError(f'{who}: hop = {hop} is outside [1, win = {win}]')
        tau_min, tau_max = hz_to_lags(rate, fmin, fmax)
        if tau_min < 1 or tau_min >= tau_max or tau_max > self.PITCH_MAX_LAG:
            raise ValueError(f'{who}: fmin = {fmin!r}, fmax = {fmax!r} at rate {rate} give the lags [{tau_min}, {tau_max}]: '
                             f'need 1 <= tau_min < tau_max <= {self.PITCH_MAX_LAG}')
        if not 0.0 < float(np.float32(threshold)) <= 1.0:             # as the library receives it: a float32
            raise ValueError(f'{who}: threshold = {threshold!r} is outside (0, 1] as a float32')
        if N > 2 ** 24:
            raise ValueError(f'{who}: N = {N} is above 2^24 samples')
        lens = None if lengths is None else self._row_table(lengths, B, 1, N, who, 'lengths')
        return B, N, 1 + N // hop, lens, rate, hop, win, tau_min, tau_max, float(threshold)

    def pitch(self, audio, lengths=None, *, rate=22050, hop=256, win=1024, fmin=60., fmax=500., threshold=0.1, stream=None):
        """YIN pitch tracks of `audio` [B, N] (tts_hip_pitch; the math is pinned in include/tts_hip.h).  `lengths` [B], each in
        1 .. N (default: full): nothing at or behind a row's length is read.  Lags tau_min = ceil(rate / fmax) ..
        tau_max = floor(rate / fmin) are searched (45 .. 367 at the defaults), over windows of `win` samples every `hop`.
        Returns float32 [3, B, F], F = 1 + N // hop: f0 in Hz (0 where unvoiced), the period in samples, the aperiodicity
        d'(tau*); zeros at and behind a row's 1 + lengths[b] // hop frames.  For hop = 256 and 1024 samples or more the frames
        are those of the default mel plan.  One row without the batch axis is taken as B = 1.  numpy in gives numpy out, a
        CUDA tensor in gives a CUDA tensor out, on `stream` (a torch.cuda.Stream) if one is given.  Returns after `stream` (or
        the engine's stream) has drained.  Needs no weights."""
        B, N, F, lens, rate, hop, win, tau_min, tau_max, threshold = self._pitch_request('pitch', audio, lengths, rate, hop, win, fmin,
                                                                                         fmax, threshold)
        return self._call('pitch', [(audio, (B, N), 'float32')], lambda new: (new((3, B, F)),),
                          lambda ins, outs, where: (ins[0], B, N, lens, rate, hop, win, tau_min, tau_max, threshold, outs[0], *where),
                          stream, twin=False)[0]

    def pitch_probe(self, audio, lengths=None, *, rate=22050, hop=256, win=1024, fmin=60., fmax=500., threshold=0.1, what='cmnd'):
        """Test hook (tts_hip_pitch_probe): one stage of `pitch`, dense with zeros at and behind a row's frames:
        what='difference' (d) / 'cmnd' (d') [B, F, tau_max + 1], 'pick' [2, B, F] (the voiced flag and tau* as float32)."""
        if what not in self.PITCH_STAGES:
            raise ValueError(f'what must be one of {tuple(self.PITCH_STAGES)}, got {what!r}')
        B, N, F, lens, rate, hop, win, tau_min, tau_max, threshold = self._pitch_request('pitch_probe', audio, lengths, rate, hop, win,
                                                                                         fmin, fmax, threshold)
        shape = (2, B, F) if what == 'pick' else (B, F, tau_max + 1)
        if int(np.prod(shape)) * 4 >= 2 ** 31:
            raise ValueError(f'pitch_probe: a result of shape {shape} is 2^31 bytes or more')
        return self._call('pitch_probe', [(audio, (B, N), 'float32')], lambda new: (new(shape),),
                          lambda ins, outs, where: (ins[0], B, N, lens, rate, hop, win, tau_min, tau_max, threshold,
                                                    self.PITCH_STAGES[what], outs[0], *where), twin=False)[0]

    PYIN_STAGES = {'trough': 0, 'obs': 1, 'delta': 2, 'back': 3, 'path': 4}      # TTS_HIP_PYIN_*
    PYIN_MAX_BINS, PYIN_MAX_BPS, PYIN_MAX_THRESHOLDS = 1024, 100, 1024

    def _pyin_request(self, who, audio, lengths, rate, hop, win, fmin, fmax, bins_per_semitone, beta, n_thresholds, max_transition_rate,
                      switch_prob, no_trough_prob, prior=None, n_bins=None, max_step=None):
        """The checked arguments of a `pyin` / `pyin_probe` call -> (B, N, F, the C arguments from `lengths` to `switch_prob`,
        tau_max, n_bins).  `prior`: a table of its own in place of `beta_prior(*beta, n_thresholds)`; `n_bins`, `max_step`: those in
        place of what `pitch.pyin_geometry` gives.  Raises before any library call."""
        from .pitch import beta_prior, pyin_geometry
        B, N, F, lens, rate, hop, win, tau_min, tau_max, _ = self._pitch_request(who, audio, lengths, rate, hop, win, fmin, fmax, 0.5)
        if bins_per_semitone != int(bins_per_semitone) or not 1 <= int(bins_per_semitone) <= self.PYIN_MAX_BPS:
            raise ValueError(f'{who}: bins_per_semitone = {bins_per_semitone!r} must be an integer in [1, {self.PYIN_MAX_BPS}]')
        geometry = pyin_geometry(rate, hop, fmin, fmax, int(bins_per_semitone), max_transition_rate)
        n_bins = geometry[0] if n_bins is None else int(n_bins)
        max_step = min(geometry[1], n_bins) if max_step is None else int(max_step)
        if not 1 <= max_step <= n_bins and 1 <= n_bins <= self.PYIN_MAX_BINS:
            raise ValueError(f'{who}: max_step = {max_step} is outside [1, n_bins = {n_bins}]')
        if not 1 <= n_bins <= self.PYIN_MAX_BINS:
            raise ValueError(f'{who}: fmin = {fmin!r}, fmax = {fmax!r} at {bins_per_semitone} bins a semitone give {n_bins} bins: '
                             f'need 1 .. {self.PYIN_MAX_BINS}')
        if prior is None:
            if n_thresholds != int(n_thresholds) or not 1 <= int(n_thresholds) <= self.PYIN_MAX_THRESHOLDS:
                raise ValueError(f'{who}: n_thresholds = {n_thresholds!r} must be an integer in [1, {self.PYIN_MAX_THRESHOLDS}]')
            prior = beta_prior(int(beta[0]), int(beta[1]), int(n_thresholds)) if tuple(beta) == (int(beta[0]), int(beta[1])) else None
            if prior is None:
                raise ValueError(f'{who}: beta = {beta!r} must be two integers')
        prior = np.ascontiguousarray(np.asarray(prior, dtype=np.float64).reshape(-1), dtype=np.float32)
        if not 1 <= len(prior) <= self.PYIN_MAX_THRESHOLDS or not (np.isfinite(prior).all() and (prior >= 0).all()):
            raise ValueError(f'{who}: the prior must hold 1 .. {self.PYIN_MAX_THRESHOLDS} finite entries that are not negative')
        if not 0.0 < float(np.float32(switch_prob)) < 1.0:
            raise ValueError(f'{who}: switch_prob = {switch_prob!r} is outside (0, 1) as a float32')
        if not 0.0 <= float(np.float32(no_trough_prob)) <= 1.0:
            raise ValueError(f'{who}: no_trough_prob = {no_trough_prob!r} is outside [0, 1]')
        if B * F * 2 * n_bins * 2 >= 2 ** 31 or B * F * n_bins * 4 >= 2 ** 31:
            raise ValueError(f'{who}: B = {B}, F = {F}, n_bins = {n_bins}: observations or backpointers of 2^31 bytes or more; split the batch')
        c_args = (lens, rate, hop, win, tau_min, tau_max, prior, len(prior), float(no_trough_prob), float(fmin), int(bins_per_semitone),
                  n_bins, max_step, float(switch_prob))
        return B, N, F, c_args, tau_max, n_bins

    def pyin(self, audio, lengths=None, *, rate=22050, hop=256, win=1024, fmin=60., fmax=500., bins_per_semitone=10, beta=(2, 18),
             n_thresholds=100, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, prior=None, n_bins=None, max_step=None, stream=None):
        """Probabilistic-YIN pitch tracks of `audio` [B, N] (tts_hip_pyin; the math is pinned in include/tts_hip.h): every trough
        of the frames' d' (those of `pitch`, bit for bit) is a candidate whose probability sums the Beta(`beta`) prior over
        `n_thresholds` thresholds, and a Viterbi decode over `bins_per_semitone` pitch bins a semitone from `fmin` to `fmax`,
        voiced and unvoiced, chooses track and voicing; a step of the track is at most `max_transition_rate` octaves a second
        (`pitch.pyin_geometry`), voicing changes with `switch_prob`.  Returns float32 [3, B, F], F = 1 + N // hop: f0 in Hz (0
        where the decoded state is unvoiced), the pitch of the decoded bin whether voiced or not, the voiced probability; zeros
        at and behind a row's frames.  `prior` (a table of threshold masses), `n_bins` and `max_step` replace what `beta` and the
        geometry give.  Operands, `lengths` and `stream` as for `pitch`.  Needs no weights."""
        B, N, F, c_args, _, _ = self._pyin_request('pyin', audio, lengths, rate, hop, win, fmin, fmax, bins_per_semitone, beta,
                                                   n_thresholds, max_transition_rate, switch_prob, no_trough_prob, prior, n_bins, max_step)
        return self._call('pyin', [(audio, (B, N), 'float32')], lambda new: (new((3, B, F)),),
                          lambda ins, outs, where: (ins[0], B, N, *c_args, outs[0], *where), stream, twin=False)[0]

    def pyin_probe(self, audio, lengths=None, *, rate=22050, hop=256, win=1024, fmin=60., fmax=500., bins_per_semitone=10, beta=(2, 18),
                   n_thresholds=100, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, prior=None, n_bins=None, max_step=None,
                   what='obs'):
        """Test hook (tts_hip_pyin_probe): one stage of `pyin`, dense with zeros at and behind a row's frames: what='trough' (p
        per lag) [B, F, tau_max + 1], 'obs' [2, B, F, n_bins] (obs, cand), 'delta' / 'back' [B, F, 2 n_bins], 'path' [B, F]."""
        if what not in self.PYIN_STAGES:
            raise ValueError(f'what must be one of {tuple(self.PYIN_STAGES)}, got {what!r}')
        B, N, F, c_args, tau_max, n_bins = self._pyin_request('pyin_probe', audio, lengths, rate, hop, win, fmin, fmax, bins_per_semitone,
                                                              beta, n_thresholds, max_transition_rate, switch_prob, no_trough_prob, prior,
                                                              n_bins, max_step)
        shape = {'trough': (B, F, tau_max + 1), 'obs': (2, B, F, n_bins), 'path': (B, F)}.get(what, (B, F, 2 * n_bins))
        if int(np.prod(shape)) * 4 >= 2 ** 31:
            raise ValueError(f'pyin_probe: a result of shape {shape} is 2^31 bytes or more')
        return self._call('pyin_probe', [(audio, (B, N), 'float32')], lambda new: (new(shape),),
                          lambda ins, outs, where: (ins[0], B, N, *c_args, self.PYIN_STAGES[what], outs[0], *where), twin=False)[0]

    def f0_error(self, f0_a, f0_b, lengths_a=None, lengths_b=None, path=None, *, gross_cents=GROSS_CENTS, stream=None):
        """F0 tracks `f0_a` [B, Fa] against `f0_b` [B, Fb] (Hz, a frame is voiced iff > 0) along `path` (tts_hip_f0_error):
        None = the diagonal below the shorter length, else int32 [B, P, 2] as `mel_dtw(return_path=True)` returns it -- a
        row's path ends at its first pair that is negative or out of the row's frames.  `lengths_*` [B]: the real frames of
        each row (default: full).  Returns float32 [6, B] = pairs, voiced_pairs, rmse_cents, mean_cents, vuv_errors,
        gross_errors (both voiced and more than `gross_cents` apart; the default is 20 %).  One row of each operand without
        the batch axis is taken as B = 1.  numpy in gives numpy out; if any operand is a CUDA tensor the others are moved to the
        GPU and a CUDA tensor comes back, on `stream` if one is given.  Needs no weights."""
        sa, sb = self._batched(f0_a, 2) if len(_dims(f0_a)) == len(_dims(f0_b)) else None, self._batched(f0_b, 2)
        if sa is None or sb is None or sa[0] != sb[0] or min(sa + sb) < 1:
            raise ValueError(f'f0_error: f0_a and f0_b must be [B, Fa] and [B, Fb] (or one row of each), got {_dims(f0_a)} and {_dims(f0_b)}')
        (B, Fa), Fb = sa, sb[1]
        P = 0
        if path is not None:
            sp = _dims(path)
            sp = (1, *sp) if len(sp) == 2 and len(_dims(f0_a)) == 1 else sp
            if len(sp) != 3 or sp[0] != B or sp[1] < 1 or sp[2] != 2:
                raise ValueError(f'f0_error: path must be [B = {B}, P, 2], got {_dims(path)}')
            P = sp[1]
            if P > Fa + Fb:
                raise ValueError(f'f0_error: a path of {P} pairs is longer than Fa + Fb = {Fa + Fb}')
        if not (np.isfinite(np.float32(gross_cents)) and np.float32(gross_cents) > 0):
            raise ValueError(f'f0_error: gross_cents = {gross_cents!r} must be finite and positive')
        if Fa > 8192 or Fb > 8192 or B * (Fa + Fb) > 2 ** 19:
            raise ValueError(f'f0_error: B = {B}, Fa = {Fa}, Fb = {Fb} is above 8192 frames a side or 2^19 frames in all; split the batch')
        la = None if lengths_a is None else self._row_table(lengths_a, B, 1, Fa, 'f0_error', 'lengths_a')
        lb = None if lengths_b is None else self._row_table(lengths_b, B, 1, Fb, 'f0_error', 'lengths_b')
        return self._call('f0_error', [(f0_a, (B, Fa), 'float32'), (f0_b, (B, Fb), 'float32'), (path, None if path is None else (B, P, 2), 'int32')],
                          lambda new: (new((6, B)),),
                          lambda ins, outs, where: (ins[0], ins[1], B, Fa, Fb, la, lb, ins[2], P, float(gross_cents), outs[0], *where),
                          stream, device=any(_is_torch_cuda(x) for x in (f0_a, f0_b, path)), twin=False)[0]

    def set_decoder_mode(self, mode: str) -> None:
        """How the autoregressive decoder loop runs: 'auto' (default: the persistent weight-stationary kernel for 1 - 2 rows,
        the fused two-kernel step for 3 - 8 rows, whichever applies otherwise), 'persistent' / 'fused' (that machine when the
        call shape allows it) or 'graph' (always one hipGraph of 7 kernels per step, the fallback of the other two)."""
        modes = {'graph': 0, 'persistent': 1, 'fused': 2, 'auto': 3}
        if mode not in modes:
            raise ValueError(f'mode must be one of {tuple(modes)}, got {mode!r}')
        self._check(self._lib.tts_hip_set_decoder_mode(self._h, modes[mode]), 'set_decoder_mode')

    @property
    def last_decoder_mode(self) -> str:
        """How the last `tacotron2_infer` call ran its loop: 'fused', 'persistent', 'graph', or 'none' before the first call."""
        return {2: 'fused', 1: 'persistent', 0: 'graph'}.get(self._lib.tts_hip_last_decoder_mode(self._h), 'none')

    def tacotron2_probe_encoder(self, tokens, speaker=None, what: str = 'memory'):
        """Test hook (tts_hip_tacotron2_probe_encoder): run the encoder of `tacotron2_infer` on tokens [B, Tin] up to a stop
        point and return what it computed there: what='conv1' / 'conv2' / 'conv3' an encoder conv's output [B, Tin, 512]
        (padded positions stored as 0), 'memory' [B, Tin, enc], 'processed_memory' [B, Tin, 128]."""
        whats = {'conv1': 0, 'conv2': 1, 'conv3': 2, 'memory': 3, 'processed_memory': 4}
        if what not in whats:
            raise ValueError(f'what must be one of {tuple(whats)}, got {what!r}')
        B, Tin = self._token_dims(tokens)
        width = 512 if whats[what] <= 2 else 128 if what == 'processed_memory' else 512 + (0 if speaker is None else _dims(speaker)[1])
        return self._call('tacotron2_probe_encoder', [(tokens, None, 'int32'), (speaker, None, 'float32')],
                          lambda new: (new((B, Tin, width)),),
                          lambda ins, outs, where: (ins[0], B, Tin, ins[1], whats[what], outs[0]))[0]

    def tacotron2_probe_postnet(self, frames, lengths, what: str = 'mel'):
        """Test hook (tts_hip_tacotron2_probe_postnet): run the postnet of `tacotron2_infer` on frames [B, T, 80] in place of
        the decoder output, masked as after a loop that produced `lengths` [B] (t <= lengths[b]), up to a stop point:
        what='conv1' .. 'conv4' [B, T, 512] (masked positions stored as 0), 'conv5' (the residual) [B, T, 80], 'mel'
        frames + residual [B, T, 80]."""
        whats = {'conv1': 0, 'conv2': 1, 'conv3': 2, 'conv4': 3, 'conv5': 4, 'mel': 5}
        if what not in whats:
            raise ValueError(f'what must be one of {tuple(whats)}, got {what!r}')
        shape = _dims(frames)
        if len(shape) != 3 or shape[2] != 80:
            raise ValueError(f'frames must be [B, T, 80], got {shape}')
        B, T = shape[:2]
        lens = self._row_table(lengths, B, *_INT32, '', 'lengths')
        return self._call('tacotron2_probe_postnet', [(frames, None, 'float32')],
                          lambda new: (new((B, T, 512 if whats[what] <= 3 else 80)),),
                          lambda ins, outs, where: (ins[0], B, T, lens, whats[what], outs[0]))[0]

    def tacotron2_postnet(self, frames, lengths):
        """Postnet + residual of `tacotron2_infer` on decoder frames [B, T, 80] whose rows end at index lengths[b] (mask
        t <= lengths[b]) -> mel [B, T, 80].  `predict(batch_backlog=...)` uses it for a row of a token batch that is cut at the
        frame cap it would have had alone: the batch's own postnet saw the frames behind the cut."""
        return self.tacotron2_probe_postnet(frames, lengths, what='mel')

    @property
    def last_conv_paths(self) -> int:
        """Bitmask of how each k = 5 conv last ran on this handle (tts_hip_last_conv_paths): bit i set = single pass, clear =
        split per tap; bits 0 - 2 encoder convs 1 - 3, bits 3 - 7 postnet convs 1 - 5; -1 before the first conv."""
        return int(self._lib.tts_hip_last_conv_paths(self._h))

    # ------------------------------------------------------------------ audio calls on rows
    def _audio_rows(self, audio, lengths, what):
        """(B, N, int32 lengths or None) of a [N] / [B, N] input; every length in [1, N].  Raises before any GPU call."""
        shape = self._batched(audio, 2)
        if shape is None:
            raise ValueError(f'{what}: audio must be [N] or [B, N], got shape {_dims(audio)}')
        B, N = shape
        if B < 1 or N < 1:
            raise ValueError(f'{what}: empty audio {_dims(audio)}')
        return B, N, None if lengths is None else self._row_table(lengths, B, 1, N, what, 'lengths')

    def _audio_call(self, name, audio, B, N, make_outputs, args, stream=None, extra=()):
        """`_call` for an entry point that begins (handle, audio [B, N], B, N, ...): `args(extras, outs)` returns the rest."""
        return self._call(name, [(audio, (B, N), 'float32'), *extra], make_outputs,
                          lambda ins, outs, where: (ins[0], B, N, *args(ins[1:], outs)), stream)

    # ------------------------------------------------------------------ mel-STFT
    def mel_stft(self, audio, stream=None):
        """audio [N] or [B, N] -> mel [B, N // 256 + 1, 80] (the reference's TacotronSTFT()(audio)).  `stream` (torch.cuda.Stream,
        device tensors only): enqueue there and return without waiting."""
        if _is_torch_cuda(audio):
            torch = self._torch()
            self._check_device(audio)
            a = audio if audio.dim() > 1 else audio[None]
            if a.shape[1] < 1024:
                a = torch.nn.functional.pad(a, (0, 1024 - a.shape[1]))
        else:
            a = np.asarray(audio, dtype=np.float32)
            if a.ndim == 1:
                a = a[None]
            if a.shape[1] < 1024:                     # MelSTFT.__call__ pads short audio (utils/audio/stft.py:113-115)
                a = np.pad(a, [(0, 0), (0, 1024 - a.shape[1])])
        B, N = int(a.shape[0]), int(a.shape[1])
        return self._audio_call('mel_stft', a, B, N, lambda new: (new((B, N // 256 + 1, 80)),), lambda extras, outs: (outs[0],), stream)[0]

    _STFT_STAGES = {'padded': 0, 'spectrum': 1, 'magnitude': 2, 'mel_linear': 3}

    def mel_stft_probe(self, audio, what: str = 'spectrum'):
        """Test hook (tts_hip_mel_stft_probe): run `mel_stft` on audio [N] or [B, N] (host array, N >= 1024: no short-audio
        pad here) up to a stage and return what it computed there, with F = N // 256 + 1: what='padded' the reflect-padded
        rows [B, N + 1024], 'spectrum' [B, F, 1026] (real parts of bins 0 .. 512, then the imaginary parts), 'magnitude'
        [B, F, 513], 'mel_linear' [B, F, 80] (before log(max(., 1e-5)))."""
        if what not in self._STFT_STAGES:
            raise ValueError(f'what must be one of {tuple(self._STFT_STAGES)}, got {what!r}')
        shape = self._batched(audio, 2)
        if shape is None:
            raise ValueError(f'audio must be [N] or [B, N], got {_dims(audio)}')
        B, N = shape
        F = N // 256 + 1
        shape = {'padded': (B, N + 1024), 'spectrum': (B, F, 1026), 'magnitude': (B, F, 513), 'mel_linear': (B, F, 80)}[what]
        return self._audio_call('mel_stft_probe', audio, B, N, lambda new: (new(shape),),
                               lambda extras, outs: (self._STFT_STAGES[what], outs[0]))[0]

    # ------------------------------------------------------------------ mel plans (any TacotronSTFT configuration, WhisperSTFT)
    _MEL_KINDS = {'tacotron': 0, 'whisper': 1}
    _MEL_NORMS = {None: 0, 'per_feature': 1, 'all_feature': 2}
    _MEL_FN_STAGES = {'padded': 0, 'spectrum': 1, 'magnitude': 2, 'mel_linear': 3, 'mel_log': 4}

    def mel_fn(self, config, window=None):
        """A mel plan (tts_hip_mel_fn_create) for `config` -- a mapping with sampling_rate, n_mel_channels, filter_length,
        hop_length, win_length, mel_fmin, mel_fmax, and optionally kind ('tacotron' | 'whisper'), normalize_mode (None |
        'per_feature' | 'all_feature') and pre_emph -- and `window` (float64 [win_length], None = periodic Hann).  Plans are
        cached by value: the same configuration returns the same `MelFn`.  They live until the engine closes."""
        cfg = dict(config)
        kind, norm = cfg.get('kind', 'tacotron'), cfg.get('normalize_mode')
        if kind not in self._MEL_KINDS or norm not in self._MEL_NORMS:
            raise ValueError(f'mel_fn: kind must be one of {tuple(self._MEL_KINDS)} and normalize_mode one of '
                             f'{tuple(self._MEL_NORMS)}, got {kind!r}, {norm!r}')
        c = MelConfigC(self._MEL_KINDS[kind], int(cfg['sampling_rate']), int(cfg['n_mel_channels']), int(cfg['filter_length']),
                       int(cfg['hop_length']), int(cfg['win_length']), self._MEL_NORMS[norm], float(cfg['mel_fmin']),
                       float(cfg['mel_fmax']), float(cfg.get('pre_emph') or 0.0))
        w = None
        if window is not None:
            w = np.ascontiguousarray(window, dtype=np.float64)
            if w.shape != (c.win_length,):
                raise ValueError(f'mel_fn: window must be [win_length = {c.win_length}], got {w.shape}')
        key = (bytes(c), None if w is None else w.tobytes())
        cache = self.__dict__.setdefault('_mel_fns', {})
        if key not in cache:
            h = ctypes.c_void_p()
            self._check(self._lib.tts_hip_mel_fn_create(self._h, ctypes.byref(c), self._ptr(w), ctypes.byref(h)), 'mel_fn_create')
            cache[key] = MelFn(h, c)
        return cache[key]

    def mel_fn_frames(self, plan, n_samples):
        """Frames a row of `n_samples` yields under `plan`; raises when the plan refuses such a row."""
        f = self._lib.tts_hip_mel_fn_frames(plan.handle, int(n_samples))
        if f < 0:
            raise ValueError(f'mel_fn: a row of {n_samples} samples is refused by this plan')
        return f

    def mel_fn_run(self, plan, audio, lengths=None, stream=None):
        """audio [N] or [B, N] -> mel [B, F, n_mel] under `plan` (`mel_fn`), F = mel_fn_frames(plan, N).  Row b holds
        lengths[b] samples (default N): its frames are what a one-row call on audio[b, :lengths[b]] gives, zero beyond, and
        nothing behind its length is read.  numpy in -> numpy out; a CUDA tensor in -> a CUDA tensor out; `stream`
        (torch.cuda.Stream, device tensors only): enqueue there and return without waiting (the plans of an engine share
        one workspace: the next mel call must be ordered after it)."""
        B, N, lens = self._audio_rows(audio, lengths, 'mel_fn_run')
        F = self.mel_fn_frames(plan, N)
        return self._audio_call('mel_fn_run', audio, B, N, lambda new: (new((B, F, plan.n_mel)),),
                               lambda extras, outs: (lens, plan.handle, outs[0]), stream)[0]

    def mel_fn_probe(self, plan, audio, what: str = 'spectrum', lengths=None):
        """Test hook (tts_hip_mel_fn_probe): run `mel_fn_run` on the same arguments (host arrays) up to a stage and return
        what it computed there, with Fr the DFT frames of N (Whisper's last one included), P = max(N, win_length) +
        2 * (filter_length // 2) and C = filter_length // 2 + 1: 'padded' [B, P] after the zero pad, the pre-emphasis and
        the reflect pad; 'spectrum' [B, Fr, 2 C]; 'magnitude' [B, Fr, C]; 'mel_linear' [B, Fr, n_mel]; 'mel_log'
        [B, F, n_mel] after the logarithm, before the normalisation / clamp."""
        if what not in self._MEL_FN_STAGES:
            raise ValueError(f'what must be one of {tuple(self._MEL_FN_STAGES)}, got {what!r}')
        B, N, lens = self._audio_rows(audio, lengths, 'mel_fn_probe')
        F = self.mel_fn_frames(plan, N)
        g = plan.geometry
        Fr = F + (1 if g['kind'] == 1 else 0)
        C = g['filter_length'] // 2 + 1
        shape = {'padded': (B, max(N, g['win_length']) + 2 * (g['filter_length'] // 2)), 'spectrum': (B, Fr, 2 * C),
                 'magnitude': (B, Fr, C), 'mel_linear': (B, Fr, plan.n_mel), 'mel_log': (B, F, plan.n_mel)}[what]
        return self._audio_call('mel_fn_probe', audio, B, N, lambda new: (new(shape),),
                               lambda extras, outs: (lens, plan.handle, self._MEL_FN_STAGES[what], outs[0]))[0]

    # ------------------------------------------------------------------ STFT with phase, inverse, Griffin-Lim (csrc/stft_inv.hip)
    def mel_fn_samples(self, plan, frames):
        """Samples `frames` frames overlap-add to under `plan`: hop * (frames - 1) + filter_length - 2 * (filter_length // 2)."""
        n = self._lib.tts_hip_mel_fn_samples(plan.handle, int(frames))
        if n < 0:
            raise ValueError(f'mel_fn_samples: frames = {frames} < 1')
        return int(n)

    def stft_transform(self, plan, audio, lengths=None, polar=True):
        """audio [N] or [B, N] -> two planes [B, F, filter_length // 2 + 1] under `plan` (Tacotron kind), F =
        mel_fn_frames(plan, N): (magnitude, phase), or with polar=False (real, imaginary) -- the reference's STFT.transform on
        the plan's padding and window.  Frames at and beyond a row's own (`lengths`) are 0.  numpy in -> numpy out, a CUDA
        tensor in -> CUDA tensors out."""
        B, N, lens = self._audio_rows(audio, lengths, 'stft_transform')
        F = self.mel_fn_frames(plan, N)
        C = plan.geometry['filter_length'] // 2 + 1
        return self._audio_call('stft_transform', audio, B, N, lambda new: (new((B, F, C)), new((B, F, C))),
                               lambda extras, outs: (lens, plan.handle, 0 if polar else 1, outs[0], outs[1]))

    def _planes(self, x, frames, what, name):
        """(B, F, C, int32 frame counts in [1, F] or None) of `x`, [F, C] or [B, F, C]."""
        shape = self._batched(x, 3)
        if shape is None:
            raise ValueError(f'{what}: {name} must be [F, C] or [B, F, C], got {_dims(x)}')
        B, F, C = shape
        return B, F, C, None if frames is None else self._row_table(frames, B, 1, F, what, 'frames')

    def stft_inverse(self, plan, plane0, plane1, frames=None, polar=True):
        """Two planes [F, C] or [B, F, C] (C = filter_length // 2 + 1; magnitude and phase, or with polar=False real and imaginary
        parts) -> audio [B, F * hop_length]: row b holds mel_fn_samples(plan, frames[b]) samples (default F frames), zeros
        beyond; nothing behind a row's frames is read."""
        if _dims(plane1) != _dims(plane0):
            raise ValueError(f'stft_inverse: planes must both be [F, C] or [B, F, C], got {_dims(plane0)} and {_dims(plane1)}')
        B, F, C, fr = self._planes(plane0, frames, 'stft_inverse', 'planes')
        if C != plan.geometry['filter_length'] // 2 + 1:
            raise ValueError(f"stft_inverse: {C} bins, the plan has {plan.geometry['filter_length'] // 2 + 1}")
        return self._call('stft_inverse', [(plane0, (B, F, C), 'float32'), (plane1, (B, F, C), 'float32')],
                          lambda new: (new((B, F * plan.geometry['hop_length'])),),
                          lambda ins, outs, where: (ins[0], B, F, ins[1], fr, plan.handle, 0 if polar else 1, outs[0]))[0]

    _GL_KINDS = {'magnitude': 0, 'log_mel': 1}
    _GL_STAGES = {'target': 0, 'operand': 1, 'frames': 2, 'signal': 3, 'spectrum': 4, 'phasor': 5}

    def _griffin_lim(self, name, plan, spec, frames, kind, n_iters, momentum, init, mel_inverse, shape, tail=(), stream=None):
        """tts_hip_griffin_lim or its probe (`tail`: the probe's iteration and stage) -> one output of `shape(B, F, bins)`."""
        if kind not in self._GL_KINDS:
            raise ValueError(f'{name}: kind must be one of {tuple(self._GL_KINDS)}, got {kind!r}')
        B, F, C, fr = self._planes(spec, frames, name, 'spec')
        bins = plan.geometry['filter_length'] // 2 + 1
        minv = None
        if mel_inverse is not None:
            minv = np.ascontiguousarray(mel_inverse, dtype=np.float64)
            if kind != 'log_mel' or minv.shape != (plan.n_mel, bins):
                raise ValueError(f"{name}: mel_inverse goes with kind='log_mel' and must be [{plan.n_mel}, {bins}]")
        return self._call(name, [(spec, (B, F, C), 'float32'), (init, (B, F, bins, 2), 'float32')], lambda new: (new(shape(B, F, bins)),),
                          lambda ins, outs, where: (ins[0], B, F, C, fr, plan.handle, self._GL_KINDS[kind], minv, ins[1], int(n_iters),
                                                    float(momentum), *tail, outs[0]), stream)[0]

    def griffin_lim(self, plan, spec, frames=None, kind='magnitude', n_iters=60, momentum=0.99, init=None, mel_inverse=None,
                    stream=None):
        """Griffin-Lim phase reconstruction (tts_hip_griffin_lim) under `plan`: spec [F, C] or [B, F, C] -> audio
        [B, F * hop_length].  kind='magnitude': C = filter_length // 2 + 1 linear magnitudes; 'log_mel': C = n_mel log-mels,
        turned into magnitudes by max(0, exp(spec) . mel_inverse) (`mel_inverse` float64 [n_mel, bins]; None: the minimum-norm
        inverse of the plan's filterbank).  `init` [B, F, bins, 2]: the initial phase as (re, im) pairs of any length (None:
        zero phase).  Row b holds `frames[b]` frames (default F).  `stream` as `mel_fn_run`."""
        return self._griffin_lim('griffin_lim', plan, spec, frames, kind, n_iters, momentum, init, mel_inverse,
                                 lambda B, F, bins: (B, F * plan.geometry['hop_length']), stream=stream)

    def griffin_lim_probe(self, plan, spec, k, what, frames=None, kind='magnitude', n_iters=3, momentum=0.99, init=None,
                          mel_inverse=None):
        """Test hook (tts_hip_griffin_lim_probe): run `griffin_lim` on the same arguments (host arrays) up to stage `what` of
        iteration k and return it: 'target' [B, F, bins]; 'operand', 'spectrum', 'phasor' [B, F, 2 bins] (real parts, then
        imaginary parts); 'frames' [B, F, filter_length]; 'signal' [B, hop * (F - 1) + filter_length] (the reflect-padded row)."""
        if what not in self._GL_STAGES:
            raise ValueError(f'what must be one of {tuple(self._GL_STAGES)}, got {what!r}')
        g = plan.geometry
        return self._griffin_lim('griffin_lim_probe', plan, spec, frames, kind, n_iters, momentum, init, mel_inverse,
                                 lambda B, F, bins: {'target': (B, F, bins), 'frames': (B, F, g['filter_length']),
                                                     'signal': (B, g['hop_length'] * (F - 1) + g['filter_length'])
                                                     }.get(what, (B, F, 2 * bins)), tail=(int(k), self._GL_STAGES[what]))

    # ------------------------------------------------------------------ WaveGlow denoiser (csrc/stft_inv.hip)
    _DN_STAGES = {'spectrum': 0, 'operand': 1, 'frames': 2}

    def _bias(self, plan, bias, what):
        """(bias, [bins], dtype) as `_call` takes an input; the bias must hold one magnitude per bin of the plan."""
        bins = plan.geometry['filter_length'] // 2 + 1
        if _dims(bias) != (bins,):
            raise ValueError(f'{what}: bias must be [{bins}] (one magnitude per bin of the plan), got {_dims(bias)}')
        return bias, (bins,), 'float32'

    def denoise(self, plan, audio, bias, strength=0.1, lengths=None, stream=None, out=None):
        """Spectral subtraction of a vocoder's bias spectrum (tts_hip_denoise) under `plan` (Tacotron kind): audio [N] or
        [B, N] -> [B, N], every bin's magnitude lowered by strength * bias[c] and clamped at 0, its phase kept, then the
        plan's inverse.  Row b holds lengths[b] samples (default N) and gets back min(lengths[b], mel_fn_samples(plan,
        mel_fn_frames(plan, lengths[b]))) of them, zeros beyond; nothing behind its length is read.  numpy in -> numpy out; a
        CUDA tensor in -> a CUDA tensor out; `stream` (torch.cuda.Stream, device tensors only): tts_hip_denoise_async is
        enqueued there and the call returns without waiting.  `out` (device tensors only): a contiguous float32 CUDA tensor
        [B, N] that takes the result; it may be `audio` itself."""
        B, N, lens = self._audio_rows(audio, lengths, 'denoise')
        bias = self._bias(plan, bias, 'denoise')
        if out is not None and not (_is_torch_cuda(audio) and _is_torch_cuda(out) and out.dtype == self._torch().float32
                                    and out.is_contiguous() and _dims(out) == (B, N)):
            raise ValueError(f'denoise: out must be a contiguous float32 CUDA tensor [{B}, {N}] next to a CUDA input')
        return self._audio_call('denoise', audio, B, N, lambda new: (new((B, N)) if out is None else out,),
                               lambda extras, outs: (lens, plan.handle, extras[0], float(strength), outs[0]), stream, [bias])[0]

    def denoise_probe(self, plan, audio, bias, strength, what, lengths=None):
        """Test hook (tts_hip_denoise_probe): run `denoise` on the same arguments (host arrays) up to stage `what` and return
        it, with F = mel_fn_frames(plan, N): 'spectrum' and 'operand' [B, F, 2 bins] (real parts, then imaginary parts),
        'frames' [B, F, filter_length]."""
        if what not in self._DN_STAGES:
            raise ValueError(f'what must be one of {tuple(self._DN_STAGES)}, got {what!r}')
        B, N, lens = self._audio_rows(audio, lengths, 'denoise_probe')
        bias = self._bias(plan, bias, 'denoise_probe')
        F = self.mel_fn_frames(plan, N)
        shape = (B, F, plan.geometry['filter_length']) if what == 'frames' else (B, F, 2 * bias[1][0])
        return self._audio_call('denoise_probe', audio, B, N, lambda new: (new(shape),),
                               lambda extras, outs: (lens, plan.handle, extras[0], float(strength), self._DN_STAGES[what], outs[0]),
                               extra=[bias])[0]

    # ------------------------------------------------------------------ time stretch (csrc/stft_inv.hip)
    _TS_STAGES = {'spectrum': 0, 'magnitude': 1, 'owner': 2, 'operand': 3, 'frames': 4}
    TIME_STRETCH_RATES = (0.25, 4.0)

    def _stretch_rows(self, plan, audio, rate, lengths, what):
        """(B, N, lengths or None, float64 rates [B], int32 samples out [B], frames out [B]) of a time-stretch call; `rate` a
        scalar or one value per row.  Raises before any GPU call."""
        B, N, lens = self._audio_rows(audio, lengths, what)
        rates = np.asarray(rate.detach().cpu().numpy() if hasattr(rate, 'detach') else rate, dtype=np.float64)
        if rates.ndim == 0:
            rates = np.full(B, float(rates))
        if rates.shape != (B,):
            raise ValueError(f'{what}: rate must be a scalar or hold one value per row, shape ({B},), got {rates.shape}')
        lo, hi = self.TIME_STRETCH_RATES
        if not (np.isfinite(rates).all() and (rates >= lo).all() and (rates <= hi).all()):
            raise ValueError(f'{what}: rate must be finite and lie in [{lo}, {hi}], got {rates.tolist()}')
        rates = np.ascontiguousarray(rates)
        each = [N] * B if lens is None else lens.tolist()
        samples = [self._lib.tts_hip_time_stretch_samples(plan.handle, int(n), float(r)) for n, r in zip(each, rates)]
        frames = [self._lib.tts_hip_time_stretch_frames(plan.handle, int(n), float(r)) for n, r in zip(each, rates)]
        if min(samples) < 0 or min(frames) < 0:
            raise ValueError(f'{what}: this plan refuses a row (rows of {each} samples; a Whisper plan, pre_emph > 0 or a row '
                             'the reflect padding cannot pad)')
        if max(samples) < 1:
            raise ValueError(f'{what}: rows of {each} samples at rates {rates.tolist()} stretch to 0 samples')
        return B, N, lens, rates, np.asarray(samples, np.int32), frames

    def time_stretch(self, plan, audio, rate, lengths=None, stream=None):
        """Change the tempo of audio [N] or [B, N] without changing its pitch (tts_hip_time_stretch): a phase vocoder with
        identity phase locking under `plan` (Tacotron kind, no pre-emphasis).  `rate` (a scalar or one value per row, in
        [0.25, 4]): 2 plays twice as fast.  Row b holds lengths[b] samples (default N).  Returns (out, out_lengths): out
        [B, max(out_lengths)] ([M] for a one-row [N] input), row b holding out_lengths[b] = round(lengths[b] / rate[b])
        samples and zeros beyond; out_lengths is a host int32 array [B].  numpy in -> numpy out; a CUDA tensor in -> a CUDA
        tensor out; `stream` (torch.cuda.Stream, device tensors only): tts_hip_time_stretch_async is enqueued there and the
        call returns without waiting."""
        B, N, lens, rates, samples, _ = self._stretch_rows(plan, audio, rate, lengths, 'time_stretch')
        M = int(samples.max())
        out, = self._audio_call('time_stretch', audio, B, N, lambda new: (new((B, M)),),
                                lambda extras, outs: (lens, rates, plan.handle, outs[0], M), stream)
        return (out[0] if len(_dims(audio)) == 1 else out), samples

    def time_stretch_probe(self, plan, audio, rate, what, lengths=None):
        """Test hook (tts_hip_time_stretch_probe): run `time_stretch` on the same arguments (host arrays) up to stage `what`
        and return it, with F = mel_fn_frames(plan, N) and T the most output frames of any row: 'spectrum' [B, F, 2 bins]
        (real parts, then imaginary parts); 'magnitude' m [B, T, bins]; 'owner' [B, T, bins] as float32, -1 where a frame has
        no peak; 'operand' Y [B, T, 2 bins]; 'frames' [B, T, filter_length]."""
        if what not in self._TS_STAGES:
            raise ValueError(f'what must be one of {tuple(self._TS_STAGES)}, got {what!r}')
        B, N, lens, rates, samples, frames = self._stretch_rows(plan, audio, rate, lengths, 'time_stretch_probe')
        bins, T = plan.geometry['filter_length'] // 2 + 1, max(frames)
        shape = {'spectrum': (B, self.mel_fn_frames(plan, N), 2 * bins), 'magnitude': (B, T, bins), 'owner': (B, T, bins),
                 'operand': (B, T, 2 * bins), 'frames': (B, T, plan.geometry['filter_length'])}[what]
        return self._audio_call('time_stretch_probe', audio, B, N, lambda new: (new(shape),),
                                lambda extras, outs: (lens, rates, plan.handle, self._TS_STAGES[what], outs[0],
                                                      int(samples.max())))[0]

    # ------------------------------------------------------------------ formant match (csrc/stft_inv.hip)
    _FM_STAGES = {'logmag': 0, 'envelope': 1, 'gain': 2, 'operand': 3, 'frames': 4}
    FORMANT_WARPS = (0.5, 2.0)
    FORMANT_MAX_GAIN_DB = 60.0

    @staticmethod
    def default_lifter(plan):
        """The lifter cut used when none is given: max(1, round(0.0015 * sampling_rate)) -- 1.5 ms, 33 at 22 050 Hz, below the
        period of a 600 Hz voice -- clipped to [1, filter_length // 2 - 1]."""
        g = plan.geometry
        return int(min(max(1, int(round(0.0015 * g['sampling_rate']))), max(1, g['filter_length'] // 2 - 1)))

    def _formant_rows(self, plan, audio, source, warp, lifter, max_gain_db, lengths, what):
        """(B, N, lengths or None, the source as `_call` takes an input, float64 warps [B], Q, max_gain_db) of a formant-match
        call; `warp` a scalar or one value per row.  Raises before any GPU call."""
        B, N, lens = self._audio_rows(audio, lengths, what)
        if source is not None and self._batched(source, 2) != (B, N):
            raise ValueError(f'{what}: source must have the shape of audio, [{B}, {N}] (or [{N}]), got {_dims(source)}')
        warps = np.asarray(warp.detach().cpu().numpy() if hasattr(warp, 'detach') else warp, dtype=np.float64)
        if warps.ndim == 0:
            warps = np.full(B, float(warps))
        if warps.shape != (B,):
            raise ValueError(f'{what}: warp must be a scalar or hold one value per row, shape ({B},), got {warps.shape}')
        lo, hi = self.FORMANT_WARPS
        if not (np.isfinite(warps).all() and (warps >= lo).all() and (warps <= hi).all()):
            raise ValueError(f'{what}: warp must be finite and lie in [{lo}, {hi}], got {warps.tolist()}')
        top = plan.geometry['filter_length'] // 2 - 1
        Q = self.default_lifter(plan) if lifter is None else lifter
        if int(Q) != Q or not 1 <= int(Q) <= top:
            raise ValueError(f'{what}: lifter must be an integer in [1, filter_length // 2 - 1 = {top}], got {lifter!r}')
        if not (np.isfinite(max_gain_db) and 0 < max_gain_db <= self.FORMANT_MAX_GAIN_DB):
            raise ValueError(f'{what}: max_gain_db must lie in (0, {self.FORMANT_MAX_GAIN_DB:g}], got {max_gain_db!r}')
        return B, N, lens, (source, (B, N), 'float32'), np.ascontiguousarray(warps), int(Q), float(max_gain_db)

    def formant_match(self, plan, audio, source=None, *, warp=1.0, lifter=None, max_gain_db=24.0, lengths=None, stream=None):
        """Give audio [N] or [B, N] the spectral envelope of `source` (same shape; None: the audio itself) and keep its own
        phases and pitch (tts_hip_formant_match) under `plan` (Tacotron kind, no pre-emphasis): both signals' log-magnitude
        spectra are smoothed by cepstral liftering (quefrencies up to `lifter`; None: `default_lifter(plan)`), the audio's
        spectrum is multiplied by exp of their difference, clamped to +-`max_gain_db` and scaled so that every frame keeps
        its energy, then the plan's inverse.  `warp` (a scalar or one value per row, in [0.5, 2]) reads the source envelope
        at k / warp: above 1 the formants move up.  Row b holds lengths[b] samples (default N) in both signals and gets back
        what `denoise` gives a row, zeros beyond.  numpy in -> numpy out; a CUDA tensor in -> a CUDA tensor out; `stream`
        (torch.cuda.Stream, device tensors only): tts_hip_formant_match_async is enqueued there and the call returns without
        waiting."""
        B, N, lens, src, warps, Q, db = self._formant_rows(plan, audio, source, warp, lifter, max_gain_db, lengths, 'formant_match')
        return self._call('formant_match', [(audio, (B, N), 'float32'), src], lambda new: (new((B, N)),),
                          lambda ins, outs, where: (ins[0], ins[1], B, N, lens, plan.handle, warps, Q, db, outs[0]), stream)[0]

    def formant_match_probe(self, plan, audio, source, what, *, warp=1.0, lifter=None, max_gain_db=24.0, lengths=None):
        """Test hook (tts_hip_formant_match_probe): run `formant_match` on the same arguments (host arrays) up to stage `what`
        and return it, with F = mel_fn_frames(plan, N): 'logmag' and 'envelope' [2, B, F, bins] (source, then audio); 'gain'
        [B, F, bins]; 'operand' [B, F, 2 bins] (real parts, then imaginary parts); 'frames' [B, F, filter_length]."""
        if what not in self._FM_STAGES:
            raise ValueError(f'what must be one of {tuple(self._FM_STAGES)}, got {what!r}')
        B, N, lens, src, warps, Q, db = self._formant_rows(plan, audio, source, warp, lifter, max_gain_db, lengths,
                                                           'formant_match_probe')
        bins, F = plan.geometry['filter_length'] // 2 + 1, self.mel_fn_frames(plan, N)
        shape = {'logmag': (2, B, F, bins), 'envelope': (2, B, F, bins), 'gain': (B, F, bins), 'operand': (B, F, 2 * bins),
                 'frames': (B, F, plan.geometry['filter_length'])}[what]
        return self._call('formant_match_probe', [(audio, (B, N), 'float32'), src], lambda new: (new(shape),),
                          lambda ins, outs, where: (ins[0], ins[1], B, N, lens, plan.handle, warps, Q, db, self._FM_STAGES[what],
                                                    outs[0]))[0]

    # ------------------------------------------------------------------ waveform clean-up (csrc/audio_proc.hip)
    _TRIM_MODES = {'start_end': 0, 'start': 1, 'end': 2}

    @staticmethod
    def _samples(value, rate, what):
        """seconds (float, times `rate`) or samples (int) -> samples, as the reference does (int(value * rate))."""
        if isinstance(value, (float, np.floating)):
            if rate is None:
                raise ValueError(f'{what} in seconds needs `rate`')
            return int(value * rate)
        return int(value)

    def reduce_noise(self, audio, rate=None, lengths=None, noise=None, noise_length=0.2, renormalize=False, stream=None):
        """Spectral-gating noise reduction (utils/audio/audio_processing.py:65-83 -> noisereducev1.py:175-290, v1 defaults).
        audio [N] or [B, N]; row b holds lengths[b] samples (default N) and its result is what a one-row call on
        audio[b, :lengths[b]] gives, zero beyond.  noise=None: each row's first `noise_length` (seconds with `rate`, or
        samples) samples are the noise clip; else noise [noise_len] / [B, noise_len].  renormalize: then
        normalize_audio(max_val=1.) per row, as load_audio does after reduce_noise.  numpy in -> numpy out; a CUDA tensor
        in -> a CUDA tensor out; `stream` (torch.cuda.Stream, device tensors only): enqueue there and return without waiting
        (the clean-up calls share one workspace per engine: the next reduce_noise / trim_silence must be ordered after it)."""
        B, N, lens = self._audio_rows(audio, lengths, 'reduce_noise')
        if noise is not None:
            if len(noise.shape) not in (1, 2) or (len(noise.shape) == 2 and int(noise.shape[0]) != B) or \
                    (len(noise.shape) == 1 and B != 1):
                raise ValueError(f'reduce_noise: noise must be [noise_len] (one row) or [{B}, noise_len], got {tuple(noise.shape)}')
            noise_len = int(noise.shape[-1])
        else:
            noise_len = self._samples(noise_length, rate, 'reduce_noise: noise_length')
        if noise_len < 1:
            raise ValueError(f'reduce_noise: the noise clip must hold at least one sample (got {noise_len})')
        out, = self._audio_call('reduce_noise', audio, B, N, lambda new: (new((B, N)),),
                               lambda extras, outs: (lens, extras[0], noise_len, int(bool(renormalize)), outs[0]),
                               stream, [(noise, (B, noise_len), 'float32')])
        return out[0] if len(audio.shape) == 1 else out

    _RN_STAGES = {'padded': 0, 'noise_padded': 1, 'spectrum': 2, 'noise_spectrum': 3, 'power_max': 4, 'threshold': 5, 'mask': 6,
                  'gated': 7, 'frames': 8}

    def reduce_noise_probe(self, audio, rate=None, lengths=None, noise=None, noise_length=0.2, what: str = 'spectrum'):
        """Test hook (tts_hip_reduce_noise_probe): run `reduce_noise` on the same arguments (host arrays) up to a stage and
        return what it computed there as float32, with Fr = ceil((N + 2560) / 512) frame slots per row and Frn =
        ceil((noise_len + 2048) / 512) noise frame slots: 'padded' [B, Fr * 512], 'noise_padded' [B, Frn * 512], 'spectrum'
        [B, Fr, 2050] (real parts of bins 0 .. 1024, then the imaginary parts; before the gate), 'noise_spectrum'
        [B, Frn, 2050], 'power_max' [2, B] (signal rows, then noise rows), 'threshold' [B, 1025] dB, 'mask' [B, Fr, 1025] as
        0 / 1, 'gated' [B, Fr, 2050], 'frames' [B, Fr, 2048] (inverse-DFT rows before the overlap-add).  Always batched."""
        if what not in self._RN_STAGES:
            raise ValueError(f'what must be one of {tuple(self._RN_STAGES)}, got {what!r}')
        B, N, lens = self._audio_rows(audio, lengths, 'reduce_noise_probe')
        if noise is not None:
            noise_len = int(np.asarray(noise).reshape(B, -1).shape[1])
        else:
            noise_len = self._samples(noise_length, rate, 'reduce_noise_probe: noise_length')
        if noise_len < 1:
            raise ValueError(f'reduce_noise_probe: the noise clip must hold at least one sample (got {noise_len})')
        Fr, Frn = -(-(N + 2560) // 512), -(-(noise_len + 2048) // 512)
        shape = {'padded': (B, Fr * 512), 'noise_padded': (B, Frn * 512), 'spectrum': (B, Fr, 2050),
                 'noise_spectrum': (B, Frn, 2050), 'power_max': (2, B), 'threshold': (B, 1025), 'mask': (B, Fr, 1025),
                 'gated': (B, Fr, 2050), 'frames': (B, Fr, 2048)}[what]
        return self._audio_call('reduce_noise_probe', audio, B, N, lambda new: (new(shape),),
                               lambda extras, outs: (lens, extras[0], noise_len, self._RN_STAGES[what], outs[0]),
                               extra=[(noise, (B, noise_len), 'float32')])[0]

    def trim_silence_probe(self, audio, rate=None, lengths=None, window_length=0.2):
        """Test hook (tts_hip_trim_silence_probe): the convolution launches of `trim_silence` on audio [N] or [B, N] (host
        array).  Returns conv [B, max(N, W) + 1] float64, W = 2 * (window_length // 2): conv[b, :nc_b] =
        np.convolve(x_b ** 2, window, 'valid') with nc_b = |lengths[b] - W| + 1, NaN beyond."""
        B, N, lens = self._audio_rows(audio, lengths, 'trim_silence_probe')
        wl = self._samples(window_length, rate, 'trim_silence_probe: window_length')
        if wl < 2:
            raise ValueError(f'trim_silence_probe: window_length must be >= 2 samples (got {wl})')
        W = 2 * (wl // 2)
        conv, = self._audio_call('trim_silence_probe', audio, B, N, lambda new: (new((B, max(N, W) + 1), 'float64'),),
                                lambda extras, outs: (lens, wl, outs[0]))
        for b in range(B):
            conv[b, abs((N if lens is None else int(lens[b])) - W) + 1:] = np.nan
        return conv

    _RESAMPLE_MAX = 1 << 24         # samples per row, in and out (csrc/resample.hip)

    def resample(self, audio, rate, target_rate, lengths=None, stream=None):
        """scipy.signal.resample(x, int(N / rate * target_rate)) per row (utils/audio/audio_processing.py:30-35), in fp32 on
        the GPU (csrc/resample.hip).  audio [N] or [B, N]; row b holds lengths[b] samples (default N) and its result is what
        a one-row call on audio[b, :lengths[b]] gives: resampled_length(lengths[b]) samples, then zeros up to
        M = resampled_length(N).  rate == target_rate returns the input as float32 and launches nothing.  numpy in -> numpy
        out; a CUDA tensor in -> a CUDA tensor out; `stream` (torch.cuda.Stream, device tensors only): enqueue there and
        return without waiting (the next resample on this engine must be ordered after it)."""
        from .audio import resampled_length
        B, N, lens = self._audio_rows(audio, lengths, 'resample')
        if int(rate) != rate or int(target_rate) != target_rate or rate <= 0 or target_rate <= 0:
            raise ValueError(f'resample: rates must be positive integers (got {rate}, {target_rate})')
        rate, target_rate = int(rate), int(target_rate)
        if N > self._RESAMPLE_MAX:
            raise ValueError(f'resample: rows of {N} samples; at most 2^24 are supported')
        M = resampled_length(N, rate, target_rate)          # raises for M < 1
        if M > self._RESAMPLE_MAX:
            raise ValueError(f'resample: {N} samples at {rate} -> {target_rate} Hz give {M}; at most 2^24 are supported')
        if lens is not None:
            for n in np.unique(lens):
                resampled_length(int(n), rate, target_rate)
        if B * max(N, M) * 4 >= 1 << 31:
            raise ValueError(f'resample: B = {B} x N = {N} (M {M}) too large for 31-bit offsets')
        one_row = len(audio.shape) == 1
        if rate == target_rate and lens is None:            # no library call: the input as float32
            if _is_torch_cuda(audio):
                self._check_device(audio)
                return audio.to(self._torch().float32)
            if stream is not None:
                raise ValueError('stream= needs device tensors')
            a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(B, N))
            return a[0] if one_row else a
        out, = self._audio_call('resample', audio, B, N, lambda new: (new((B, M)),),
                               lambda extras, outs: (lens, rate, target_rate, outs[0], M), stream)
        return out[0] if one_row else out

    def resample_probe(self, audio, rate, target_rate, lengths=None):
        """Test hook (tts_hip_resample_probe): run `resample` on the same arguments (host arrays, rate != target_rate) up to
        the end of the forward chain -> complex64 [B, N // 2 + 1]: row b holds bins 0 .. lengths[b] // 2 of
        rfft(audio[b, :lengths[b]]), zeros beyond.  Always batched."""
        from .audio import resampled_length
        B, N, lens = self._audio_rows(audio, lengths, 'resample_probe')
        M = resampled_length(N, int(rate), int(target_rate))
        out, = self._audio_call('resample_probe', audio, B, N, lambda new: (new((B, N // 2 + 1, 2)),),
                               lambda extras, outs: (lens, int(rate), int(target_rate), outs[0], M))
        return out.view(np.complex64)[..., 0]

    def resample_fft_probe(self, lines, inverse=False):
        """Test hook (tts_hip_resample_fft_probe): the complex fp32 FFT of the resampling chains on `lines` [n, 2^logL]
        (complex64, 6 <= logL <= 25) -> complex64 [n, 2^logL], unscaled.  Up to 2^13 points in natural order; above, the
        forward transform leaves bin k2 + L2 * k1 (L2 = 2^logL / 8192) at k2 * 8192 + k1 and the inverse takes that order
        and returns the natural one."""
        a = np.ascontiguousarray(lines, dtype=np.complex64)
        if a.ndim != 2 or a.shape[1] < 1 or a.shape[1] & (a.shape[1] - 1):
            raise ValueError(f'resample_fft_probe: lines must be [n, 2^logL], got {a.shape}')
        out = np.empty_like(a)
        self._check(self._lib.tts_hip_resample_fft_probe(self._h, self._ptr(a), int(a.shape[0]), int(a.shape[1]).bit_length() - 1,
                                                         int(bool(inverse)), self._ptr(out)), 'resample_fft_probe')
        return out

    def trim_silence(self, audio, rate=None, lengths=None, threshold=0.1, window_length=0.2, add_start=0, add_end=1.5,
                     mode='start_end'):
        """Window-method silence trimming (utils/audio/audio_processing.py:274-370: power 2, triangular window, adaptive
        thresholds, max_trim_factor 5).  audio [N] -> (start, end) ints; [B, N] -> (start, end) int32 arrays [B]; the
        trimmed row b is audio[b, start[b]:end[b]] (of its first lengths[b] samples).  `window_length` in seconds (float,
        with `rate`) or samples (int); `add_start` / `add_end` are margins in window lengths."""
        B, N, lens = self._audio_rows(audio, lengths, 'trim_silence')
        if mode not in self._TRIM_MODES:
            raise ValueError(f'trim_silence: invalid mode {mode!r} (start, end or start_end)')
        wl = self._samples(window_length, rate, 'trim_silence: window_length')
        if wl < 2:
            raise ValueError(f'trim_silence: window_length must be >= 2 samples (got {wl})')
        if not (np.isfinite(threshold) and np.isfinite(add_start) and np.isfinite(add_end)) or add_start < 0 or add_end < 0:
            raise ValueError('trim_silence: threshold and margins must be finite, margins >= 0')
        # one int32 [2, B] result (start row, end row): a CUDA input costs one device-to-host copy
        cuts, = self._audio_call('trim_silence', audio, B, N, lambda new: (new((2, B), 'int32'),),
                                lambda extras, outs: (lens, wl, float(threshold), float(add_start), float(add_end),
                                                      self._TRIM_MODES[mode], outs[0][0], outs[0][1]))
        start, end = cuts.cpu().numpy() if _is_torch_cuda(cuts) else cuts
        if len(audio.shape) == 1:
            return int(start[0]), int(end[0])
        return start, end

    # ------------------------------------------------------------------ silence removal (csrc/silence.hip)
    _SILENCE_METHODS = {'rms': 0, 'threshold': 1, 'remove': 2}
    _SILENCE_MODES = {'start_end': 0, 'start': 1, 'end': 2, 'remove': 3}
    _SILENCE_DEFAULTS = {'rms': (-25, 0.1), 'threshold': (0.1, 0.), 'remove': (0.025, 0.15)}    # threshold, min_silence
    _SILENCE_MAX = 1 << 24          # samples per row

    def _silence_call(self, who, audio, rate, lengths, method, mode, threshold, min_silence, block_size, replace_by,
                      min_voice_time):
        """(B, N, int32 lengths or None, the C arguments from `method` to `min_voice_time`) of a remove_silence[_probe] call;
        raises for what the C side refuses, before any GPU call."""
        B, N, lens = self._audio_rows(audio, lengths, who)
        if isinstance(method, bytes):
            method = method.decode()
        if isinstance(mode, bytes):
            mode = mode.decode()
        if method not in self._SILENCE_METHODS:
            raise ValueError(f'{who}: unknown method {method!r} (supported: {sorted(self._SILENCE_METHODS)})')
        if mode not in self._SILENCE_MODES:
            raise ValueError(f'{who}: invalid mode {mode!r} (start, end, start_end or remove)')
        if mode == 'remove' and method != 'rms':
            raise ValueError(f"{who}: mode 'remove' belongs to method 'rms' (got method {method!r})")
        if rate is None or int(rate) != rate or rate <= 0:
            raise ValueError(f'{who}: rate must be a positive integer (got {rate})')
        rate = int(rate)
        d_thr, d_sil = self._SILENCE_DEFAULTS[method]
        threshold = d_thr if threshold is None else threshold
        min_silence = d_sil if min_silence is None else min_silence
        bs = rb = 1
        if method == 'rms':
            bs = self._samples(block_size, rate, who + ': block_size')
            rb = self._samples(replace_by, rate, who + ': replace_by')
            if bs < 1:
                raise ValueError(f'{who}: block_size must be >= 1 sample (got {bs})')
            if not 0 <= rb < 1 << 31:
                raise ValueError(f'{who}: replace_by must be >= 0 samples (got {rb})')
            if not np.isfinite(min_voice_time) or min_voice_time < 0:
                raise ValueError(f'{who}: min_voice_time must be finite and >= 0 (got {min_voice_time})')
            bs = min(bs, 1 << 30)
        else:
            min_voice_time = 0.
        if not np.isfinite(threshold) or (method != 'rms' and threshold < 0):
            raise ValueError(f'{who}: threshold must be finite{"" if method == "rms" else " and >= 0"} (got {threshold})')
        if not np.isfinite(min_silence) or min_silence < 0:
            raise ValueError(f'{who}: min_silence must be finite and >= 0 (got {min_silence})')
        if method == 'remove':
            w = int(min_silence * rate)
            shortest = N if lens is None else int(lens.min())
            if threshold <= 0 or w < 1:
                raise ValueError(f'{who}: the mean-window method needs threshold > 0 and a window of w >= 1 samples '
                                 f'(got threshold {threshold}, w = {w})')
            if shortest < w:
                raise ValueError(f'{who}: a row of L = {shortest} samples is shorter than the window w = {w}')
        if B > 65535 or N > self._SILENCE_MAX or B * N * 4 >= 1 << 31:
            raise ValueError(f'{who}: B = {B} x N = {N} too large (B <= 65535, N <= 2^24, B * N * 4 < 2^31)')
        args = (self._SILENCE_METHODS[method], self._SILENCE_MODES[mode], rate, float(threshold), float(min_silence), bs, rb,
                float(min_voice_time))
        return B, N, lens, args

    def remove_silence(self, audio, rate, lengths=None, method='rms', mode='start_end', threshold=None, min_silence=None,
                       block_size=0.01, replace_by=0.5, min_voice_time=0.2, stream=None):
        """The reference's numpy trim methods (utils/audio/audio_processing.py), sample for sample, with the kept samples
        compacted on the GPU (csrc/silence.hip).  method 'rms' (:100-200; `threshold` in dB, default -25; `min_silence` 0.1 s;
        `block_size`, `replace_by`: seconds as floats, samples as ints; `min_voice_time` seconds, 0 disables the merging;
        mode start, end, start_end or remove, which also shortens the pauses inside), 'threshold' (:385-394; `threshold` an
        amplitude, default 0.1; mode start, end or start_end) or 'remove' (:372-383, the mean-window method; `threshold`
        0.025, `min_silence` 0.15 s; rows must hold at least int(min_silence * rate) samples).  threshold / min_silence None:
        the method's reference default.  A row in which the rms method finds no silence is returned unchanged (the reference
        raises IndexError in the three slice modes).  audio [N] (numpy) -> the kept samples, 1-D; [B, N] -> (out [B, N],
        out_lengths [B]): row b is the result of a one-row call on audio[b, :lengths[b]] (default N), then zeros.  A CUDA
        tensor in ([N] or [B, N]) -> CUDA tensors (out, int32 out_lengths) of the input's rank, without synchronization of
        the lengths; `stream` (torch.cuda.Stream, device tensors only): enqueue there and return without waiting (the
        clean-up calls share one workspace per engine: the next one must be ordered after it)."""
        B, N, lens, args = self._silence_call('remove_silence', audio, rate, lengths, method, mode, threshold, min_silence,
                                              block_size, replace_by, min_voice_time)
        out, out_len = self._audio_call('remove_silence', audio, B, N, lambda new: (new((B, N)), new((B,), 'int32')),
                                       lambda extras, outs: (lens, *args, outs[0], outs[1]), stream)
        if len(audio.shape) != 1:
            return out, out_len
        return (out[0], out_len[0]) if _is_torch_cuda(audio) else out[0, :int(out_len[0])].copy()

    _SILENCE_STAGES = {'flags': (0, 'uint8'), 'intervals': (1, 'int32'), 'mask': (2, 'uint8'), 'tile_offsets': (3, 'int32'),
                       'prefix': (4, 'float64')}

    def remove_silence_probe(self, audio, rate, what, lengths=None, method='rms', mode='start_end', threshold=None,
                             min_silence=None, block_size=0.01, replace_by=0.5, min_voice_time=0.2):
        """Test hook (tts_hip_remove_silence_probe): run `remove_silence` on the same arguments (host arrays) up to a stage
        and return its rows [B, width], the width being what the C side reports: 'flags' uint8 [B, NB] (rms; 1 = silent
        block), 'intervals' int32 [B, 2 + 2 * cap] (rms, threshold; n, cut, d0[cap], d1[cap]: the mask keeps t < cut outside
        every [d0[m], d1[m]), m < n), 'mask' uint8 [B, N], 'tile_offsets' int32 [B, NT] (kept samples before each tile of
        2048), 'prefix' float64 [B, N + 1] (mean-window; sums of the fp32 squares).  What lies behind a row's own extent
        (its blocks, its n intervals, its lengths[b] samples, its tiles) is unspecified.  Always batched."""
        if what not in self._SILENCE_STAGES:
            raise ValueError(f'what must be one of {tuple(self._SILENCE_STAGES)}, got {what!r}')
        stage, dtype = self._SILENCE_STAGES[what]
        B, N, lens, args = self._silence_call('remove_silence_probe', audio, rate, lengths, method, mode, threshold, min_silence,
                                              block_size, replace_by, min_voice_time)
        width = ctypes.c_int32(0)
        tail = lambda extras, outs: (lens, *args, stage, outs[0] if outs else None, ctypes.byref(width))
        self._audio_call('remove_silence_probe', audio, B, N, lambda new: (), tail)               # no output: the width alone
        return self._audio_call('remove_silence_probe', audio, B, N, lambda new: (new((B, width.value), dtype),), tail)[0]

    # ------------------------------------------------------------------ measurement hooks
    def kernel_timing(self, enable: bool) -> None:
        self._check(self._lib.tts_hip_kernel_timing(self._h, 1 if enable else 0), 'kernel_timing')

    def kernel_time_us(self, kind: int):
        avg = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        self._check(self._lib.tts_hip_kernel_time_us(self._h, int(kind), ctypes.byref(avg), ctypes.byref(n)),
                    'kernel_time_us')
        return avg.value, n.value

    def probe_mfma_f32(self):
        """(TFLOP/s, shader clock in GHz) of a bare fp32 MFMA loop on this device right now (tts_hip_probe_mfma_f32, ~60 ms)."""
        tf, ghz = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.tts_hip_probe_mfma_f32(self._h, ctypes.byref(tf), ctypes.byref(ghz)), 'probe_mfma_f32')
        return tf.value, ghz.value

    def synchronize(self) -> None:
        self._check(self._lib.tts_hip_synchronize(self._h), 'synchronize')
