"""Runtime plug-in for the reference's execution seam.

Mirrors /root/reference/utils/keras/runtimes/runtime.py:19-41 (`Runtime` ABC: per-path engine cache, abstract
`__call__` and `load_engine`) and utils/keras/runtimes/__init__.py:23-45 (`build_runtime` + `_runtimes` registry), so a
maintainer registers the backend with one line (`_runtimes['hip'] = HipRuntime`) and
`BaseModel(runtime='hip', ...)` (models/interfaces/base_model.py:139-209) hands every `compiled_infer` call
(base_model.py:367-375) to `HipRuntime.__call__`.

Call contracts honoured:
  Tacotron2  models/tts/tacotron2.py:162  compiled_infer(int32[1, Tin] | (tokens, float32[1, E]), max_length=10., **kw)
             -> object with .mel [B, Tmax, 80], .lengths [B], .attention_weights [B, Tmax, Tin] (+ the other fields of
             Tacotron2InferenceOutput, tacotron2_arch.py:52-56); unknown kwargs are ignored.
  WaveGlow   models/tts/waveglow.py:82-132 compiled_infer(float32[B, T, 80], **kw) -> float32[B, T*256];
             honours z / sigma / deterministic (waveglow_arch.py:244).
Randomness: like the reference (prenet dropout and z are sampled inside the graph, on the device:
tacotron2_arch.py:197-201, waveglow_arch.py:272-274,299-302) the default path draws both ON THE GPU -- the engine's
documented Philox4x32-10 stream (include/tts_hip.h, oracle/philox_ref.py), keyed by the runtime's seed and a running block
offset -- so no host-made tensor crosses PCIe.  The dropout bits and the noise are separate streams of one seed (key = seed
XOR a purpose constant in the high word: MASK_STREAM / NOISE_STREAM).  Explicit control stays: pass `prenet_masks` / `z`, or
`deterministic=True`, or `seed=` (that call then starts at offset 0 of that seed's streams and is reproducible).
Per-row streams (`streams=[...]`, one id per row): every row draws from its own stream, keyed by `stream_key(seed, purpose,
utterance, part, trial)` at offset 0, so a sentence's masks and noise do not depend on how it was batched.
"""
from __future__ import annotations

import os
import threading
from abc import ABCMeta, abstractmethod

import numpy as np

from .engine import HipEngine, Tacotron2InferenceOutput, _is_torch_cuda


# An explicit `seed=` names one stream per PURPOSE: the prenet dropout bits and the WaveGlow noise of the same seed must not be
# the same Philox blocks (both would start at offset 0 of one key and be correlated), so the purpose is XORed into the key's
# high word.  The engine-level calls (HipEngine.waveglow_infer(seed=...), tts_hip_random_fill) take the key as given.
MASK_STREAM = 0x4D41534B << 32          # "MASK"
NOISE_STREAM = 0x5A4E5345 << 32         # "ZNSE"
_U64 = (1 << 64) - 1


def rank_stream(seed: int, rank: int) -> int:
    """Key of rank `rank`'s stream under a job-wide seed: ranks synthesize different shards and must not draw identical noise."""
    return (int(seed) ^ (((int(rank) + 1) * 0x9E3779B97F4A7C15) & _U64)) & _U64 if rank else int(seed) & _U64


def _mix64(x: int) -> int:
    """splitmix64's output function of state x + golden gamma (Steele, Lea, Flood, OOPSLA'14): _mix64(0) is its first output."""
    x = (int(x) + 0x9E3779B97F4A7C15) & _U64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _U64
    return x ^ (x >> 31)


def stream_key(seed: int, purpose: int, utterance: int = 0, part: int = 0, trial: int = 0) -> int:
    """Philox key of ONE row's stream: derived from what the row is -- (seed, MASK_STREAM / NOISE_STREAM, utterance number,
    part of the text, retry) -- not from where it sits in a batch.  The stream always starts at offset 0."""
    k = _mix64((int(seed) ^ int(purpose)) & _U64)
    for v in (utterance, part, trial):
        k = _mix64(k ^ (int(v) & _U64))
    return k


def _row_ids(streams, B, width):
    """`streams` -> B tuples of `width` ints (a bare int is an utterance number; missing trailing fields are 0)."""
    ids = [tuple(int(v) for v in (s if isinstance(s, (tuple, list)) else (s,))) for s in streams]
    if len(ids) != B or any(not 1 <= len(i) <= width for i in ids):
        raise ValueError(f'streams must hold one id of at most {width} ints per row ({B} rows), got {streams!r}')
    return [i + (0,) * (width - len(i)) for i in ids]


def frame_cap(n_tok, max_length, default=None):
    """Frames the decoder may run for `n_tok` tokens (tacotron2_arch.py:886-897): a float `max_length` is frames per token
    (the reference's float32 product, truncated), an int is the count itself, None the `default`; never below 1."""
    if max_length is None:
        frames = default
    elif isinstance(max_length, float):
        frames = int(np.float32(n_tok) * np.float32(max_length))
    else:
        frames = int(max_length)
    return max(1, frames)


def mask_blocks(rows, frames):
    """Philox blocks (4 values each) behind the prenet dropout of `rows` x `frames` decoder steps: 2 layers x 256 units."""
    return (rows * frames * 512 + 3) // 4


def noise_blocks(rows, frames):
    """Philox blocks behind WaveGlow's noise for `rows` x `frames` mel frames: 256 samples per frame."""
    return (rows * frames * 256 + 3) // 4


# per purpose: (blocks one call draws, fields of a row's `streams` id, the keyword that holds explicit values)
_DRAWS = {MASK_STREAM: (mask_blocks, 3, 'prenet_masks'), NOISE_STREAM: (noise_blocks, 2, 'z')}


def _tokens_and_speaker(inputs):
    """`inputs` of a Tacotron2 call, tokens or (tokens, speaker) -> (tokens [B, Tin], speaker or None)."""
    if isinstance(inputs, (tuple, list)):
        tokens, speaker = inputs[0], (inputs[1] if len(inputs) > 1 else None)
    else:
        tokens, speaker = inputs, None
    if not _is_torch_cuda(tokens):
        tokens = np.asarray(tokens)
    if tokens.ndim == 1:
        tokens = tokens[None]
    return tokens, speaker


def sample_prenet_masks(rng, B, max_len):
    """Multiplicative prenet dropout masks [B, max_len, 2, 256] in {0, 2} (Bernoulli(0.5), scale 1 / (1 - 0.5):
    tacotron2_arch.py:188-203), drawn from the bits of `rng.integers(0, 256, uint8)` -- 6x cheaper on the host than
    thresholding `rng.random` floats (0.7 ms instead of 4.6 ms for a 1280-step budget), which matters because the reference
    keeps this dropout ON at inference, i.e. every `tts()` call samples them."""
    n = int(B) * int(max_len) * 2 * 256
    bits = rng.integers(0, 256, size=(n + 7) // 8, dtype=np.uint8)
    return (np.unpackbits(bits)[:n].reshape(B, max_len, 2, 256).astype(np.float32)) * np.float32(2.0)


class Runtime(metaclass=ABCMeta):
    """Plug-in interface of the reference's execution seam (utils/keras/runtimes/runtime.py:19-41): constructed as
    `cls(path, **kwargs)` by `build_runtime`, called in place of `model.infer`, with the loaded engine shared between
    instances.  Two deliberate differences from the reference's class: the shared-engine table is keyed by everything that
    changes what gets loaded -- (class, path, device, speaker_embedding_dim), not the path alone, so `device=1` or another
    speaker width never silently returns the first engine -- and it is guarded by a lock (the reference's dict is not)."""
    _engines = {}
    _engines_lock = threading.Lock()

    @classmethod
    def _engine_key(cls, path, kwargs):
        return (cls.__name__, str(path), int(kwargs.get('device', 0) or 0), int(kwargs.get('speaker_embedding_dim', 0) or 0))

    def __init__(self, path, *, engine=None, reload=False, **kwargs):
        self.path = path
        if engine is not None:
            self.engine = engine
            return
        key = self._engine_key(path, kwargs)
        with Runtime._engines_lock:
            if reload or key not in Runtime._engines:
                Runtime._engines[key] = self.load_engine(path, **kwargs)
            self.engine = Runtime._engines[key]

    def __repr__(self):
        return f'<{type(self).__name__} path={self.path}>'

    @abstractmethod
    def __call__(self, *args, **kwargs):
        """Runs inference on the engine."""

    @staticmethod
    @abstractmethod
    def load_engine(path, **kwargs):
        """Builds the engine for `path`."""


class HipRuntime(Runtime):
    """MI355X engine behind the reference's `compiled_infer`.

    path   : a TTSW weight file (text_to_speech_amd.weights.save_ttsw) or a `.safetensors` file with the same tensor
             names, or 'synthetic' / 'synthetic:<seed>' for the
             seeded synthetic weights of SURVEY.md section 8d.
    model  : 'tacotron2' | 'waveglow' | None (None: dispatch on the input dtype -- integer tokens vs float mels).
    vocoder_precision : 'f32' (exact fp32 MFMA, default) or 'f16' (fp16 GEMM operands with fp32 accumulation: the
             counterpart of the reference's `mixed_float16` policy, utils/keras/gpu.py).
    synthesizer_precision : 'f32' (default) or 'f16' (decoder LSTM weights in fp16, everything else fp32).
    """

    def __init__(self, path, *, model=None, engine=None, reload=False, device=0, seed=None, **kwargs):
        super().__init__(path, engine=engine, reload=reload, device=device, **kwargs)
        self.model = model
        self._rng = np.random.default_rng(seed)       # host generator (only `sample_prenet_masks` callers use it)
        # device stream: key + running block offset (a block = 4 values); an unseeded runtime takes its key from the OS
        self._seed = int(seed) if seed is not None else int(np.random.SeedSequence().generate_state(2, np.uint32).view(np.uint64)[0])
        self._offset = 0
        self.max_decoder_steps = int(kwargs.get('max_decoder_steps', 2000))
        self.vocoder_precision = kwargs.get('vocoder_precision', 'f32')
        if self.vocoder_precision not in ('f32', 'f16', 'f16x3'):
            raise ValueError(f"vocoder_precision must be 'f32', 'f16x3' or 'f16', got {self.vocoder_precision!r}")
        self.synthesizer_precision = kwargs.get('synthesizer_precision', 'f32')
        if self.synthesizer_precision not in ('f32', 'f16'):
            raise ValueError(f"synthesizer_precision must be 'f32' or 'f16', got {self.synthesizer_precision!r}")
        # The reference retries a sentence up to `max_trial` times with fresh prenet dropout (models/tts/tacotron2.py:160-179):
        # the encoder output of the last token batch is kept so that a retry only re-runs the decoder loop.
        self._encoded = None                     # (key, EncodedBatch)
        self._denoise_stream = None              # torch stream the vocoder and its denoiser share (waveglow_infer)
        self.encoder_reuses = 0

    @staticmethod
    def load_engine(path, device=0, speaker_embedding_dim=0, **kwargs):
        eng = HipEngine(device)
        if isinstance(path, str) and path.startswith('synthetic'):
            from . import weights
            from .config import Tacotron2Config, WaveGlowConfig
            seed = int(path.split(':', 1)[1]) if ':' in path else 1234
            eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=seed))
            eng.load_state(weights.synth_tacotron2(Tacotron2Config(speaker_embedding_dim=speaker_embedding_dim),
                                                   seed=seed))
        else:
            if not os.path.exists(path):
                raise FileNotFoundError(path)
            if str(path).endswith('.safetensors'):
                from . import weights
                eng.load_state(weights.load_safetensors(path))
            else:
                eng.load_weights(path)
        eng.finalize()
        return eng

    # ------------------------------------------------------------------ dispatch
    def __call__(self, inputs, *args, **kwargs):
        model = self.model
        if model is None:
            first = inputs[0] if isinstance(inputs, (tuple, list)) else inputs
            kind = str(getattr(first, 'dtype', ''))
            model = 'tacotron2' if 'int' in kind else 'waveglow'
        if model == 'tacotron2':
            return self.tacotron2_infer(inputs, **kwargs)
        if model == 'waveglow':
            return self.waveglow_infer(inputs, *args, **kwargs)
        raise ValueError(f'unknown model {model!r}')

    # ------------------------------------------------------------------ Tacotron2.infer (tacotron2_arch.py:866-925)
    def tacotron2_infer(self, inputs, *, max_length=None, early_stopping=True, attn_mask_offset=0.5,
                        attn_mask_win_len=None, prenet_masks=None, deterministic=False, seed=None, precision=None,
                        streams=None, on_device=False, **_ignored):
        """`on_device=True`: host tokens (and speaker) are uploaded first, so the outputs are CUDA tensors that stay on the GPU
        (what `mel_dtw` then reads in place).
        `streams=[(utterance, part, trial), ...]` (one id per row; excludes `prenet_masks` / `deterministic=True`): row b's
        dropout masks come from its own stream `stream_key(seed or the runtime's seed, MASK_STREAM, *id)` at offset 0; the
        runtime's running offset is neither used nor advanced.  A row then draws the same masks in any batch (its mel is its
        own up to the fp32 re-association between decoder machines)."""
        tokens, speaker = _tokens_and_speaker(inputs)
        B = int(tokens.shape[0])
        n_tok = int((tokens != 0).sum(1).max()) if isinstance(max_length, float) else None       # :888-892
        if on_device:
            tokens, speaker = self._uploaded(tokens, np.int32), self._uploaded(speaker)
        max_len = frame_cap(n_tok, max_length, self.max_decoder_steps)                               # :886-887 (the hparam)
        if attn_mask_win_len is not None and isinstance(attn_mask_offset, float):   # :894-897
            attn_mask_offset = int(np.float32(attn_mask_win_len) * np.float32(attn_mask_offset))
        mask_seed, row_mask_seeds = self._draw(MASK_STREAM, B, max_len, prenet_masks, deterministic, seed, streams)
        run = dict(max_len=max_len, early_stopping=bool(early_stopping), attn_mask_win_len=attn_mask_win_len,
                   attn_mask_offset=int(attn_mask_offset or 0), precision=precision or self.synthesizer_precision)
        if not hasattr(self.engine, 'tacotron2_encode'):        # an engine object without the split entry points
            if row_mask_seeds is not None:
                return self.engine.tacotron2_infer(tokens, speaker=speaker, row_mask_seeds=row_mask_seeds, **run)
            if mask_seed is not None:
                prenet_masks = sample_prenet_masks(np.random.default_rng(mask_seed[0] + mask_seed[1]), B, max_len)
            return self.engine.tacotron2_infer(tokens, speaker=speaker, prenet_masks=prenet_masks, **run)
        encoded = self._encoded_batch(tokens, speaker)
        try:
            return self.engine.tacotron2_decode(
                encoded, prenet_masks=prenet_masks, **run,
                **({'mask_seed': mask_seed} if row_mask_seeds is None else {'row_mask_seeds': row_mask_seeds}))
        except Exception:
            # a failed decode may have been caused by the encoded batch itself (e.g. the encoder's block exchange timed out and
            # left its status in the buffer): a retry must run the encoder again, not reuse it
            self._drop_encoded()
            raise

    # ------------------------------------------------------------------ Tacotron2.call (tacotron2_arch.py:806-849)
    def tacotron2_forward(self, inputs, mel_input, mel_lengths=None, *, prenet_masks=None, deterministic=False, seed=None,
                          precision=None, on_device=False):
        """Teacher-forced pass: `inputs` as for `tacotron2_infer` (tokens or (tokens, speaker)), `mel_input` [B, T, 80]
        already shifted (frame 0 the zero go-frame), `mel_lengths` [B].  Dropout as in `tacotron2_infer`: explicit
        `prenet_masks`, `deterministic=True`, `seed=` (offset 0 of that seed's mask stream) or, by default, the runtime's
        seed at its running offset, which the call advances by the B * T * 512 values it draws.  The pass runs on the
        runtime's one kept EncodedBatch, as `tacotron2_infer` does (the encoder runs into it unless it already holds these
        tokens), so neither call costs the other its cached chunk graphs.  Unknown keywords are an error: a misspelt
        `deterministic` must not draw dropout unnoticed.  `on_device=True`: host `mel_input` / `prenet_masks` are uploaded
        first, so the outputs are CUDA tensors that stay on the GPU (what `tacotron2_loss` then reads in place).  Returns the
        engine's Tacotron2ForwardOutput."""
        tokens, speaker = _tokens_and_speaker(inputs)
        if len(mel_input.shape) == 2:
            mel_input = mel_input[None]
        if on_device:
            mel_input, prenet_masks = (self._uploaded(x) for x in (mel_input, prenet_masks))
        B, T = int(mel_input.shape[0]), int(mel_input.shape[1])
        mask_seed, _ = self._draw(MASK_STREAM, B, T, prenet_masks, deterministic, seed)
        draw = {} if mask_seed is None else {'seed': mask_seed[0], 'offset': mask_seed[1]}
        precision = precision or self.synthesizer_precision
        if not hasattr(self.engine, 'tacotron2_encode'):        # an engine object without the split entry points
            return self.engine.tacotron2_forward(tokens, mel_input, mel_lengths, speaker=speaker, prenet_masks=prenet_masks,
                                                 precision=precision, **draw)
        encoded = self._encoded_batch(tokens, speaker)
        try:
            return self.engine.tacotron2_forward(encoded, mel_input, mel_lengths, prenet_masks=prenet_masks,
                                                 precision=precision, **draw)
        except Exception:
            self._drop_encoded()            # as in tacotron2_infer: a retry must run the encoder again
            raise

    def _uploaded(self, x, dtype=np.float32):
        """None, a CUDA tensor as it is, or the host array `x` as a tensor of `dtype` (float32) on the engine's GPU."""
        if x is None or _is_torch_cuda(x):
            return x
        import torch
        return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype)).to(torch.device('cuda', self.engine.device))

    # ------------------------------------------------------------------ TacotronLoss.call (losses/tacotron_loss.py:115-167)
    def tacotron2_loss(self, mel_target, gate_target, decoder_output, mel, stop_tokens, **kwargs):
        """The reference's TacotronLoss per sample on the engine (`HipEngine.tacotron2_loss`, whose keywords these are) ->
        float32 [K, B].  The outputs of `tacotron2_forward(..., on_device=True)` go in without leaving the GPU."""
        return self.engine.tacotron2_loss(mel_target, gate_target, decoder_output, mel, stop_tokens, **kwargs)

    # ------------------------------------------------------------------ MCD along a DTW path (include/tts_hip.h: tts_hip_mel_dtw)
    def mel_dtw(self, a, b, lengths_a=None, lengths_b=None, **kwargs):
        """Mel-cepstral distortion of log-mels `a` [B, Ta, n_mel] against `b` [B, Tb, n_mel] along their DTW path on the engine
        (`HipEngine.mel_dtw`, whose keywords these are) -> float32 [3, B] (cost, path length, MCD in dB), and the path with
        `return_path=True`.  The mel of `tacotron2_infer(..., on_device=True)` goes in without leaving the GPU."""
        return self.engine.mel_dtw(a, b, lengths_a, lengths_b, **kwargs)

    # ------------------------------------------------------------------ pitch (include/tts_hip.h: tts_hip_pitch, tts_hip_f0_error)
    def pitch(self, audio, lengths=None, **kwargs):
        """YIN pitch tracks of `audio` [B, N] on the engine (`HipEngine.pitch`, whose keywords these are) -> float32 [3, B, F]
        (f0 in Hz, period, aperiodicity).  The vocoder's audio on the GPU goes in without leaving it."""
        return self.engine.pitch(audio, lengths, **kwargs)

    def pitch_probe(self, audio, lengths=None, **kwargs):
        """Test hook: one stage of `pitch` (`HipEngine.pitch_probe`)."""
        return self.engine.pitch_probe(audio, lengths, **kwargs)

    def pyin(self, audio, lengths=None, **kwargs):
        """Probabilistic-YIN pitch tracks of `audio` [B, N] on the engine (`HipEngine.pyin`, whose keywords these are) -> float32
        [3, B, F]: f0 (0 where unvoiced), the decoded bin's pitch, the voiced probability."""
        return self.engine.pyin(audio, lengths, **kwargs)

    def pyin_probe(self, audio, lengths=None, **kwargs):
        """Test hook: one stage of `pyin` (`HipEngine.pyin_probe`)."""
        return self.engine.pyin_probe(audio, lengths, **kwargs)

    def f0_error(self, f0_a, f0_b, lengths_a=None, lengths_b=None, path=None, **kwargs):
        """Two F0 tracks compared along a path (`HipEngine.f0_error`, whose keywords these are) -> float32 [6, B]."""
        return self.engine.f0_error(f0_a, f0_b, lengths_a, lengths_b, path, **kwargs)

    def _draw(self, purpose, rows, frames, explicit, deterministic, seed, streams=None):
        """Where a call's random values (`purpose`: MASK_STREAM / NOISE_STREAM) come from -> (stream, row streams), at most
        one of them set: row streams ([key per row], [0 per row]) for `streams` ids, keyed by `seed` or the runtime's seed;
        neither for `explicit` values or `deterministic`; else the stream (key, offset) -- offset 0 of `seed`'s key, or the
        runtime's key at its running offset, which only this last case advances, by the blocks of `rows` x `frames`."""
        blocks, id_width, explicit_name = _DRAWS[purpose]
        if streams is not None:
            if explicit is not None or deterministic:
                raise ValueError(f'streams excludes {explicit_name} and deterministic=True')
            base = self._seed if seed is None else int(seed)
            return None, ([stream_key(base, purpose, *i) for i in _row_ids(streams, rows, id_width)], [0] * rows)
        if explicit is not None or deterministic:
            return None, None
        if seed is not None:
            return ((int(seed) ^ purpose) & _U64, 0), None
        offset = self._offset
        self._offset += blocks(rows, frames)
        return ((self._seed ^ purpose) & _U64, offset), None

    def _encoded_batch(self, tokens, speaker):
        """The runtime's one EncodedBatch, holding `tokens` (+ `speaker`): kept as it is when it already does, else the
        encoder runs again INTO it.  Encoder reuse (the reference retries a sentence with fresh dropout,
        models/tts/tacotron2.py:160-179): inputs are recognised by CONTENT -- host inputs by their bytes, device inputs by
        comparing them on the device with the runtime's own copy of the batch that was encoded (an address / version key is
        not enough: the caching allocator hands the address of a freed token tensor to the next sentence's tensor of the same
        shape)."""
        dev = _is_torch_cuda(tokens)
        if dev:
            key = self._device_key(tokens, speaker)
        else:
            spk_np = None if speaker is None else (speaker.detach().cpu().numpy() if _is_torch_cuda(speaker) else np.asarray(speaker))
            key = ('host', tokens.shape, tokens.astype(np.int32).tobytes(),
                   None if spk_np is None else spk_np.astype(np.float32).tobytes())
        if self._encoded is not None and (self._encoded[0] is key if dev else self._encoded[0] == key):
            self.encoder_reuses += 1
        elif self._encoded is not None:
            # one encoded-batch handle per runtime, overwritten sentence after sentence: no device allocation per sentence,
            # and the decoder's cached step graphs (keyed by that buffer) are replayed instead of re-captured
            handle = self._encoded[1]
            self._encoded = None
            try:
                self._encoded = (key, self.engine.tacotron2_encode(tokens, speaker=speaker, into=handle))
            except Exception:
                handle.close()
                raise
        else:
            self._encoded = (key, self.engine.tacotron2_encode(tokens, speaker=speaker))
        return self._encoded[1]

    def _device_key(self, tokens, speaker):
        """Key of a device token batch: the cached key itself when the contents equal the batch it was made from (one tiny
        comparison kernel + a host read of its verdict), else a new key holding private copies of the inputs."""
        import torch
        spk_dev = speaker is not None and _is_torch_cuda(speaker)
        if self._encoded is not None and self._encoded[0][0] == 'dev':
            _, kept_tok, kept_spk = self._encoded[0]
            same = (kept_tok.device == tokens.device and tuple(kept_tok.shape) == tuple(tokens.shape)
                    and (kept_spk is None) == (speaker is None))
            if same and speaker is not None:
                spk = speaker if spk_dev else torch.as_tensor(np.asarray(speaker), dtype=torch.float32)
                same = tuple(kept_spk.shape) == tuple(spk.shape) and bool(torch.equal(kept_spk, spk.to(device=kept_spk.device, dtype=torch.float32)))
            if same and bool(torch.equal(kept_tok, tokens.to(torch.int32))):
                return self._encoded[0]
        spk_copy = None
        if speaker is not None:
            spk_copy = (speaker if spk_dev else torch.as_tensor(np.asarray(speaker), dtype=torch.float32)).to(
                device=tokens.device, dtype=torch.float32).clone()
        return ('dev', tokens.to(torch.int32).clone(), spk_copy)

    def _drop_encoded(self):
        if self._encoded is not None:
            try:
                self._encoded[1].close()
            finally:
                self._encoded = None

    # ------------------------------------------------------------------ WaveGlow.infer (waveglow_arch.py:244-306)
    def waveglow_infer(self, mel, z=None, sigma=1.0, deterministic=False, seed=None, precision=None, lengths=None,
                       packed=False, streams=None, denoiser_strength=None, **_ignored):
        """`lengths` [B] (frames of each row that are real): a batch of unequal rows -- every row's audio is that of its own
        frames, zeros behind it (HipEngine.waveglow_infer); the noise is drawn in the batch layout either way.
        `packed=True` (with `lengths`): the same call computed as one packed row; noise values and the running offset are
        those of the call without it.
        `streams=[(utterance, part), ...]` (one id per row; excludes `z` / `deterministic=True`): row b's noise comes from
        its own stream `stream_key(seed or the runtime's seed, NOISE_STREAM, utterance, part, 0)` at offset 0; the running
        offset is neither used nor advanced.  With `lengths` (packed or not) a row's audio is then the same in any batch, up
        to fp32 re-association; a padded batch (no `lengths`) keeps hearing its padding.
        `denoiser_strength` (None or 0: off, the call is today's): the audio stays on the device and goes through this
        precision's `Denoiser` there -- `strength` x the vocoder's bias spectrum taken off every frame, each row with
        lengths[b] * 256 samples as its length -- on one stream with the vocoder, before anything comes to the host; a CUDA
        mel still gives a CUDA tensor."""
        if denoiser_strength is not None and not float(denoiser_strength) >= 0:
            raise ValueError(f'denoiser_strength must be >= 0 (or None), got {denoiser_strength!r}')
        if packed and lengths is None:
            raise ValueError('packed=True needs lengths (one frame count per row)')
        if not _is_torch_cuda(mel):
            mel = np.asarray(mel, dtype=np.float32)
        if mel.ndim == 2:
            mel = mel[None]
        B, T = int(mel.shape[0]), int(mel.shape[1])
        ragged = {} if lengths is None else {'lengths': lengths, 'packed': True} if packed else {'lengths': lengths}
        noise, row_seeds = self._draw(NOISE_STREAM, B, T, z, deterministic, seed, streams)
        draw = ({'row_seeds': row_seeds} if row_seeds is not None else {'z': z} if noise is None
                else {'seed': noise[0], 'offset': noise[1]})
        precision = precision or self.vocoder_precision
        if not denoiser_strength:
            return self.engine.waveglow_infer(mel, sigma=float(sigma), precision=precision, **draw, **ragged)
        import torch
        denoiser = self.denoiser(precision)
        denoiser.bias                                   # the model's bias is taken (once) before anything is enqueued
        # vocoder and denoiser are enqueued on one stream of the runtime's own (torch's default stream has no handle the engine
        # could enqueue on); what the caller does next on the current stream waits for it
        if self._denoise_stream is None:
            self._denoise_stream = torch.cuda.Stream(self.engine.device)
        stream, current = self._denoise_stream, torch.cuda.current_stream(self.engine.device)
        if 'z' in draw:
            draw['z'] = self._uploaded(draw['z'])
        audio = self.engine.waveglow_infer(self._uploaded(mel), sigma=float(sigma), precision=precision, stream=stream, **draw, **ragged)
        samples = None if lengths is None else np.maximum(self.engine._frame_lengths(lengths, B, T).astype(np.int64) * 256, 1)
        audio = denoiser(audio, float(denoiser_strength), lengths=samples, stream=stream)
        current.wait_stream(stream)
        audio.record_stream(current)
        return audio if _is_torch_cuda(mel) else audio.cpu().numpy()

    def denoiser(self, precision=None):
        """The `Denoiser` of this runtime's vocoder in `precision` (default: the runtime's): one per precision and engine
        handle, kept on the engine.  Its bias comes from a call of its own with explicit zero noise: the runtime's running
        noise offset is neither used nor advanced."""
        from .denoiser import Denoiser
        precision = precision or self.vocoder_precision
        kept = self.engine.__dict__.setdefault('_denoisers', {})
        if precision not in kept:
            kept[precision] = Denoiser(self.engine, precision=precision)
        return kept[precision]

    def denoise(self, audio, strength=0.1, lengths=None, precision=None):
        """`audio` [N] or [B, N] (a waveform of this runtime's vocoder, e.g. one stitched from several calls) through
        `denoiser(precision)` -> [B, N]."""
        return self.denoiser(precision)(audio, strength, lengths=lengths)

    def time_stretch(self, audio, rate, lengths=None, plan=None):
        """`audio` [N] or [B, N] played `rate` times as fast at the same pitch on this runtime's engine
        (`effects.time_stretch`, default plan 1024 / 256 / 1024) -> (out, out_lengths)."""
        from .effects import time_stretch
        return time_stretch(audio, rate, engine=self.engine, plan=plan, lengths=lengths)

    def pitch_shift(self, audio, n_steps, lengths=None, plan=None, **kwargs):
        """`audio` [N] or [B, N] raised by `n_steps` semitones at the same duration on this runtime's engine
        (`effects.pitch_shift`; `preserve_formants=True` keeps the voice's spectral envelope, `formant_steps` moves it)."""
        from .effects import pitch_shift
        return pitch_shift(audio, n_steps, engine=self.engine, plan=plan, lengths=lengths, **kwargs)

    def formant_shift(self, audio, n_steps, lengths=None, plan=None, **kwargs):
        """`audio` [N] or [B, N] with its formants moved by `n_steps` semitones, pitch and duration kept
        (`effects.formant_shift`, default plan 1024 / 256 / 1024)."""
        from .effects import formant_shift
        return formant_shift(audio, n_steps, engine=self.engine, plan=plan, lengths=lengths, **kwargs)

    def waveglow_encode(self, audio, mel, lengths=None, stream=None):
        """The forward flow of the vocoder, audio [B, T*256] + mel [B, T, 80] -> (z [B, T*32, 8], stats [3, B]), fp32
        (HipEngine.waveglow_encode); a single utterance ([T*256] with [T, 80]) gets its batch axis."""
        if len(mel.shape) == 2:
            audio, mel = audio[None], mel[None]
        return self.engine.waveglow_encode(audio, mel, lengths=lengths, stream=stream)


_runtimes = {'hip': HipRuntime}


def build_runtime(runtime, path, *args, **kwargs):
    """Same signature and error behaviour as the reference's `build_runtime` (runtimes/__init__.py:23-37)."""
    if runtime not in _runtimes:
        raise ValueError('Unsupported runtime !\n  Accepted : {}\n  Got : {}'.format(tuple(_runtimes.keys()), runtime))
    return _runtimes[runtime](path, *args, **kwargs)


__all__ = ['Runtime', 'HipRuntime', 'build_runtime', 'Tacotron2InferenceOutput', 'stream_key', 'frame_cap']
