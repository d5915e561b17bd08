"""Host-side WaveGlow wrapper: the argument / return contract of the reference's `models.tts.WaveGlow.infer`.

Same behaviour as /root/reference/models/tts/waveglow.py:61-142 (`infer`: path / 2-D / 3-D mel input, `audio_len = T * 256`,
optional pad-to-`win_len` with -11, window / hop chunking with centre-half stitching) and :156-164 (`_get_steps`),
pinned by outputs of the reference's own `_get_steps` and stitch statements (tests/golden/host_vectors.json,
tests/test_host_vectors.py) and the known-answer tests in tests/test_host_logic.py.
The compute call (`self.compiled_infer`) is a `HipRuntime`; nothing here touches a CPU fallback.
"""
from __future__ import annotations

import math

import numpy as np

from .engine import _is_torch_cuda


def window_starts(length, win_len, hop_len):
    """First frames of the analysis windows: the fewest windows of `win_len` frames, at most `hop_len` apart, that cover
    `length` frames, re-spaced evenly so that the last one ends exactly at `length` (the rule of
    models/tts/waveglow.py:156-164).  E.g. (1000, 256, 192) -> 0, 186, 372, 558, 744."""
    n = 1 + max(0, int(math.ceil((length - win_len) / hop_len)))
    if n == 1:
        return [0]
    spacing = (length - win_len) / (n - 1)
    return np.round(spacing * np.arange(n)).astype(np.int32)


_get_steps = window_starts          # the reference's name for it


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


# ---- exact time tiling ------------------------------------------------------------------------------------------------
# WaveGlow inference is feed-forward with a finite receptive field: per flow the 8 dilated k=3 convs reach
# 1 + 2 + ... + 128 = 255 groups (of 8 samples) to each side, 12 flows -> 3060 groups = 95.6 mel frames, plus the 4-frame
# window of the upsampling transposed conv.  A tile computed from its frames plus HALO_FRAMES of
# real context on each side therefore reproduces the full-sequence samples of its core region exactly; only samples whose
# receptive field crosses an artificial tile edge differ, and those all lie inside the discarded halo.  (The reference's
# own windowing, `infer(win_len=...)` below, is approximate: it discards half of a 64-frame overlap.)
HALO_FRAMES = 100


def tile_plan(n_frames, tile_frames, halo=HALO_FRAMES):
    """[(start, stop, lo, hi)]: core frames [start, stop) are taken from a run over mel[lo:hi]."""
    if tile_frames <= 0:
        raise ValueError('tile_frames must be positive')
    plan = []
    for start in range(0, n_frames, tile_frames):
        stop = min(n_frames, start + tile_frames)
        plan.append((start, stop, max(0, start - halo), min(n_frames, stop + halo)))
    return plan


def infer_tiled(compiled_infer, mel, z=None, tile_frames=4096, halo=HALO_FRAMES, tiles=None, **kwargs):
    """Exact vocoding of a long mel [B, T, 80] in time tiles; `tiles` (indices into tile_plan) restricts the work to a
    subset (multi-GPU sharding of one utterance) -- the result then is a list of (start, stop, audio [B, (stop-start)*256])."""
    T = mel.shape[1]
    plan = tile_plan(T, tile_frames, halo)
    chosen = range(len(plan)) if tiles is None else tiles
    out = []
    for i in chosen:
        start, stop, lo, hi = plan[i]
        zz = None if z is None else z[:, lo * 32:hi * 32]
        if _is_torch_cuda(mel):
            sub = mel[:, lo:hi].contiguous()
            zz = None if zz is None else zz.contiguous()
        else:
            sub = np.ascontiguousarray(mel[:, lo:hi])
        a = compiled_infer(sub, z=zz, **kwargs)
        out.append((start, stop, a[:, (start - lo) * 256:(stop - lo) * 256]))
    if tiles is not None:
        return out
    parts = [_to_numpy(a) for _, _, a in out]
    return np.concatenate(parts, axis=1)


class WaveGlow:
    """`vocoder(mel, **kwargs)` object accepted by `Tacotron2.infer(..., vocoder=...)`: the argument / return contract of
    the reference's `models.tts.WaveGlow.infer` (models/tts/waveglow.py:61-142).

    mel: a `.npy` path, [T, 80] or [B, T, 80] -> audio [B, T * 256] (windowed single-utterance mode: [T * 256]).
    Without `win_len` the whole mel is vocoded in one call; a batch of unequal utterances then takes `lengths=[...]` (frames
    of each row that are real): row b's audio[:lengths[b] * 256] is that of its own frames, zeros behind it (`packed=True` next
    to it: the same audio computed as one packed row, work proportional to sum(lengths)).  With it (frames; a float means "a multiple of": rounded up,
    or down with `use_slice`; capped by `max_win_len`):
      * a mel that fits one window is vocoded directly -- padded to the window with -11 first only if `force_pad`
        (default: only for the keras runtime, i.e. never here), the result cut back to T * 256 samples;
      * a batch is vocoded directly;
      * a longer utterance is cut into overlapping windows (`hop_len` frames apart; negative = window minus that many,
        float = fraction of the window), each vocoded alone or all as one batch (`batch=True`), and stitched by dropping
        half of every overlap from each side.  This is the reference's approximation (the vocoder's receptive field is
        longer than the half-overlap); `infer_exact` is the exact alternative.
    `denoiser_strength` (HipRuntime.waveglow_infer): a direct call passes it on; stitched windows and `infer_exact` vocode without
    it and denoise the whole waveform once at the end (`HipRuntime.denoise`) -- per-window denoising would change the frames
    at every seam."""
    rate = 22050
    pad_mel_value = -11.
    runtime = 'hip'

    def __init__(self, compiled_infer):
        self.compiled_infer = compiled_infer

    def _resolve_window(self, n_frames, win_len, use_slice, max_win_len):
        if isinstance(win_len, float):
            count = max(1, n_frames // win_len) if use_slice else math.ceil(n_frames / win_len)
            win_len = int(count * win_len) if not use_slice else int(count) * int(win_len)
        return int(win_len if max_win_len is None else min(max_win_len, win_len))

    def _pad_frames(self, mel, n_frames):
        extra = n_frames - mel.shape[1]
        if _is_torch_cuda(mel):
            import torch
            return torch.nn.functional.pad(mel, (0, 0, 0, extra), value=self.pad_mel_value)
        return np.pad(np.asarray(mel), [(0, 0), (0, extra), (0, 0)], constant_values=self.pad_mel_value)

    def _denoise_whole(self, audio, strength, precision):
        """An assembled waveform [N] or [B, N] through the runtime's denoiser, in the shape it came in."""
        denoise = getattr(self.compiled_infer, 'denoise', None)
        if denoise is None:
            raise ValueError('denoiser_strength on an assembled waveform needs a runtime with denoise (HipRuntime) behind the model')
        out = _to_numpy(denoise(audio, strength, precision=precision))
        return out[0] if len(audio.shape) == 1 else out

    def infer(self, mel, *, win_len=None, hop_len=-64, force_pad=None, batch=False, use_slice=False,
              max_win_len=None, **kwargs):
        if isinstance(mel, str):
            mel = np.load(mel)
        if len(mel.shape) == 2:
            mel = mel[None]
        n_frames = mel.shape[1]
        n_samples = n_frames * 256
        if win_len is None:
            return self.compiled_infer(mel, **kwargs)[:, :n_samples]
        # with windows the keyword belongs to one call of a whole waveform: a direct call below, or the stitched result
        strength = kwargs.pop('denoiser_strength', None)
        direct = {'denoiser_strength': strength} if strength else {}

        win_len = self._resolve_window(n_frames, win_len, use_slice, max_win_len)
        kwargs['padding_multiple'] = win_len
        if n_frames <= win_len:
            if force_pad is None:
                force_pad = self.runtime == 'keras'               # waveglow.py:95 -- False for this runtime
            if not force_pad:
                return self.compiled_infer(mel, **direct)
            return self.compiled_infer(self._pad_frames(mel, win_len), **kwargs, **direct)[:, :n_samples]
        if mel.shape[0] > 1:
            return self.compiled_infer(mel, **kwargs, **direct)

        if isinstance(hop_len, float):
            hop_len = int(win_len * hop_len)
        if hop_len < 0:
            hop_len += win_len
        starts = np.asarray(window_starts(n_frames, win_len, hop_len))
        windows = [mel[:, s0:s0 + win_len] for s0 in starts]
        if batch:
            if _is_torch_cuda(mel):
                import torch
                stacked = torch.cat(windows, dim=0)
            else:
                stacked = np.concatenate([np.asarray(w) for w in windows], axis=0)
            pieces = list(_to_numpy(self.compiled_infer(stacked, **kwargs)))
        else:
            pieces = [_to_numpy(self.compiled_infer(w, **kwargs)[0]) for w in windows]
        # consecutive windows share (end of k) - (start of k + 1) frames: each gives up half of those samples
        shared = (starts[:-1] + win_len - starts[1:]) * 256
        head = np.concatenate([[0], shared // 2])
        tail = np.concatenate([-(-shared // 2), [0]])            # the reference slices `[: -overlap // 2]` = ceil half
        last = len(pieces) - 1
        # (sic) a window that shares NO frame with its successor (hop_len == win_len) is sliced `part[start : -0 // 2]` =
        # `part[start : 0]` by the reference (models/tts/waveglow.py:136-139): empty.  Kept, because the contract here is the
        # reference's output on the same arguments (pinned by tests/golden/host_vectors.json); overlapping windows -- every
        # default -- are seamless.
        ends = [len(p) - t if (i == last or t > 0) else 0 for i, (p, t) in enumerate(zip(pieces, tail))]
        stitched = np.concatenate([p[h:e] for p, h, e in zip(pieces, head, ends)], axis=-1)
        return self._denoise_whole(stitched, strength, kwargs.get('precision')) if strength else stitched

    __call__ = infer

    # ---- the forward flow: audio -> z and its likelihood (the direction the published model is trained and scored with)
    MAX_RUN_FRAMES = 31744              # B * T of one `waveglow_encode` call (include/tts_hip.h)

    def _encode_runtime(self, what):
        encode = getattr(self.compiled_infer, 'waveglow_encode', None)
        if encode is None:
            raise ValueError(f'{what} needs a runtime with waveglow_encode (HipRuntime) behind the model')
        return encode

    def _recording(self, audio, mel, load_kwargs):
        """One recording as (waveform float32 [frames * 256] zero-padded or cut to its mel's frames, mel float32 [frames, 80]):
        `audio` is a file name (loaded by `audio.load_audio` at the model's rate with `load_kwargs`) or a waveform, taken as it
        is; `mel` None: the mel of those samples, through `audio.load_mel` on the model's engine."""
        from .audio import load_audio, load_mel
        engine = getattr(self.compiled_infer, 'engine', None)
        if isinstance(audio, (str, bytes, dict)):
            wave = load_audio(audio, self.rate, engine=engine, **load_kwargs)
        else:
            wave = audio
        wave = np.asarray(_to_numpy(wave), dtype=np.float32).reshape(-1)
        if mel is None:
            mel = load_mel(wave, self.rate, engine=engine, normalize=False)      # (of the samples that are encoded)
        mel = np.asarray(_to_numpy(mel), dtype=np.float32)
        if mel.ndim == 3 and mel.shape[0] == 1:
            mel = mel[0]
        if mel.ndim != 2 or mel.shape[1] != 80:
            raise ValueError(f'mel must be [frames, 80], got {mel.shape}')
        n = mel.shape[0] * 256
        padded = np.zeros(n, dtype=np.float32)
        padded[:min(n, len(wave))] = wave[:n]
        return padded, mel

    @staticmethod
    def _nll(stats, frames, sigma):
        """[4, N]: nll per sample, sum_z2, sum_log_s, log_det_w from stats [3, N] and the rows' frame counts (0 frames: nll 0)."""
        stats = np.asarray(stats, dtype=np.float64)
        frames = np.asarray(frames, dtype=np.float64)
        total = stats[0] / (2.0 * float(sigma) ** 2) - stats[1] - stats[2]
        nll = np.where(frames > 0, total / np.maximum(frames * 256.0, 1.0), 0.0)
        return np.stack([nll, stats[0], stats[1], stats[2]])

    def encode(self, audio, mel=None, **load_kwargs):
        """A recording's latent under the model: `audio` (a file name or a waveform) and its `mel` [frames, 80] -- None: through
        `audio.load_mel` on the model's engine, with `load_kwargs` for the file -- go through the forward flow; the audio is
        zero-padded to frames * 256 samples.  Returns {'z' [frames * 32, 8] (what `infer(mel, z=z[None] * tau)` re-synthesizes
        from), 'mel' [frames, 80], 'nll' (per sample, sigma = 1, without the constant log(2 pi) / 2), 'sum_z2', 'sum_log_s',
        'log_det_w'}.  Needs a runtime with `waveglow_encode` (HipRuntime) behind the model."""
        encode = self._encode_runtime('encode')
        wave, mel = self._recording(audio, mel, load_kwargs)
        z, stats = encode(wave[None], mel[None])
        nll, z2, ls, ld = self._nll(_to_numpy(stats), [mel.shape[0]], 1.0)[:, 0]
        return {'z': _to_numpy(z)[0], 'mel': mel, 'nll': float(nll), 'sum_z2': float(z2), 'sum_log_s': float(ls),
                'log_det_w': float(ld)}

    def evaluate(self, items, *, batch_size=8, sigma=1.0, **load_kwargs):
        """The model's negative log-likelihood on held-out recordings.  `items`: waveforms, file names or (audio, mel) pairs,
        each prepared as in `encode`.  Consecutive items form ragged batches of at most `batch_size` rows that also fit one run
        (rows * longest row <= MAX_RUN_FRAMES), padded with zeros and passed with their `lengths`, so every item gets what a
        call of its own gives it; only the [3, B] statistics come to the host.  Per item
            nll = (sum_z2 / (2 sigma^2) - sum_log_s - log_det_w) / (frames * 256)      (0 for an empty item)
        Returns {'names' ('nll', 'sum_z2', 'sum_log_s', 'log_det_w'), 'per_item' float64 [4, N] in input order, 'mean' [4]}."""
        encode = self._encode_runtime('evaluate')
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f'batch_size must be at least 1, got {batch_size}')
        if not float(sigma) > 0:
            raise ValueError(f'sigma must be positive, got {sigma}')
        names = ('nll', 'sum_z2', 'sum_log_s', 'log_det_w')
        prepared = []
        for item in items:
            audio, mel = item if isinstance(item, tuple) else (item, None)
            prepared.append(self._recording(audio, mel, load_kwargs))
        per_item = np.zeros((4, len(prepared)), dtype=np.float64)
        start = 0
        while start < len(prepared):
            stop, longest = start, 0
            while stop < len(prepared) and stop - start < batch_size:
                t = max(longest, prepared[stop][1].shape[0])
                if (stop - start + 1) * max(t, 1) > self.MAX_RUN_FRAMES:
                    break
                stop, longest = stop + 1, t
            if stop == start:
                raise ValueError(f'item {start} holds {prepared[start][1].shape[0]} frames, above one run\'s limit '
                                 f'({self.MAX_RUN_FRAMES})')
            rows = prepared[start:stop]
            T = max(longest, 1)
            audio = np.zeros((len(rows), T * 256), dtype=np.float32)
            mels = np.zeros((len(rows), T, 80), dtype=np.float32)
            lengths = np.array([m.shape[0] for _, m in rows], dtype=np.int32)
            for r, (w, m) in enumerate(rows):
                audio[r, :len(w)] = w
                mels[r, :m.shape[0]] = m
            _, stats = encode(audio, mels, lengths=lengths)
            per_item[:, start:stop] = self._nll(_to_numpy(stats), lengths, sigma)
            start = stop
        mean = per_item.mean(axis=1) if len(prepared) else np.zeros(4)
        return {'names': names, 'per_item': per_item, 'mean': mean}

    def copy_synthesis(self, mels, *, n_cep=13, **infer_kwargs):
        """Copy synthesis: every mel of `mels` ([T, 80] each) is vocoded (`infer` with `infer_kwargs`), the audio analysed again
        with the engine's default mel plan (`mel_stft`), and the input mel compared with the re-analysed one frame by frame --
        the un-aligned mel-cepstral distortion of `mel_dtw(align=False)` over the frames both have; audio and mels stay on the
        GPU.  Returns {'names': ['mcd', 'frames'], 'per_item': float32 [2, N] in input order, 'mean': {name: float}}.  Needs a
        runtime with an `engine` (HipRuntime) behind the model."""
        engine = getattr(self.compiled_infer, 'engine', None)
        if getattr(engine, 'mel_dtw', None) is None or getattr(engine, 'mel_stft', None) is None:
            raise ValueError('copy_synthesis needs a runtime with an engine (HipRuntime) behind the model')
        upload = getattr(self.compiled_infer, '_uploaded', lambda x: x)
        names = ['mcd', 'frames']
        per_item = np.zeros((2, len(mels)), dtype=np.float32)
        for i, mel in enumerate(mels):
            if len(mel.shape) != 2:
                raise ValueError(f'mels[{i}] must be [T, 80], got {tuple(mel.shape)}')
            mel = upload(mel)[None]
            stats = _to_numpy(engine.mel_dtw(mel, engine.mel_stft(self.infer(mel, **infer_kwargs)), n_cep=n_cep, align=False))
            per_item[:, i] = stats[2, 0], stats[1, 0]
        mean = {name: float(per_item[k].astype(np.float64).mean()) if len(mels) else float('nan') for k, name in enumerate(names)}
        return {'names': names, 'per_item': per_item, 'mean': mean}

    RESYNTHESIS_NAMES = ['f0_rmse_cents', 'f0_mean_cents', 'vuv_error', 'gross_error', 'voiced_pairs', 'pairs']

    def resynthesis_f0(self, items, f0_method='yin', f0_config=None, **infer_kwargs):
        """Does the vocoder keep the pitch?  `items` as for `evaluate`: recordings (waveforms or file names) or (audio, mel)
        pairs, each prepared by `_recording`.  The mel is vocoded (`infer` with `infer_kwargs`), `pitch` (tts_hip_pitch, the
        defaults at the model's rate) runs on the recording zero-padded to frames * 256 samples and on the vocoded audio, and
        `f0_error` compares the two tracks on the diagonal; audio and tracks stay on the GPU.  Returns {'names':
        RESYNTHESIS_NAMES, 'per_item': float32 [6, N] in input order, 'mean': {name: float}}: the F0 RMSE and the mean
        deviation of the voiced pairs in cents, the voicing error rate (of the pairs), the gross pitch error rate (more than
        20 % off; of the voiced pairs, 0 without any), the voiced pairs and the pairs.  Needs a runtime with an `engine`
        (HipRuntime) behind the model.  `f0_method='pyin'` tracks both with `pyin` (tts_hip_pyin) in place of `pitch`;
        `f0_config`: further keywords of the tracker (the rate stays the model's)."""
        from .pitch import track_f0
        engine = getattr(self.compiled_infer, 'engine', None)
        if getattr(engine, 'pitch', None) is None or getattr(engine, 'f0_error', None) is None:
            raise ValueError('resynthesis_f0 needs a runtime with an engine (HipRuntime) behind the model')
        f0_config = dict(f0_config or {}, rate=self.rate)
        upload = getattr(self.compiled_infer, '_uploaded', lambda x: x)
        names = self.RESYNTHESIS_NAMES
        per_item = np.zeros((len(names), len(items)), dtype=np.float32)
        for i, item in enumerate(items):
            audio, mel = item if isinstance(item, tuple) else (item, None)
            wave, mel = self._recording(audio, mel, {})
            if mel.shape[0] < 1:
                raise ValueError(f'items[{i}] holds no frame')
            vocoded = self.infer(upload(mel)[None], **infer_kwargs)
            f0_rec = track_f0(engine, f0_method, upload(wave)[None], **f0_config)[0]
            f0_voc = track_f0(engine, f0_method, vocoded, **f0_config)[0]
            s = _to_numpy(engine.f0_error(f0_rec, f0_voc))[:, 0]
            per_item[:, i] = s[2], s[3], s[4] / max(s[0], 1), s[5] / max(s[1], 1), s[1], s[0]
        mean = {name: float(per_item[k].astype(np.float64).mean()) if len(items) else float('nan') for k, name in enumerate(names)}
        return {'names': list(names), 'per_item': per_item, 'mean': mean}

    def infer_exact(self, mel, *, tile_frames=4096, z=None, **kwargs):
        """Long-form vocoding without the approximation of `infer(win_len=...)`: halo tiling, bit-for-bit the samples of
        one run over the whole mel (which one C-ABI call only accepts up to ~31.7 k frames).  `denoiser_strength`: the tiles
        are vocoded without it and the whole waveform is denoised once."""
        if isinstance(mel, str):
            mel = np.load(mel)
        if len(mel.shape) == 2:
            mel = mel[None]
        strength = kwargs.pop('denoiser_strength', None)
        if strength and kwargs.get('tiles') is not None:
            raise ValueError('infer_exact: denoiser_strength needs the whole waveform, not a subset of its tiles')
        audio = infer_tiled(self.compiled_infer, mel, z=z, tile_frames=tile_frames, **kwargs)
        return self._denoise_whole(audio, strength, kwargs.get('precision')) if strength else audio
