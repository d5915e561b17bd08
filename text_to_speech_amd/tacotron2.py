"""Host-side Tacotron2 wrapper and the `tts()` / `stream()` facade.

Restates the host logic of the reference's models/tts/tacotron2.py:104-241 (`Tacotron2.infer`: split / clean / encode,
per-part batch-1 call, retry while the frame/token ratio is outside (min_fpt_ratio, max_fpt_ratio) up to `max_trial`
times, slice to `lengths`, vocoder call, concatenation, result dict with keys text, cleaned, splitted, mel, attention,
audio, rate, time), :276-352 (`get_inference_callbacks`: the `predicted` map / `map.json` cache and the savers),
:354-367 (`precompile_for_stream`, `stream`), models/interfaces/base_model.py:676-711 (`predict`) and
models/tts/__init__.py:62-101 (`tts`, `stream`).  Callbacks live in text_to_speech_amd/callbacks.py; audio players /
notebook displayers are out of scope.
"""
from __future__ import annotations

import logging
import queue as _queue
import time

import os

import numpy as np

from .callbacks import (AudioSaver, default_audio_format, Callback, FunctionCallback, JSONSaver, QueueCallback, SpectrogramSaver,
                        apply_callbacks, load_json)
from .runtime import frame_cap
from .text import CharTokenizer, split_sentences, split_text

logger = logging.getLogger(__name__)


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def attention_durations(attention, length=None):
    """Per-token durations from the alignments of one utterance: `attention` [T, Tin] -> int64 [Tin], durations[i] = number
    of frames t < length (default T) whose attention argmax (first index on ties) is token i.  They sum to `length`."""
    att = _to_numpy(attention)
    if att.ndim != 2:
        raise ValueError(f'attention must be [T, Tin], got {att.shape}')
    n = att.shape[0] if length is None else int(length)
    if not 0 <= n <= att.shape[0]:
        raise ValueError(f'length {n} is outside [0, T = {att.shape[0]}]')
    return np.bincount(att[:n].argmax(axis=1), minlength=att.shape[1]).astype(np.int64)


def shift_mel_target(mel):
    """Decoder input of a teacher-forced pass for the target `mel` [F, 80]: the zero go-frame, then target frames 0 .. F - 2
    (the reference's prepare_data, models/tts/tacotron2.py:243-259: pad(mel, [(1, 0), (0, 0)])[:-1], length F)."""
    mel = np.asarray(_to_numpy(mel), dtype=np.float32)
    if mel.ndim != 2 or mel.shape[0] < 1:
        raise ValueError(f'mel must be [frames >= 1, n_mel], got {mel.shape}')
    return np.concatenate([np.zeros((1, mel.shape[1]), np.float32), mel[:-1]], axis=0)


class Tacotron2:
    rate = 22050
    pad_mel_value = 0.      # what a batch of mels is padded with (the reference's BaseAudioModel default, base_audio_model.py:37)

    def __init__(self, compiled_infer, lang='en', tokenizer=None, pred_dir=None):
        self.compiled_infer = compiled_infer
        if isinstance(tokenizer, str):                           # a shipped model's `saving/tokenizer.json`
            tokenizer = CharTokenizer.load_from_file(tokenizer, lang=lang)
        self.tokenizer = tokenizer or CharTokenizer(lang)
        self.pred_dir = pred_dir or os.path.join('pretrained_models', 'tacotron2_hip', 'outputs')

    def clean_text(self, text, **kwargs):
        return self.tokenizer.clean_text(text, **kwargs)

    def encode_text(self, text, cleaned=False):
        return self.tokenizer.encode(text, cleaned=cleaned)

    def infer(self, text, *, callbacks=None, predicted=None, overwrite=False, return_output=True, utterance=None, **kwargs):
        """One text (or a dict holding it under 'text' / 'content') -> its result dict.  The keywords of the stages
        (`_stage_kwargs`): `embeddings`, `max_length=10.`, `max_text_length=-1`, `max_trial=5`, `min_fpt_ratio=2.`,
        `max_fpt_ratio=10.` (`_synthesize`), `vocoder`, `vocoder_config` (`_vocode_parts`), `silence_time=0.15`,
        `reduce_noise`, `trim_silence`, `speed=1.0` (tempo; 1.25 speaks a quarter faster), `pitch_steps=0.0` (semitones),
        `preserve_formants=False` (the shifted voice keeps its spectral envelope), `formant_steps=0.0` (semitones the envelope
        itself moves by: the apparent size of the speaker)
        (`_finish`; none of these is part of the `map.json` key); every other keyword reaches the text cleaner and both models.
        `utterance` (an int; `predict(sentence_streams=True)` numbers its inputs): every random draw of this text comes
        from a stream of its own -- part p at trial t decodes with the id (utterance, p, t) and is vocoded with (utterance, p),
        passed to the models as `streams=[...]` (HipRuntime) -- so with a `seed` the audio does not depend on batching."""
        kwargs = self._resolve_embeddings(kwargs)
        text = _input_text(text)                                     # get_text_from_paragraph (tacotron2.py:369-370)
        callbacks = _as_callbacks(callbacks)
        if _is_cached(text, predicted, overwrite):
            return _replay(text, predicted, callbacks)
        decode, vocode, finish = _stage_kwargs(kwargs)
        part, = self._synthesize([text], [utterance], 1, **decode)
        return self._finish(part, *self._vocode_parts(part, utterance, **vocode), callbacks=callbacks, predicted=predicted,
                            return_output=return_output, **finish)

    def _resolve_embeddings(self, kwargs):
        """The keywords of a call with `embeddings` resolved to what the synthesizer takes; a resolved vector passes through
        unchanged, so a path that resolved once per call can hand its keywords to `infer`.  Here: nothing to resolve."""
        return kwargs

    def teacher_forced(self, text, mel=None, audio=None, *, deterministic=True, **load_kwargs):
        """The model's mel for exactly the frames of a recording of `text` (Tacotron2.call, teacher forced): `mel` [F, 80]
        is the target, or `audio` (a file name or a waveform) goes through `audio.load_mel` on the model's engine with
        `load_kwargs`; `embeddings=`: the speaker, as for `infer`.  Returns {'text', 'cleaned', 'mel' [F, 80] (ground-truth
        aligned), 'decoder_output' [F, 80], 'stop_tokens' [F], 'attention' [F, Tin], 'durations' [Tin] (frames per token,
        summing to F)}.  Needs a runtime with `tacotron2_forward` (HipRuntime) behind the model."""
        load_kwargs = dict(self._resolve_embeddings(load_kwargs))
        embeddings = load_kwargs.pop('embeddings', None)
        forward = getattr(self.compiled_infer, 'tacotron2_forward', None)
        if forward is None:
            raise ValueError('teacher_forced needs a runtime with tacotron2_forward (HipRuntime) behind the model')
        if (mel is None) == (audio is None):
            raise ValueError('pass exactly one of mel and audio')
        mel = self._recording_mel(mel, audio, load_kwargs)
        cleaned = self.clean_text(text)
        tokens = np.asarray(self.encode_text(cleaned, cleaned=True), dtype=np.int32)
        if tokens.size == 0:
            raise ValueError('the text encodes to no token')
        mel_input = shift_mel_target(mel)
        n = mel_input.shape[0]
        inputs = tokens[None] if embeddings is None else (tokens[None], np.asarray(embeddings, np.float32)[None])
        out = forward(inputs, mel_input[None], np.asarray([n], np.int32), deterministic=deterministic)
        attention = _to_numpy(out.attention_weights)[0, :n]
        return {'text': text, 'cleaned': cleaned, 'mel': _to_numpy(out.mel)[0, :n],
                'decoder_output': _to_numpy(out.decoder_output)[0, :n], 'stop_tokens': _to_numpy(out.stop_tokens)[0, :n],
                'attention': attention, 'durations': attention_durations(attention, n)}

    def _recording_mel(self, mel, audio, load_kwargs):
        """The target of a teacher-forced pass as float32 [F, 80]: `mel` itself, or `audio` (a file name or a waveform) through
        `audio.load_mel` on the model's engine with `load_kwargs`."""
        if mel is None:
            from .audio import load_mel
            mel = load_mel(audio, engine=getattr(self.compiled_infer, 'engine', None), **load_kwargs)
        mel = np.asarray(_to_numpy(mel), dtype=np.float32)
        if mel.ndim == 3 and mel.shape[0] == 1:
            mel = mel[0]
        return mel

    def evaluate(self, items, *, batch_size=8, loss=None, deterministic=True, **load_kwargs):
        """The reference's TacotronLoss of the model on held-out recordings: `items` is a list of (text, mel [F, 80]) or
        (text, audio) pairs -- `audio`, a file name or a 1-D waveform, goes through `audio.load_mel` on the model's engine with
        `load_kwargs`, as in `teacher_forced`; `embeddings=`: the speaker, as for `infer`.  Every item is prepared as the
        reference's `prepare_data` does (models/tts/tacotron2.py:243-259: target = the mel, input = `shift_mel_target(mel)`,
        gate = zeros with a final 1); consecutive items form batches of at most `batch_size`, padded with the reference's
        padding values (`get_dataset_config`, :267-274: tokens with the blank id, mels with `self.pad_mel_value`, gates with
        1).  Each batch is one ragged `tacotron2_forward` and one `tacotron2_loss` on its outputs, which stay on the GPU: only
        the [K, B] result comes back.  `loss`: a `losses.TacotronLoss` (default: its defaults).  Returns {'names': its
        output_names, 'per_item': float32 [K, N] in input order, 'mean': {name: float}}.  Needs a runtime with
        `tacotron2_forward` and `tacotron2_loss` (HipRuntime) behind the model."""
        from .losses import TacotronLoss, mean_losses
        load_kwargs = dict(self._resolve_embeddings(load_kwargs))
        embeddings = load_kwargs.pop('embeddings', None)
        runtime = self.compiled_infer
        if getattr(runtime, 'tacotron2_forward', None) is None or getattr(runtime, 'tacotron2_loss', None) is None:
            raise ValueError('evaluate needs a runtime with tacotron2_forward and tacotron2_loss (HipRuntime) behind the model')
        loss = loss or TacotronLoss()
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f'batch_size must be at least 1, got {batch_size}')
        prepared = []
        for i, item in enumerate(items):
            if not isinstance(item, (tuple, list)) or len(item) != 2:
                raise ValueError(f'items[{i}] must be a (text, mel) or (text, audio) pair')
            text, recording = item
            is_mel = not isinstance(recording, str) and len(getattr(recording, 'shape', ())) >= 2
            mel = self._recording_mel(recording if is_mel else None, None if is_mel else recording, load_kwargs)
            tokens = np.asarray(self.encode_text(self.clean_text(text), cleaned=True), dtype=np.int32)
            if tokens.size == 0:
                raise ValueError(f'items[{i}]: the text encodes to no token')
            prepared.append((tokens, mel, shift_mel_target(mel)))
        if not prepared:
            raise ValueError('evaluate needs at least one item')
        names = loss.output_names
        per_item = np.zeros((len(names), len(prepared)), dtype=np.float32)
        blank, pad = int(self.tokenizer.blank_token_idx), np.float32(self.pad_mel_value)
        for r0 in range(0, len(prepared), batch_size):
            rows = prepared[r0:r0 + batch_size]
            B, Tin, T = len(rows), max(len(t) for t, _, _ in rows), max(len(m) for _, m, _ in rows)
            tok = np.full((B, Tin), blank, dtype=np.int32)
            mel_input, target = (np.full((B, T, rows[0][1].shape[1]), pad, dtype=np.float32) for _ in range(2))
            gate = np.ones((B, T), dtype=np.float32)
            for r, (tokens, mel, shifted) in enumerate(rows):
                tok[r, :len(tokens)], mel_input[r, :len(mel)], target[r, :len(mel)], gate[r, :len(mel) - 1] = tokens, shifted, mel, 0.
            inputs = tok if embeddings is None else (tok, np.repeat(np.asarray(embeddings, np.float32)[None], B, axis=0))
            out = runtime.tacotron2_forward(inputs, mel_input, np.asarray([len(m) for _, m, _ in rows], np.int32),
                                            deterministic=deterministic, on_device=True)
            per_item[:, r0:r0 + B] = _to_numpy(loss([target, gate], out, engine=runtime))
        return {'names': names, 'per_item': per_item, 'mean': mean_losses(names, per_item)}

    SYNTHESIS_NAMES = ['mcd_dtw', 'path_len', 'frames', 'target_frames', 'frame_ratio', 'stopped']

    SYNTHESIS_F0_NAMES = ['f0_rmse_cents', 'vuv_error', 'gross_error', 'voiced_pairs']

    def evaluate_synthesis(self, items, *, batch_size=8, max_length=10., n_cep=13, deterministic=True, vocoder=None, pitch=None,
                           f0_method='yin', f0_config=None, **load_kwargs):
        """The model as it is used -- free-running, through its own stop token and attention -- against held-out recordings:
        mel-cepstral distortion along the DTW path (`metrics`, tts_hip_mel_dtw) of every synthesized mel against its
        recording's.  `items` as for `evaluate`: (text, mel [F, 80]) or (text, audio) pairs; `embeddings=`: the speaker.
        Consecutive items form batches of at most `batch_size`: one call of the model's runtime on the 0-padded tokens
        (`max_length` as for `infer`: a float is frames per token of the longest row), then one `mel_dtw` of the returned mel
        against the targets padded with `self.pad_mel_value`, with the rows' `lengths` and the targets' frame counts as the
        length tables.  The mels stay on the GPU: only the lengths and the [3, B] result come to the host.  A row the model
        gave 0 frames is left out of the DTW call and of the means: mcd_dtw, path_len and frame_ratio NaN, frames 0, stopped 1.
        Returns {'names': SYNTHESIS_NAMES, 'per_item': float32 [6, N] in input order, 'mean': {name: float} over the rows that
        produced frames}; `stopped` is 1 where the row ended by its stop token before the batch's frame cap.  Needs a runtime
        with `mel_dtw` (HipRuntime) behind the model.
        `vocoder` (a `WaveGlow` wrapper; default None: names and values as above): intonation as well.  Every item must then be
        (text, audio) -- a (text, mel) item raises, there is no recording to track; the recording is loaded once
        (`audio.load_audio` with `load_kwargs`, `stft_fn` aside) and its mel taken from those samples.  The batch's mels are vocoded in one ragged
        call (`vocoder.infer(mel, lengths=frames)`), `pitch` (tts_hip_pitch; `pitch`: its keywords, the hop stays 256 so that
        the tracks share the mels' frames) runs on the vocoded and on the recorded audio, the DTW call also returns its path,
        and `f0_error` along that path appends SYNTHESIS_F0_NAMES: the F0 RMSE of the voiced pairs in cents, the voicing error
        rate (of the pairs), the gross pitch error rate (of the voiced pairs; 0 without any) and the voiced pairs.  Audio,
        tracks and path stay on the GPU; it needs `pitch` and `f0_error` on the runtime as well.  `f0_method='pyin'` tracks both
        with `pyin` (tts_hip_pyin) in place of `pitch`; `f0_config`: the tracker's keywords, on top of `pitch=`."""
        from .pitch import F0_METHODS, track_f0
        if f0_method not in F0_METHODS:
            raise ValueError(f'evaluate_synthesis: f0_method must be one of {F0_METHODS}, got {f0_method!r}')
        load_kwargs = dict(self._resolve_embeddings(load_kwargs))
        embeddings = load_kwargs.pop('embeddings', None)
        runtime = self.compiled_infer
        if getattr(runtime, 'mel_dtw', None) is None or not callable(runtime):
            raise ValueError('evaluate_synthesis needs a runtime with mel_dtw (HipRuntime) behind the model')
        pitch = dict(pitch or {}, **(f0_config or {}))
        if vocoder is not None:
            tracker = 'pitch' if f0_method == 'yin' else 'pyin'
            if getattr(runtime, tracker, None) is None or getattr(runtime, 'f0_error', None) is None:
                raise ValueError(f'evaluate_synthesis(vocoder=) needs a runtime with {tracker} and f0_error (HipRuntime) behind the model')
            if int(pitch.get('hop', 256)) != 256:
                raise ValueError(f"evaluate_synthesis: the pitch tracks share the mels' frames, hop must stay 256, got {pitch['hop']!r}")
        elif pitch:
            raise ValueError('evaluate_synthesis: pitch= configures the tracker of vocoder=, which is None')
        elif f0_method != 'yin':
            raise ValueError('evaluate_synthesis: f0_method= chooses the tracker of vocoder=, which is None')
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f'batch_size must be at least 1, got {batch_size}')
        prepared, waves = [], []
        for i, item in enumerate(items):
            if not isinstance(item, (tuple, list)) or len(item) != 2:
                raise ValueError(f'items[{i}] must be a (text, mel) or (text, audio) pair')
            text, recording = item
            is_mel = not isinstance(recording, str) and len(getattr(recording, 'shape', ())) >= 2
            if vocoder is not None and is_mel:
                raise ValueError(f'items[{i}] is a (text, mel) pair: with vocoder= the pitch of the recording is tracked, pass (text, audio)')
            if vocoder is not None:
                # loaded once, with the waveform's keywords only; the mel is that of these very samples, taken as they are
                from .audio import load_audio
                audio_kwargs = {k: v for k, v in load_kwargs.items() if k != 'stft_fn'}
                wave = load_audio(recording, self.rate, engine=getattr(runtime, 'engine', None), **audio_kwargs)
                wave = np.asarray(_to_numpy(wave), dtype=np.float32).reshape(-1)
                waves.append(wave)
                mel_kwargs = {'stft_fn': load_kwargs['stft_fn']} if load_kwargs.get('stft_fn') is not None else {}
                mel = self._recording_mel(None, wave, dict(mel_kwargs, normalize=False))
            else:
                mel = self._recording_mel(recording if is_mel else None, None if is_mel else recording, load_kwargs)
            tokens = np.asarray(self.encode_text(self.clean_text(text), cleaned=True), dtype=np.int32)
            if tokens.size == 0:
                raise ValueError(f'items[{i}]: the text encodes to no token')
            prepared.append((tokens, mel))
        if not prepared:
            raise ValueError('evaluate_synthesis needs at least one item')
        names = self.SYNTHESIS_NAMES + (self.SYNTHESIS_F0_NAMES if vocoder is not None else [])
        per_item = np.full((len(names), len(prepared)), np.nan, dtype=np.float32)
        pad = np.float32(self.pad_mel_value)
        for r0 in range(0, len(prepared), batch_size):
            rows = prepared[r0:r0 + batch_size]
            B, Tin, T = len(rows), max(len(t) for t, _ in rows), max(len(m) for _, m in rows)
            tok = np.zeros((B, Tin), dtype=np.int32)
            target = np.full((B, T, rows[0][1].shape[1]), pad, dtype=np.float32)
            for r, (tokens, mel) in enumerate(rows):
                tok[r, :len(tokens)], target[r, :len(mel)] = tokens, mel
            inputs = tok if embeddings is None else (tok, np.repeat(np.asarray(embeddings, np.float32)[None], B, axis=0))
            out = runtime(inputs, max_length=max_length, deterministic=deterministic, on_device=True)
            frames = np.asarray(_to_numpy(out.lengths), dtype=np.int64).reshape(B)
            wanted = np.asarray([len(m) for _, m in rows], dtype=np.int64)
            cap = int(out.mel.shape[1])
            block = per_item[:, r0:r0 + B]
            block[2], block[3], block[5] = frames, wanted, frames < cap
            keep = np.flatnonzero(frames > 0)
            if keep.size and vocoder is not None:
                mel = out.mel if keep.size == B else out.mel[keep.tolist()]
                la, lb = frames[keep].astype(np.int32), wanted[keep].astype(np.int32)
                stats, path = runtime.mel_dtw(mel, target if keep.size == B else target[keep], la, lb, n_cep=n_cep, return_path=True)
                stats = _to_numpy(stats)
                block[0, keep], block[1, keep], block[4, keep] = stats[2], stats[1], frames[keep] / wanted[keep]
                spoken = [waves[r0 + r] for r in keep]
                recorded = np.zeros((keep.size, max(len(w) for w in spoken)), dtype=np.float32)
                for r, w in enumerate(spoken):
                    recorded[r, :len(w)] = w
                samples = np.asarray([len(w) for w in spoken], dtype=np.int32)
                f0_syn = track_f0(runtime, f0_method, vocoder.infer(mel, lengths=la), la * 256, **pitch)[0]
                f0_rec = track_f0(runtime, f0_method, recorded, samples, **pitch)[0]
                # a recording below 1024 samples has fewer pitch frames than mel frames: the path ends where the track does
                f0 = _to_numpy(runtime.f0_error(f0_syn, f0_rec, la, np.minimum(lb, 1 + samples // 256).astype(np.int32), path))
                block[6, keep], block[9, keep] = f0[2], f0[1]
                block[7, keep] = f0[4] / np.maximum(f0[0], 1)
                block[8, keep] = f0[5] / np.maximum(f0[1], 1)
            elif keep.size:
                whole = keep.size == B                               # (no copy of the mel when every row produced frames)
                stats = _to_numpy(runtime.mel_dtw(out.mel if whole else out.mel[keep.tolist()], target if whole else target[keep],
                                                  frames[keep].astype(np.int32), wanted[keep].astype(np.int32), n_cep=n_cep))
                block[0, keep], block[1, keep], block[4, keep] = stats[2], stats[1], frames[keep] / wanted[keep]
        ok = per_item[2] > 0
        mean = {name: float(per_item[k, ok].astype(np.float64).mean()) if ok.any() else float('nan') for k, name in enumerate(names)}
        return {'names': list(names), 'per_item': per_item, 'mean': mean}

    # A text goes through four stages: `_prepare_text` (split / clean / encode), `_decode_rows` (tokens -> mels; the
    # autoregressive, latency-bound half; `_synthesize` is the two together), `_vocode_parts` or `_vocode_group` (mels ->
    # waveforms; the throughput-bound half) and `_finish` (result, cache entry, callbacks).  `infer`, `_infer_overlapped` and
    # `_infer_backlog` only decide which text is in which stage when.
    def _prepare_text(self, text, max_text_length=-1, **kwargs):
        """Split / clean / encode -> the result-dict stub of `text`, with the token arrays of its parts under `encoded`."""
        if max_text_length == -1:
            splitted = [text]
        elif max_text_length == -2:
            splitted = split_sentences(text)
        else:
            splitted = split_text(text, max_text_length)
        splitted = [self.clean_text(sent, **kwargs) for sent in splitted]
        splitted = [s for s in splitted if any(c.isalnum() for c in s)]
        if not splitted:
            splitted = ['']
        cleaned = '\n\n'.join(splitted) if len(splitted) > 1 else splitted[0]
        encoded = [self.encode_text(t, cleaned=True) for t in splitted]
        splitted = [splitted[i] for i in range(len(splitted)) if len(encoded[i]) > 0]
        encoded = [np.asarray(enc) for enc in encoded if len(enc) > 0]
        return {'text': text, 'cleaned': cleaned, 'splitted': splitted, 'mel': [], 'attention': [], 'encoded': encoded}

    def _synthesize(self, texts, utterances, k, *, embeddings=None, max_length=10., max_text_length=-1, max_trial=5,
                    min_fpt_ratio=2., max_fpt_ratio=10., **kwargs):
        """texts -> their result-dict stubs with `mel` / `attention` filled, one entry per part: the parts of all the texts
        are the rows of token batches of at most `k` rows, one `_decode_rows` each (k = 1: one part per call, the
        reference's loop).  `utterances`: the texts' numbers for per-row streams, or a None each."""
        t0 = time.time()
        parts = [self._prepare_text(text, max_text_length, **kwargs) for text in texts]
        rows = [(ti, p, enc) for ti, part in enumerate(parts) for p, enc in enumerate(part.pop('encoded'))]
        for r0 in range(0, len(rows), k):
            chunk = rows[r0:r0 + k]
            row_ids = None if utterances[0] is None else [(int(utterances[ti]), p) for ti, p, _ in chunk]
            decoded = self._decode_rows([enc for _, _, enc in chunk], row_ids, embeddings=embeddings, max_length=max_length,
                                        max_trial=max_trial, min_fpt_ratio=min_fpt_ratio, max_fpt_ratio=max_fpt_ratio, **kwargs)
            for (ti, _, _), (mel, attn) in zip(chunk, decoded):
                parts[ti]['mel'].append(mel)
                parts[ti]['attention'].append(attn)
        for part in parts:
            part['synth_time'] = (time.time() - t0) / len(parts)
        return parts

    def _decode_rows(self, tokens, row_ids, *, embeddings, max_length, max_trial, min_fpt_ratio, max_fpt_ratio, **kwargs):
        """Decodes the token arrays `tokens` as the rows of one 0-padded batch -> [(mel [n_i, 80], attention [n_i, Tin])].
        Row i ends at min(its length, the `frame_cap` it would have had alone): the runtime sizes the loop by the longest row
        (and the mel of a row cut that way gets the postnet of its own frames, on a HIP engine); for a row decoded alone the
        runtime's cap is its own.  Rows outside the frame / token window are decoded again together, up to `max_trial` times
        in all, and keep their last result.  `row_ids` [(utterance, part)] per row, or None: every call passes
        `streams=[(utterance, part, trial), ...]` for its rows; a row is in the call of trial t only after failing t times
        itself, so its own trial advances and the rows that passed are not drawn for again."""
        decoded, pending = [None] * len(tokens), list(range(len(tokens)))
        for trial in range(max_trial):
            n_tok = [len(tokens[i]) for i in pending]
            tok = np.zeros((len(pending), max(n_tok)), dtype=tokens[0].dtype)
            for r, i in enumerate(pending):
                tok[r, :n_tok[r]] = tokens[i]
            inputs = tok if embeddings is None else (tok, np.repeat(np.asarray(embeddings)[None], len(pending), axis=0))
            ids = {} if row_ids is None else {'streams': [(*row_ids[i], trial) for i in pending]}
            outputs = self.compiled_infer(inputs, max_length=max_length, **ids, **kwargs)
            lengths = _to_numpy(outputs.lengths)
            frames = [int(n) for n in lengths]
            # (a row decoded alone ends where the synthesizer says, as in the reference's loop: behind HipRuntime that is
            # within its cap already, and a synthesizer that counts its frames otherwise is not second-guessed)
            if len(pending) > 1 and max_length is not None:
                frames = [min(n, frame_cap(t, max_length)) for n, t in zip(frames, n_tok)]
            mels = {r: outputs.mel[r, :frames[r]] for r in range(len(pending))}
            # A row cut by its cap: the postnet (five k = 5 convs) of the batch saw the frames the longer loop produced behind
            # the cut, where the row alone ends.  Its last ~10 frames are computed again from the decoder output, masked there.
            cut = [r for r in range(len(pending)) if frames[r] < int(lengths[r])]
            engine = getattr(self.compiled_infer, 'engine', None)
            if cut and hasattr(engine, 'tacotron2_postnet'):
                t_cut = max(frames[r] for r in cut)
                dec = _to_numpy(outputs.decoder_output)[cut, :t_cut]
                redo = engine.tacotron2_postnet(dec, [frames[r] - 1 for r in cut])
                for j, r in enumerate(cut):
                    mels[r] = redo[j, :frames[r]]
            failed = []
            for r, i in enumerate(pending):
                decoded[i] = (mels[r], outputs.attention_weights[r, :frames[r], :n_tok[r]])
                ratio = frames[r] / n_tok[r]
                if not min_fpt_ratio < ratio < max_fpt_ratio:
                    failed.append(i)
                    logger.info('Inference failed (lengths : %s, frame/token ratio : %.2f) !', lengths[r:r + 1], ratio)
            pending = failed
            if not pending:
                break
        for _ in pending:
            logger.warning('Inference failed too much time ! Result is probably not perfect')
        return decoded

    def _vocode_parts(self, part, utterance=None, *, vocoder=None, vocoder_config={}, **kwargs):
        """One vocoder call per part of one text, on its 2-D mel -> (the waveforms of the text's non-empty parts, in order;
        None without a vocoder, seconds spent)."""
        if vocoder is None:
            return None, 0.
        t1 = time.time()
        audios = []
        for p, mel in enumerate(part['mel']):
            if mel.shape[0] > 0:
                ids = {} if utterance is None else {'streams': [(int(utterance), p)]}
                audio = vocoder(mel, **ids, **{**kwargs, **vocoder_config})
                if len(audio.shape) == 2:
                    audio = audio[0]
                audios.append(_to_numpy(audio))
        return audios, time.time() - t1

    def _vocode_group(self, parts, utterances, *, vocoder=None, vocoder_config={}, packed=False, **kwargs):
        """ONE vocoder call for all the non-empty parts of several texts, as the rows of a 0-padded batch with `lengths` =
        their frame counts (`packed`: the call also gets `packed=True`), so every waveform is that of its own frames ->
        (per text what `_vocode_parts` gives, seconds spent)."""
        if vocoder is None:
            return [None] * len(parts), 0.
        t1 = time.time()
        audios = [[] for _ in parts]
        voiced = [(ti, p, _to_numpy(mel)) for ti, part in enumerate(parts) for p, mel in enumerate(part['mel'])
                  if mel.shape[0] > 0]
        if voiced:
            n_frames = np.asarray([m.shape[0] for _, _, m in voiced], np.int32)
            batch = np.zeros((len(voiced), int(n_frames.max()), voiced[0][2].shape[1]), np.float32)
            for r, (_, _, m) in enumerate(voiced):
                batch[r, :m.shape[0]] = m
            ragged = {'packed': True} if packed else {}
            ids = {} if utterances[0] is None else {'streams': [(int(utterances[ti]), p) for ti, p, _ in voiced]}
            audio = _to_numpy(vocoder(batch, lengths=n_frames, **ragged, **ids, **{**kwargs, **vocoder_config}))
            for r, (ti, _, m) in enumerate(voiced):
                audios[ti].append(audio[r, :m.shape[0] * 256].copy())
        return audios, time.time() - t1

    def _clean_waveform(self, audio, vocoder, reduce_noise, trim_silence):
        """The reference's waveform clean-up (audio_processing.reduce_noise, trim_silence) at self.rate: `trim_silence` True is
        method 'window' with its defaults, a non-empty dict holds the keywords of `audio.trim_silence` (e.g. {'method': 'rms',
        'mode': 'remove'}, which also shortens the pauses inside the utterance); an empty dict, like False, trims nothing.
        It runs on the engine of the vocoder that produced `audio` (the synthesizer's only when the vocoder has none).  With
        `predict(..., overlap=True)` the synthesizer's handle is busy in the producer thread, and calls on one handle must
        be serialised, so the clean-up has to stay on the vocoder's handle, in the thread that vocodes."""
        eng = getattr(getattr(vocoder, 'compiled_infer', None), 'engine', None) or getattr(self.compiled_infer, 'engine', None)
        if eng is None or not hasattr(eng, 'reduce_noise'):
            raise ValueError('reduce_noise / trim_silence need a HIP engine behind the model')
        audio = np.asarray(audio, np.float32)
        if reduce_noise:
            audio = eng.reduce_noise(audio, self.rate)
        if isinstance(trim_silence, dict) and trim_silence:         # {'method': 'rms', 'mode': 'remove', ...}: audio.trim_silence's keywords
            from .audio import trim_silence as trim_with_method
            audio = trim_with_method(audio, engine=eng, rate=self.rate, **trim_silence)
        elif trim_silence and not isinstance(trim_silence, dict):
            start, end = eng.trim_silence(audio, self.rate)
            audio = audio[start:end]
        return audio

    def _apply_effects(self, audio, vocoder, speed, pitch_steps, preserve_formants=False, formant_steps=0.0):
        """`speed` (tempo, `effects.time_stretch`) and then `pitch_steps` (`effects.pitch_shift`, which takes
        `preserve_formants` and `formant_steps`; without a pitch change `formant_steps` is `effects.formant_shift`) on the
        concatenated utterance, on the engine `_clean_waveform` would use.  All must be finite; the engine refuses a speed
        outside [0.25, 4] and formant steps beyond an octave."""
        from . import effects
        eng = getattr(getattr(vocoder, 'compiled_infer', None), 'engine', None) or getattr(self.compiled_infer, 'engine', None)
        if eng is None or not hasattr(eng, 'time_stretch'):
            raise ValueError('speed / pitch_steps need a HIP engine behind the model')
        audio = np.asarray(audio, np.float32)
        if speed != 1.0:
            audio, _ = effects.time_stretch(audio, float(speed), engine=eng)
        if formant_steps != 0.0 or (preserve_formants and pitch_steps != 0.0):
            audio = effects.pitch_shift(audio, float(pitch_steps), engine=eng, preserve_formants=bool(preserve_formants),
                                        formant_steps=float(formant_steps))
        elif pitch_steps != 0.0:
            audio = effects.pitch_shift(audio, float(pitch_steps), engine=eng)
        return audio

    def _finish(self, part, audios, vocoder_time, *, callbacks=None, predicted=None, return_output=True, vocoder=None,
                silence_time=0.15, reduce_noise=False, trim_silence=False, speed=1.0, pitch_steps=0.0, preserve_formants=False,
                formant_steps=0.0):
        """The last stage: `audios` (the waveforms of the text's non-empty parts, in order; None without a vocoder) ->
        concatenation, `speed` / `pitch_steps` / `preserve_formants` / `formant_steps` (`_apply_effects`; the defaults 1.0,
        0.0, False and 0.0 call nothing, and `preserve_formants` alone changes nothing), clean-up, result dict ('time' is the
        duration after them), `predicted` entry, callbacks, return value.  Like the other keywords of this stage, `speed`,
        `pitch_steps`, `preserve_formants` and `formant_steps` are not part of the `map.json` key: a cached text is replayed
        as it was first made."""
        text, synth_time = part['text'], part.get('synth_time', 0.)
        audio_infos = {}
        if vocoder is not None:
            if len(audios) > 0:
                audios = audios[0] if len(audios) == 1 else np.concatenate(audios, axis=0)
                if (speed != 1.0 or pitch_steps != 0.0 or formant_steps != 0.0) and len(audios) > 0:
                    audios = self._apply_effects(audios, vocoder, speed, pitch_steps, preserve_formants, formant_steps)
                if (reduce_noise or trim_silence) and len(audios) > 0:
                    audios = self._clean_waveform(audios, vocoder, reduce_noise, trim_silence)
                audio_infos = {'audio': audios, 'rate': self.rate, 'time': len(audios) / self.rate}
                logger.info('%.2f s generated in %.3f s (%.3f synthesizer + %.3f vocoder)', audio_infos['time'],
                            synth_time + vocoder_time, synth_time, vocoder_time)
            else:
                audio_infos = {'audio': np.zeros((int(silence_time * self.rate),), dtype='float32'),
                               'rate': self.rate, 'time': silence_time}
        output = {k: part[k] for k in ('text', 'cleaned', 'splitted', 'mel', 'attention')}
        output.update(audio_infos)
        if callbacks:
            if predicted is None:
                predicted = {}
            if text not in predicted:
                predicted[text] = {k: v for k, v in output.items() if k not in ('mel', 'attention', 'audio')}
            apply_callbacks(callbacks, predicted[text], output, save=True)
        if return_output:
            return output
        if vocoder is None or 'audio' in (predicted or {}).get(text, {}):
            return (predicted or {}).get(text, {})
        return {k: v for k, v in output.items() if k not in ('mel', 'attention')}

    def get_inference_callbacks(self, *, vocoder=None, save=None, save_mel=None, save_audio=None, directory=None,
                                mel_dir=None, audio_dir=None, mel_filename='mel-{}.npy',
                                audio_filename=None, post_processing=None, **_):
        """(predicted, callbacks) with the reference's flag resolution (tacotron2.py:276-352): results are saved when a
        `directory` is given or there is no vocoder; mels only without a vocoder; `map.json` in `directory` is both the
        cache that `infer` consults and the index the JSON saver rewrites."""
        if vocoder is None:
            save_audio = False
        elif save_audio is None:
            save_audio = save is not False
        if save is None:
            save = bool(directory) or vocoder is None
        if save_mel is None:
            save_mel = save and vocoder is None
        save = bool(save_mel or save_audio)                        # (sic: with a vocoder, audio is saved unless save=False)
        if vocoder is not None and save:
            save_audio = True
        predicted, callbacks = {}, []
        if save:
            if directory is None:
                directory = self.pred_dir
            os.makedirs(directory, exist_ok=True)
            map_file = os.path.join(directory, 'map.json')
            predicted = load_json(map_file, {})
            if save_mel:
                callbacks.append(SpectrogramSaver(file_format=os.path.join(mel_dir or os.path.join(directory, 'mels'),
                                                                           mel_filename)))
            if save_audio:
                callbacks.append(AudioSaver(file_format=os.path.join(audio_dir or os.path.join(directory, 'audios'),
                                                                     audio_filename or default_audio_format())))
            callbacks.append(JSONSaver(data=predicted, filename=map_file, primary_key='text'))
        if post_processing is not None:
            for fn in (post_processing if isinstance(post_processing, list) else [post_processing]):
                if callable(fn):
                    callbacks.append(FunctionCallback(fn))
                elif hasattr(fn, 'put'):
                    callbacks.append(QueueCallback(fn))
        return predicted, callbacks

    _callback_kwargs = ('save', 'save_mel', 'save_audio', 'directory', 'mel_dir', 'audio_dir', 'mel_filename',
                        'audio_filename', 'post_processing')

    def predict(self, inputs, *, predicted=None, callbacks=None, return_results=True, return_output=None,
                overlap=False, batch_backlog=None, pack_vocoder=False, sentence_streams=False, **kwargs):
        """BaseModel.predict (base_model.py:676-711): builds the callbacks unless the caller brings its own `predicted`
        map, then runs `infer` sequentially; returns the result dicts (or the `predicted` entries when a JSON saver is
        active and `return_output` was not forced).
        `batch_backlog=k` (k >= 2): inputs that are already waiting are synthesized together -- the next input plus up to
        k - 1 more that a `queue.Queue` holds right now (a list / iterator: its next items) are decoded as the rows of one
        token batch and vocoded in one call with per-row lengths (`_infer_backlog`); a lone input takes the batch-1 path, so
        nothing waits for a batch to fill.  Results, callbacks and the `predicted` map see the inputs in their order, as in
        the sequential loop.  With `deterministic=True` the audio is the sequential loop's up to fp32 re-association in the
        decoder; otherwise dropout masks and noise are drawn from the runtime's stream in the batch's layout: the same
        distribution, another realisation than the sequential loop's.  Not combined with `overlap=True`.
        `pack_vocoder=True` (needs `batch_backlog >= 2`): the group's one vocoder call gets `packed=True` -- the same audio,
        computed on the frames that exist instead of rows x longest row (HipEngine.waveglow_infer).
        `sentence_streams=True`: every input taken from `inputs` gets the next utterance number (from 0; a text served from
        the cache consumes one too, so grouping cannot shift later sentences) and all its random draws come from streams of
        its own (`infer(utterance=...)`): with a `seed`, a sentence's dropout masks and noise -- and so its audio, up to fp32
        re-association between the decoder machines and vocoder layouts -- are the same in the sequential loop, with
        `overlap=True`, and in any `batch_backlog` grouping (packed or not), from run to run."""
        backlog = batch_backlog is not None and int(batch_backlog) >= 2
        if pack_vocoder and not backlog:
            raise ValueError('pack_vocoder=True needs batch_backlog >= 2 (it packs the vocoder call of a backlog group)')
        if batch_backlog is not None and int(batch_backlog) < 1:
            raise ValueError(f'batch_backlog must be None or >= 1, got {batch_backlog!r}')
        if backlog and overlap:
            raise ValueError('batch_backlog and overlap=True cannot be combined')
        if isinstance(inputs, (str, dict)):
            inputs = [inputs]
        elif isinstance(inputs, _queue.Queue) and not backlog:
            inputs = _iterate(inputs)
        join_callbacks = predicted is None
        if predicted is None:
            predicted, built = self.get_inference_callbacks(**kwargs)
            callbacks = built + _as_callbacks(callbacks)
        else:
            callbacks = _as_callbacks(callbacks)
        if return_output is None:
            return_output = not any(isinstance(cb, JSONSaver) for cb in callbacks)
        kwargs = {k: v for k, v in kwargs.items() if k not in self._callback_kwargs}
        run = dict(predicted=predicted, callbacks=callbacks, return_output=return_output)
        results = []
        if backlog:                                                # (these two resolve the speaker once per call, `infer` per text)
            outputs = self._infer_backlog(inputs, int(batch_backlog), pack_vocoder=bool(pack_vocoder),
                                          sentence_streams=bool(sentence_streams), **run, **self._resolve_embeddings(kwargs))
        elif overlap and kwargs.get('vocoder') is not None:
            outputs = self._infer_overlapped(inputs, sentence_streams=bool(sentence_streams), **run,
                                             **self._resolve_embeddings(kwargs))
        else:
            outputs = ((inp, self.infer(inp, utterance=n if sentence_streams else None, **run, **kwargs))
                       for n, inp in enumerate(inputs))
        for inp, output in outputs:
            if return_results:
                results.append(output if return_output else predicted[_input_text(inp)])
        if join_callbacks:
            for cb in callbacks:
                cb.join()
        return results

    def _infer_overlapped(self, inputs, *, predicted, callbacks, return_output, overwrite=False, sentence_streams=False,
                          **kwargs):
        """Sentence-level software pipeline: a worker thread runs `_synthesize` for the next input while this thread
        vocodes the previous one.  The synthesizer and the vocoder must sit on different engine handles (two HIP streams;
        calls on one handle are serialised) -- `get_models(..., overlap=True)` builds such a pair.  Measured on MI355X
        (scripts/overlap_probe.py, 600-frame sentences): 39.2 -> 34.6 ms per sentence with the fp16 vocoder, 87.8 -> 78.5 ms
        in fp32; the decoder's launches only get CU slots as WN GEMM blocks retire, so it runs 2.4x / 5.6x slower while a
        vocoder call is in flight, but that time was idle before.  Results keep the input order."""
        import threading
        decode, vocode, finish = _stage_kwargs(kwargs)
        q = _queue.Queue(maxsize=2)
        DONE = object()

        def producer():
            try:
                for n, inp in enumerate(inputs):
                    text, number = _input_text(inp), n if sentence_streams else None
                    part = None                                       # a cached text: the consumer replays it in its turn
                    if not _is_cached(text, predicted, overwrite):
                        part, = self._synthesize([text], [number], 1, **decode)
                    q.put((inp, text, number, part, None))
            except BaseException as exc:                              # noqa: BLE001 -- re-raised in the consumer
                q.put((None, None, None, None, exc))
            finally:
                q.put(DONE)

        th = threading.Thread(target=producer, name='tacotron2-synth', daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is DONE:
                    break
                inp, text, number, part, exc = item
                if exc is not None:
                    raise exc
                if part is None:
                    yield inp, _replay(text, predicted, callbacks)
                else:
                    yield inp, self._finish(part, *self._vocode_parts(part, number, **vocode), callbacks=callbacks,
                                            predicted=predicted, return_output=return_output, **finish)
        finally:
            while th.is_alive():                                      # drain so that the producer can finish
                try:
                    q.get(timeout=0.05)
                except _queue.Empty:
                    pass
            th.join()

    def _infer_backlog(self, inputs, k, *, predicted, callbacks, return_output, overwrite=False, pack_vocoder=False,
                       sentence_streams=False, **kwargs):
        """`predict(batch_backlog=k)`: yields (input, result) in input order.  Per group of waiting inputs (`_backlog_groups`):
        the parts of all its texts are the rows of 0-padded token batches of at most k rows, one `compiled_infer` call each;
        every row keeps the frame cap, the frame / token ratio test and the retries it would have had alone (rows that fail
        are decoded again together); ONE vocoder call per group (`_vocode_group`); then each text is finished (`_finish`) in
        input order.  A group with at most one text to synthesize takes `infer`, cache replays included.
        `sentence_streams`: inputs are numbered as the groups take them from the source; the row of part p of utterance n
        decodes with the id (n, p, trial) -- a retried row keeps its id and advances only its own trial -- and is vocoded
        with (n, p), exactly as the sequential path does."""
        decode, vocode, finish = _stage_kwargs(kwargs)
        run = dict(predicted=predicted, callbacks=callbacks, return_output=return_output)
        is_cached = lambda text: _is_cached(text, predicted, overwrite)
        taken = 0
        for group in _backlog_groups(inputs, k, is_cached):
            number = {text: taken + j if sentence_streams else None for j, (_, text) in enumerate(group)}
            taken += len(group)                                   # (a group never holds a text twice)
            fresh = [text for _, text in group if not is_cached(text)]
            if len(fresh) <= 1:
                for inp, text in group:
                    yield inp, self.infer(inp, utterance=number[text], overwrite=overwrite, **run, **kwargs)
                continue
            numbers = [number[text] for text in fresh]
            parts = self._synthesize(fresh, numbers, k, **decode)
            audios, vocoder_time = self._vocode_group(parts, numbers, packed=pack_vocoder, **vocode)
            done = dict(zip(fresh, zip(parts, audios)))
            for inp, text in group:                               # input order: cache replays between the fresh texts
                if text in done:
                    yield inp, self._finish(*done[text], vocoder_time / len(fresh), **run, **finish)
                else:
                    yield inp, _replay(text, predicted, callbacks)

    def precompile_for_stream(self, **kwargs):
        for m in (64, 128):                                    # tacotron2.py:354-356 (warm-up of both shape buckets)
            self.infer('hello {}'.format(m), max_trial=1, padding_multiple=m, **kwargs)

    def stream(self, stream, *, vocoder, **kwargs):
        """`predict(return_output=False, return_results=False)` over an iterable or a `queue.Queue` (None ends it);
        results leave through the callbacks (tacotron2.py:363-367, base_model.py:713)."""
        self.precompile_for_stream(vocoder=vocoder, **{k: v for k, v in kwargs.items()
                                                       if k not in self._callback_kwargs + ('callbacks', 'predicted', 'overlap',
                                                                                            'batch_backlog', 'pack_vocoder',
                                                                                            'sentence_streams')})
        kwargs.setdefault('return_output', False)
        kwargs.setdefault('return_results', False)
        # batch_backlog looks at what the queue holds right now, so `predict` gets the queue itself
        return self.predict(stream, vocoder=vocoder, **kwargs)


# ---- multi-speaker wrapper (models/tts/sv2tts_tacotron2.py:18-128, utils/embeddings.py:249-286) --------------------------
def select_embedding(embeddings, mode='random', **filters):
    """One speaker embedding (1-D) out of a collection: a 2-D array, a 1-D array (a collection of one) or a pandas
    DataFrame with an 'embedding' column (then `filters` on other columns narrow the choice; no match = no filter, with a
    warning).  mode: an int (row), 'mean' / 'avg' / 'average', 'random' (Python's `random`, like the reference) or a
    callable taking the [n, E] array."""
    import random
    if hasattr(embeddings, 'columns'):
        rows = embeddings
        used = {k: v for k, v in filters.items() if k in embeddings.columns}
        if used:
            keep = np.ones(len(embeddings), dtype=bool)
            for col, want in used.items():
                vals = embeddings[col]
                keep &= np.asarray(vals.isin(list(want)) if isinstance(want, (list, tuple, set)) else vals == want)
            if keep.any():
                rows = embeddings[keep]
            else:
                logger.warning('No embedding respect filters %s', filters)
        pool = np.stack([np.asarray(e, dtype=np.float32) for e in rows['embedding'].values])
    else:
        pool = _to_numpy(embeddings)
        if pool.ndim == 1:
            pool = pool[None]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool):
        return pool[mode]
    if callable(mode):
        return mode(pool)
    if mode in ('mean', 'avg', 'average'):
        return pool.mean(axis=0)
    if mode == 'random':
        return pool[random.randrange(len(pool))]
    raise ValueError("Unknown embedding selection mode !\n  Accepted : {}\n  Got : {}".format(
        "(int, callable, 'mean', 'random')", mode))


class SV2TTSTacotron2(Tacotron2):
    """Tacotron2 conditioned on a speaker embedding (encoder output 512 + `embedding_dim`).  `infer(text, embeddings=...)`
    takes the vector itself, or a selector resolved against the model's collection (`self.embeddings`): None -> the default
    mode ('mean' when `use_label_embedding`, else 'random'), an int -> that row, a str -> that mode, a dict ->
    `select_embedding(**dict)`; the reference's default is `embeddings=0`, the first row."""

    def __init__(self, compiled_infer, lang='fr', *, embeddings=None, embeddings_dir=None, embedding_dim=256,
                 use_label_embedding=False, encoder_name=None, **kwargs):
        super().__init__(compiled_infer, lang=lang, **kwargs)
        # `embeddings`: the collection itself (matrix / DataFrame) or a file of one (csv / npy / pkl / the reference's h5);
        # `embeddings_dir`: the model's `<name>/embeddings` directory, searched like sv2tts_tacotron2.py:53-67 (the only
        # file in it, else `embeddings.<ext>`)
        if embeddings is None and embeddings_dir is not None and os.path.isdir(embeddings_dir):
            found = sorted(os.listdir(embeddings_dir))
            embeddings = os.path.join(embeddings_dir, found[0] if len(found) == 1 else 'embeddings')
        if isinstance(embeddings, str):
            from .embeddings import load_embeddings
            embeddings = load_embeddings(embeddings)
        self.embeddings = embeddings
        self.embedding_dim = embedding_dim
        self.use_label_embedding = use_label_embedding
        self.encoder_name = encoder_name

    def select_embedding(self, embeddings=None, mode=None):
        if not hasattr(embeddings, 'shape'):                     # a selector, not data
            if mode is None:
                mode = embeddings
            embeddings = self.embeddings
        if embeddings is None:
            raise ValueError('this model has no speaker embeddings: pass `embeddings=<vector>` or set `model.embeddings`')
        if mode is None:
            mode = {'mode': 'mean' if self.use_label_embedding else 'random'}
        elif not isinstance(mode, dict):
            mode = {'mode': mode}
        vec = np.asarray(select_embedding(embeddings, **mode), dtype=np.float32)
        if vec.shape != (self.embedding_dim,):
            raise ValueError(f'speaker embedding must have shape ({self.embedding_dim},), got {vec.shape}')
        return vec

    def _resolve_embeddings(self, kwargs):
        embeddings = kwargs.get('embeddings', 0)
        if embeddings is None or isinstance(embeddings, (int, str, dict)):       # a selector, not the vector itself
            embeddings = self.select_embedding(embeddings)
        return {**kwargs, 'embeddings': embeddings}


def _as_callbacks(callbacks):
    """Accepts Callback instances, plain callables (called with the merged entry + result as keyword arguments, like the
    reference's `post_processing` functions) and queues."""
    if not callbacks:
        return []
    out = []
    for cb in callbacks:
        if isinstance(cb, Callback):
            out.append(cb)
        elif hasattr(cb, 'put'):
            out.append(QueueCallback(cb))
        elif callable(cb):
            out.append(FunctionCallback(cb))
        else:
            raise TypeError(f'unsupported callback {cb!r}')
    return out


def _iterate(stream):
    if isinstance(stream, _queue.Queue):
        while True:
            item = stream.get()
            if item is None:
                return
            yield item
    else:
        yield from stream


def _input_text(inp):
    return inp['text' if 'text' in inp else 'content'] if isinstance(inp, dict) else inp


def _is_cached(text, predicted, overwrite):
    return bool(predicted) and not overwrite and text in predicted


def _replay(text, predicted, callbacks):
    """A cached text: its entry goes through the callbacks again, nothing is re-saved, and is the result."""
    if callbacks:
        apply_callbacks(callbacks, predicted[text], {}, save=False)
    return predicted[text]


_SYNTHESIZE_KWARGS = ('embeddings', 'max_length', 'max_text_length', 'max_trial', 'min_fpt_ratio', 'max_fpt_ratio')
_VOCODE_KWARGS = ('vocoder', 'vocoder_config')
_FINISH_KWARGS = ('vocoder', 'silence_time', 'reduce_noise', 'trim_silence', 'speed', 'pitch_steps', 'preserve_formants',
                  'formant_steps')


def _stage_kwargs(kwargs):
    """The keywords of `infer` / `predict`, split once -> those of (`_synthesize`, `_vocode_parts` / `_vocode_group`,
    `_finish`).  A keyword no stage names (`seed`, `deterministic`, `padding_multiple`, ...) is the models': it goes to the
    text cleaner and the synthesizer with the first set and to the vocoder with the second, as the reference hands its
    `**kwargs` on -- so a misspelt stage keyword is handed on like them, not refused.  Each stage's signature holds the
    defaults of its own keywords (`infer`'s docstring only repeats them)."""
    named = set(_SYNTHESIZE_KWARGS + _VOCODE_KWARGS + _FINISH_KWARGS)
    models = {k: v for k, v in kwargs.items() if k not in named}
    pick = lambda names: {k: kwargs[k] for k in names if k in kwargs}
    return {**models, **pick(_SYNTHESIZE_KWARGS)}, {**models, **pick(_VOCODE_KWARGS)}, pick(_FINISH_KWARGS)


def _backlog_groups(source, k, is_cached=lambda text: False):
    """Groups of [(input, text)] for `predict(batch_backlog=k)`: the next input (a `queue.Queue` is waited on, None ends
    it), then more that are waiting right now (`get_nowait`; a list / iterator: its next items) until the group holds k
    texts to synthesize.  Cached texts ride along in their place without counting; a text that already sits in the group
    closes it and opens the next one, so a repeat finds the entry its first occurrence left in the cache."""
    is_queue = isinstance(source, _queue.Queue)
    it = None if is_queue else iter(source)
    END = object()

    def take(block):
        if is_queue:
            try:
                item = source.get() if block else source.get_nowait()
            except _queue.Empty:
                return None
            return END if item is None else item
        return next(it, END)

    held = None
    while True:
        first = held if held is not None else take(True)
        held = None
        if first is END:
            return
        group, texts, n_fresh, ended = [(first, _input_text(first))], {_input_text(first)}, 0, False
        n_fresh += not is_cached(group[0][1])
        while n_fresh < k:
            item = take(False)
            if item is None:
                break
            if item is END:
                ended = True
                break
            text = _input_text(item)
            if text in texts:
                held = item
                break
            group.append((item, text))
            texts.add(text)
            n_fresh += not is_cached(text)
        yield group
        if ended:
            return


_models = {}


def get_models(path='synthetic', device=0, lang='en', overlap=False, vocoder=None, **kwargs):
    """(Tacotron2, WaveGlow) pair -- the analogue of models/tts/__init__.py:get_models.  By default both share one engine
    handle; `overlap=True` gives the vocoder its own handle (second HIP stream, second weight copy) so that
    `stream(..., overlap=True)` can run the two models concurrently.  `vocoder='griffin_lim'`: (Tacotron2, GriffinLim) on the
    synthesizer's engine -- no WaveGlow weights are needed; Griffin-Lim has no handle of its own to overlap with, so it is
    refused together with `overlap=True`."""
    from .runtime import HipRuntime, build_runtime
    from .waveglow import WaveGlow
    spk_dim = int(kwargs.get('speaker_embedding_dim', 0) or 0)
    embeddings = kwargs.pop('embeddings', None)
    if vocoder not in (None, 'griffin_lim'):
        raise ValueError(f"vocoder must be None (WaveGlow) or 'griffin_lim', got {vocoder!r}")
    if vocoder and overlap:
        raise ValueError("vocoder='griffin_lim' runs on the synthesizer's engine: overlap=True does not apply")
    key = (path, device, lang, bool(overlap), spk_dim) + ((vocoder,) if vocoder else ())
    if key not in _models and vocoder == 'griffin_lim':
        from .griffin_lim import GriffinLim
        synth = build_runtime('hip', path, model='tacotron2', device=device, **kwargs)
        model = (SV2TTSTacotron2(synth, lang=lang, embedding_dim=spk_dim, embeddings=embeddings) if spk_dim
                 else Tacotron2(synth, lang=lang))
        _models[key] = (model, GriffinLim(synth.engine))
    elif key not in _models:
        synth = build_runtime('hip', path, model='tacotron2', device=device, **kwargs)
        if overlap:
            eng = HipRuntime.load_engine(path, device=device, **kwargs)
            voc = build_runtime('hip', path, model='waveglow', engine=eng, device=device, **kwargs)
        else:
            voc = build_runtime('hip', path, model='waveglow', engine=synth.engine, device=device, **kwargs)
        model = (SV2TTSTacotron2(synth, lang=lang, embedding_dim=spk_dim, embeddings=embeddings) if spk_dim
                 else Tacotron2(synth, lang=lang))
        _models[key] = (model, WaveGlow(voc))
    elif embeddings is not None and spk_dim:
        _models[key][0].embeddings = embeddings
    return _models[key]


def _named_vocoder(model, vocoder):
    """`vocoder='griffin_lim'` beside a caller's own model: a GriffinLim on that model's engine (nothing is loaded or cached);
    everything else as it came."""
    if isinstance(vocoder, str) and vocoder == 'griffin_lim':
        engine = getattr(getattr(model, 'compiled_infer', None), 'engine', None)
        if engine is not None:
            from .griffin_lim import GriffinLim
            return GriffinLim(engine)
    return vocoder


def tts(text, *, lang='en', model=None, vocoder=None, path='synthetic', device=0, **kwargs):
    """models.tts.tts (models/tts/__init__.py:62-77): one text -> its result dict; a list of texts -> list of dicts."""
    vocoder = _named_vocoder(model, vocoder)
    if model is None or vocoder is None or isinstance(vocoder, str):
        m, v = get_models(path, device, lang, vocoder=vocoder if isinstance(vocoder, str) else None)
        model, vocoder = model or m, v if vocoder is None or isinstance(vocoder, str) else vocoder
    res = model.predict(text, vocoder=vocoder, **kwargs)
    return res[0] if isinstance(text, (str, dict)) else res


def stream(stream, *, lang='en', model=None, vocoder=None, path='synthetic', device=0, **kwargs):
    """models.tts.stream (models/tts/__init__.py:80-101); `overlap=True` pipelines Tacotron2(n + 1) with WaveGlow(n)."""
    if model is None or vocoder is None:
        m, v = get_models(path, device, lang, overlap=bool(kwargs.get('overlap', False)))
        model, vocoder = model or m, vocoder or v
    return model.stream(stream, vocoder=vocoder, **kwargs)
