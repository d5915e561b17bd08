"""Batched text -> audio pipeline that keeps the mel spectrogram on the GPU between Tacotron2 and WaveGlow.

The reference bounces every sentence through the host (`outputs.mel[0, :len]` -> numpy -> vocoder,
/root/reference/models/tts/tacotron2.py:181-189) and always runs batch 1.  Here a batch of utterances is decoded
together, the padded mel batch (pad value -11, the reference's `pad_mel_value`, models/tts/waveglow.py:27) is vocoded in
one call -- the reference's own batched path does the same (`mel.shape[0] > 1` -> direct inference, waveglow.py:108-112)
-- and only the final waveforms are copied back.  This is BASELINE.json config 3's shape (batch 8, mixed lengths).
"""
from __future__ import annotations

import numpy as np

PAD_MEL_VALUE = -11.0
RATE = 22050                        # WaveGlow's output rate (the reference's Tacotron2.rate)


class TTSPipeline:
    def __init__(self, engine, seed=None, vocoder_precision='f32', synthesizer_precision='f32', rank=None):
        from .runtime import rank_stream
        self.engine = engine
        self.vocoder_precision = vocoder_precision      # 'f16': BASELINE.json configs 3 / 5
        self.synthesizer_precision = synthesizer_precision
        self._rng = np.random.default_rng(seed)
        self._seed = int(seed) if seed is not None else int(np.random.SeedSequence().generate_state(2, np.uint32).view(np.uint64)[0])
        # one job-wide seed on every rank: each rank draws from its own key (ranks synthesize different shards; with one key
        # they would all start at offset 0 and give different utterances the same noise)
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self._job_seed = self._seed & 0xFFFFFFFFFFFFFFFF       # un-ranked: per-row streams are keyed by the utterance, not the rank
        self._seed = rank_stream(self._seed, rank)
        self._offset = 0                                # running block offset in the engine's device-side Philox stream

    def synthesize_tokens(self, tokens, speaker=None, max_length=10.0, deterministic=False, prenet_masks=None, z=None,
                          sigma=1.0, early_stopping=True, round_frames_to=8, on_device=False, reduce_noise=False,
                          trim_silence=False, ragged=False, row_ids=None):
        """tokens int32 [B, Tin] (0 = pad) -> (list of B float32 waveforms, lengths [B] in frames, steps run).
        `ragged`: the decoder's lengths go to the vocoder (HipEngine.waveglow_infer(lengths=...)) instead of a -11 fill, so
        every waveform is what its sentence gives when vocoded alone; False (default): the reference's batched path, where
        the rows shorter than the longest hear the padding in their last ~96 frames.
        `on_device`: nothing is copied to the host -- returns (audio [B, S] float32 device tensor, zero beyond each row's
        samples, sample counts [B] int64 device tensor, steps run).
        `reduce_noise` / `trim_silence`: the reference's waveform clean-up (audio_processing.reduce_noise, trim_silence with
        method 'window') on the device, each row with its own sample count as its length, at RATE Hz; trimming changes the
        lengths, so it needs host output (on_device=False).  `trim_silence` is a flag here: a dict of `audio.trim_silence`
        keywords (as `Tacotron2.infer` takes) is refused, not read as True; trim the returned rows with `audio.trim_silence`.
        `row_ids` [B] (ints, e.g. the global utterance indices `synthesize_sharded(with_ids=True)` hands a rank; excludes
        `prenet_masks`, `z` and `deterministic=True`): row b's dropout masks and noise come from streams of its own, keyed by
        `stream_key(job seed, MASK_STREAM / NOISE_STREAM, row_ids[b], 0, 0)` with the job-wide seed as given (not this rank's
        `rank_stream`); the running offset is untouched.  An utterance then draws the same values in any batch, on any rank
        and at any world size; with `ragged=True` its audio is its own as well (up to fp32 re-association), while the padded
        path (`ragged=False`) keeps hearing the batch's padding."""
        if isinstance(trim_silence, dict):
            raise ValueError('synthesize_tokens: trim_silence is a flag (method \'window\'); for another method pass the rows '
                             'to audio.trim_silence(row, engine=..., rate=..., method=...)')
        if on_device and trim_silence:
            raise ValueError('trim_silence=True needs on_device=False (trimmed rows have new lengths)')
        import torch
        from .runtime import MASK_STREAM, NOISE_STREAM, frame_cap, mask_blocks, noise_blocks, stream_key
        eng = self.engine
        dev = torch.device('cuda', eng.device)
        as_dev = lambda x, dt: (x.to(device=dev, dtype=dt) if torch.is_tensor(x)
                                else torch.as_tensor(np.asarray(x), dtype=dt).to(dev))
        tok = as_dev(tokens, torch.int32)
        B = int(tok.shape[0])
        max_len = frame_cap(int((tok != 0).sum(dim=1).max()), max_length)
        mask_rows = noise_rows = None
        if row_ids is not None:
            if prenet_masks is not None or z is not None or deterministic:
                raise ValueError('row_ids excludes prenet_masks, z and deterministic=True')
            ids = [int(i) for i in (row_ids.tolist() if hasattr(row_ids, 'tolist') else row_ids)]
            if len(ids) != B:
                raise ValueError(f'row_ids must hold one id per row ({B} rows), got {len(ids)}')
            mask_rows = ([stream_key(self._job_seed, MASK_STREAM, i) for i in ids], [0] * B)
            noise_rows = ([stream_key(self._job_seed, NOISE_STREAM, i) for i in ids], [0] * B)
        elif prenet_masks is None and not deterministic:          # drawn on the device (engine's Philox stream)
            prenet_masks = eng.random_prenet_masks(B, max_len, self._seed, self._offset)
            self._offset += mask_blocks(B, max_len)
        elif prenet_masks is not None:
            prenet_masks = as_dev(prenet_masks, torch.float32)
        if speaker is not None:
            speaker = as_dev(speaker, torch.float32)
        out = eng.tacotron2_infer(tok, speaker=speaker, max_len=max_len, early_stopping=early_stopping,
                                  prenet_masks=prenet_masks, want_attention=False,
                                  precision=self.synthesizer_precision,
                                  **({} if mask_rows is None else {'row_mask_seeds': mask_rows}))
        lengths = out.lengths.clamp(min=0)
        steps = eng.last_steps
        T = int(lengths.max())
        if T <= 0:
            if on_device:
                return torch.zeros((B, 1), dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int64, device=dev), steps
            return [np.zeros((0,), np.float32) for _ in range(B)], lengths.cpu().numpy(), steps
        if round_frames_to > 1:                         # keeps the WaveGlow workspace sizes (and M tiles) stable
            T = min(max_len, (T + round_frames_to - 1) // round_frames_to * round_frames_to)
        mel = out.mel[:, :T].clone()
        voc = {}
        if ragged:                                      # frames beyond a row's length are never read: no fill
            voc['lengths'] = lengths.to(torch.int32).cpu().numpy()
        else:
            valid = torch.arange(T, device=dev)[None, :] < lengths[:, None]
            mel = torch.where(valid[:, :, None], mel, torch.full_like(mel, PAD_MEL_VALUE))
        if noise_rows is not None:
            audio = eng.waveglow_infer(mel.contiguous(), sigma=sigma, precision=self.vocoder_precision, row_seeds=noise_rows,
                                       **voc)
        elif z is None and not deterministic:
            audio = eng.waveglow_infer(mel.contiguous(), sigma=sigma, precision=self.vocoder_precision, seed=self._seed,
                                       offset=self._offset, **voc)
            self._offset += noise_blocks(B, T)
        else:
            if z is not None:
                z = as_dev(z, torch.float32)[:, :T * 32]
            audio = eng.waveglow_infer(mel.contiguous(), z=z, sigma=sigma, precision=self.vocoder_precision, **voc)
        if reduce_noise or trim_silence:
            n_samp = np.maximum(lengths.cpu().numpy().astype(np.int64) * 256, 1)      # a row needs >= 1 sample
            if reduce_noise:
                audio = eng.reduce_noise(audio, RATE, lengths=n_samp)
            if trim_silence:
                start, end = eng.trim_silence(audio, RATE, lengths=n_samp)
        if on_device:
            counts = lengths.to(torch.int64) * 256
            keep = torch.arange(T * 256, device=dev)[None, :] < counts[:, None]
            return torch.where(keep, audio, torch.zeros_like(audio)), counts, steps
        audio_h = audio.cpu().numpy()
        n = lengths.cpu().numpy()
        if trim_silence:
            return [audio_h[b, int(start[b]):int(end[b])].copy() if n[b] > 0 else np.zeros((0,), np.float32)
                    for b in range(B)], n, steps
        return [audio_h[b, :int(n[b]) * 256].copy() for b in range(B)], n, steps

    def shard_fn(self, row_streams=False, **kwargs):
        """`row_streams=True`: a three-argument `synth_fn(local_tokens, local_speaker, ids)` for
        `synthesize_sharded(with_ids=True)` -- the global utterance indices become `synthesize_tokens(row_ids=ids)`, so an
        utterance gets the same masks and noise at every world size.  Otherwise:
        `synth_fn(local_tokens, local_speaker) -> (audio [n, S] zero padded, sample counts [n])` for
        `distributed.synthesize_sharded`: this rank's share of the utterances through `synthesize_tokens(**kwargs)`.  Both
        results are DEVICE tensors (the waveforms go from WaveGlow's output buffer straight into the RCCL gather; the only
        device-to-host copy of the job is rank 0's, after the gather)."""
        def synth(local_tokens, local_speaker):
            audio, counts, _ = self.synthesize_tokens(local_tokens, speaker=local_speaker, on_device=True, **kwargs)
            return audio, counts

        def synth_rows(local_tokens, local_speaker, ids):
            audio, counts, _ = self.synthesize_tokens(local_tokens, speaker=local_speaker, on_device=True, row_ids=ids, **kwargs)
            return audio, counts
        return synth_rows if row_streams else synth
