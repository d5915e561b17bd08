"""numpy restatement of the reference's teacher-forced pass, Tacotron2.call (TEST INFRASTRUCTURE).

Follows /root/reference/architectures/tacotron2_arch.py:806-849 (Tacotron2.call) and :526-607 (Tacotron2Decoder.call), built
from the pieces of oracle.tacotron2_ref that Tacotron2.infer's restatement is made of (encoder, prenet, lstm_cell, attention,
postnet, _sigmoid): step t reads frame t of the GIVEN mel, every row runs all T steps, no stop test and no attention window.

    mel_input [B, T, 80]   already shifted: frame 0 is the zero go-frame, frame t is target frame t - 1
                           (models/tts/tacotron2.py:243-259)
    mel_lengths [B]        each in 1 .. T; the decoder mask is t <= mel_lengths[b] (:555 -- note the <=)
    prenet_masks           None (deterministic) or [B, T, 2, 256] multiplicative masks (:188-203)

`planted` (tests only) restates one of the mistakes a device path could make, so that the tests can show their bound tells
each from the truth: 'unshifted' feeds target frame t where frame t - 1 belongs, 'mask_lt' masks with t < length, 'mask_prev'
applies the dropout mask of step t - 1.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import tacotron2_ref as ref

ForwardOutput = namedtuple('ForwardOutput', ['decoder_output', 'mel', 'stop_tokens', 'attention_weights'])


def shift(target):
    """[B, F, 80] target frames -> the decoder input: the zero go-frame, then frames 0 .. F - 2."""
    return np.concatenate([np.zeros_like(target[:, :1]), target[:, :-1]], axis=1)


def forward(tokens, mel_input, mel_lengths, w, cfg, speaker_embedding=None, prenet_masks=None, dtype=np.float32, planted=None):
    w = {k: v.astype(dtype) for k, v in w.items() if k.startswith('tacotron2/')}
    tokens = np.asarray(tokens, dtype=np.int32)
    x = np.asarray(mel_input, dtype=dtype)
    lengths = np.asarray(mel_lengths, dtype=np.int64)
    if prenet_masks is not None:
        prenet_masks = np.asarray(prenet_masks, dtype=dtype)
    if planted == 'unshifted':
        x = np.concatenate([x[:, 1:], x[:, -1:]], axis=1)
    memory, mask = ref.encoder(tokens, w, cfg, speaker_embedding)
    memory = np.where(mask[:, :, None], memory, 0).astype(dtype)
    d = 'tacotron2/decoder'
    pm = memory @ w[f'{d}/lsa/memory_layer/kernel']
    B, T = x.shape[:2]
    Tin, enc = memory.shape[1:]
    h_att = np.zeros((B, cfg.attention_rnn_dim), dtype); c_att = np.zeros_like(h_att)
    h_dec = np.zeros((B, cfg.decoder_rnn_dim), dtype); c_dec = np.zeros_like(h_dec)
    ctx = np.zeros((B, enc), dtype)
    prev_w = np.zeros((B, Tin), dtype); cum_w = np.zeros((B, Tin), dtype)
    cell_out = np.zeros((B, T, cfg.decoder_rnn_dim + enc), dtype)
    attn = np.zeros((B, T, Tin), dtype)
    for t in range(T):
        drop = None if prenet_masks is None else prenet_masks[:, max(t - 1, 0) if planted == 'mask_prev' else t]
        p_out = ref.prenet(x[:, t], w, drop)
        h_att, c_att = ref.lstm_cell(np.concatenate([p_out, ctx], -1), h_att, c_att, w[f'{d}/attention_rnn/kernel'],
                                     w[f'{d}/attention_rnn/recurrent_kernel'], w[f'{d}/attention_rnn/bias'])
        ctx, prev_w, cum_w = ref.attention(h_att, memory, pm, prev_w, cum_w, mask, w)
        h_dec, c_dec = ref.lstm_cell(np.concatenate([h_att, ctx], -1), h_dec, c_dec, w[f'{d}/decoder_rnn/cell_0/kernel'],
                                     w[f'{d}/decoder_rnn/cell_0/recurrent_kernel'], w[f'{d}/decoder_rnn/cell_0/bias'])
        cell_out[:, t] = np.concatenate([h_dec, ctx], -1)
        attn[:, t] = prev_w
    frames = cell_out @ w[f'{d}/linear_projection/kernel'] + w[f'{d}/linear_projection/bias']
    stop = ref._sigmoid(cell_out @ w[f'{d}/gate_output/kernel'] + w[f'{d}/gate_output/bias'])[..., 0]
    ar = np.arange(T)[None]
    dec_mask = ar < lengths[:, None] if planted == 'mask_lt' else ar <= lengths[:, None]
    dec_out = np.where(dec_mask[:, :, None], frames, 0).astype(dtype)
    mel = dec_out + ref.postnet(dec_out, dec_mask, w, cfg)
    return ForwardOutput(decoder_output=dec_out, mel=mel, stop_tokens=stop, attention_weights=attn)


OUTPUTS = ('decoder_output', 'mel', 'stop_tokens', 'attention_weights')


def deviations(a, b):
    """Largest absolute difference per output, as a dict."""
    return {n: float(np.abs(np.asarray(getattr(a, n), np.float64) - np.asarray(getattr(b, n), np.float64)).max()) for n in OUTPUTS}


def bounds(r32, r64):
    """The GPU tests' bound per output: tol = max(16 * d32, 64 * 2^-24 * scale), d32 the float32 restatement's largest
    deviation from the float64 one for this very case, scale the float64 output's largest magnitude.  16: the device sums the
    same ~1.5 k-term products in another association, errors of d32's class (the free-running path sits about 2x above its
    float32 floor), and every mistake planted in tests/test_teacher_forced.py stays above 10 x tol.  The floor: libm and the
    device's exp / tanh differ by an ulp."""
    d32 = deviations(r32, r64)
    return {n: max(16.0 * d32[n], 64.0 * 2.0 ** -24 * float(np.abs(getattr(r64, n)).max())) for n in OUTPUTS}


def make_case(lens, T, mel_lengths, seed=0, spk_dim=0, pad=-11.5):
    """Tokens [B, max(lens)] with `lens` real tokens per row, a mel input [B, T, 80] that is a shifted random target (zero
    go-frame) up to each row's length and `pad` past it, and a speaker matrix when spk_dim > 0."""
    rng = np.random.default_rng(seed)
    B, Tin = len(lens), max(lens)
    tok = rng.integers(1, 148, (B, Tin)).astype(np.int32)
    for b, n in enumerate(lens):
        tok[b, n:] = 0
    target = rng.uniform(-8.0, 1.0, (B, T, 80)).astype(np.float32)
    x = shift(target)
    for b, n in enumerate(mel_lengths):
        x[b, n:] = pad
    spk = rng.standard_normal((B, spk_dim)).astype(np.float32) * 0.1 if spk_dim else None
    return tok, x, np.asarray(mel_lengths, np.int32), spk
