"""A float64 numpy restatement of the reference's TacotronLoss (custom_train_objects/losses/tacotron_loss.py: `call`,
`compute_mel_loss`, `output_names`), written from that file and from Keras' `binary_crossentropy`, not from the kernel: the
checker of tests/test_taco_loss.py and tests/test_taco_loss_gpu.py.  It also holds the cases both files share and the planted
mistakes the GPU bound has to stay a factor ten below.

The inputs are what the GPU gets (float32 values); everything here is float64 but the two clip constants, which Keras takes
as float32 (`epsilon()` = 1e-7 cast to the tensor's dtype).
"""
import numpy as np

KINDS = ('mse', 'mae', 'weighted_mse', 'weighted_mae')
CHUNK = 16                      # kLossChunkFrames of csrc/taco_loss_call.h: frames of a row one block sums
FINISH_TILE = 200               # chunks whose partial sums the finishing launch loads at once (FT of csrc/taco_loss.hip)
PAD = -11.0                     # what the cases pad their mels with
RTOL, ATOL = 2e-6, 1e-12        # |got - ref| <= RTOL |ref| + ATOL on every output (the derivation: DESIGN.md section 4.3e)

CLIP_LO, CLIP_HI = np.float32(1e-7), np.float32(1 - 1e-7)


def output_names(mel_loss):
    kinds = list(mel_loss) if isinstance(mel_loss, (list, tuple)) else [mel_loss]
    return ['loss'] + [f'{k}_mel_loss' for k in kinds] + [f'{k}_mel_postnet_loss' for k in kinds] + ['gate_loss']


def _divide_no_nan(a, b):
    return np.where(b == 0, 0.0, a / np.where(b == 0, 1.0, b))


def mel_loss(y, p, kind, mask, *, frame_mean=False, extrema_lengths=None):
    """compute_mel_loss for one kind -> [B].  y, p [B, T, C] float64; mask [B, T] or None.  The two keywords plant mistakes:
    `frame_mean` averages over frames instead of over the spectrogram, `extrema_lengths` takes the row extrema of the weighted
    kinds over each row's real frames only."""
    if 'mse' in kind:
        e = np.square(y - p)
    elif 'mae' in kind:
        e = np.abs(y - p)
    else:
        raise ValueError(f'Unknown loss : {kind}')
    if 'weighted' in kind:
        if extrema_lengths is None:
            lo, hi = y.min(axis=(1, 2), keepdims=True), y.max(axis=(1, 2), keepdims=True)
        else:
            lo = np.stack([y[b, :n].min() for b, n in enumerate(extrema_lengths)]).reshape(-1, 1, 1)
            hi = np.stack([y[b, :n].max() for b, n in enumerate(extrema_lengths)]).reshape(-1, 1, 1)
        w = y - lo + 1.0
        e = e * (w / (hi - lo + 1.0))
    e = e.sum(axis=2)
    channels = 1.0 if frame_mean else float(y.shape[2])
    if mask is None:
        return _divide_no_nan(e.sum(axis=1), np.full(y.shape[0], y.shape[1] * channels))
    return _divide_no_nan((e * mask).sum(axis=1), mask.sum(axis=1) * channels)


def gate_bce(g, x, from_logits, clip=True):
    """Keras' binary_crossentropy per element (no label smoothing: the reference's `call` never applies it)."""
    if from_logits:
        return np.maximum(x, 0.0) - x * g + np.log1p(np.exp(-np.abs(x)))
    o = np.clip(x, np.float64(CLIP_LO), np.float64(CLIP_HI)) if clip else x
    with np.errstate(divide='ignore', invalid='ignore'):
        return -(g * np.log(o) + (1.0 - g) * np.log(1.0 - o))


def tacotron_loss(mel_target, gate_target, decoder_output, mel, stop_tokens, *, mel_loss_kinds='mse', mask_mel_padding=True,
                  from_logits=False, finish_weight=1., not_finish_weight=1., mistake=None, lengths=None):
    """TacotronLoss.call -> float64 [K, B], rows as `output_names(mel_loss_kinds)`.  `mistake` plants one of MISTAKES
    (`lengths`: the rows' real frame counts, which three of them need)."""
    assert mistake is None or mistake in MISTAKES
    y, g, d, p, x = (np.asarray(a, dtype=np.float64) for a in (mel_target, gate_target, decoder_output, mel, stop_tokens))
    kinds = list(mel_loss_kinds) if isinstance(mel_loss_kinds, (list, tuple)) else [mel_loss_kinds]
    fw, nfw = (not_finish_weight, finish_weight) if mistake == 'swapped finish weights' else (finish_weight, not_finish_weight)
    bce = gate_bce(g, x, from_logits, clip=mistake != 'missing clip') * (g * fw + (1.0 - g) * nfw)
    if mistake == 'gate mean over the row length':
        gate = np.stack([bce[b, :n].sum() / n for b, n in enumerate(lengths)])
    else:
        gate = bce.mean(axis=1)
    mask = 1.0 - g if mask_mel_padding else None
    if mistake == 'mask keeps the last real frame' and mask is not None:
        mask = mask.copy()
        for b, n in enumerate(lengths):
            mask[b, n - 1] = 1.0
    extra = dict(frame_mean=mistake == 'mean over frames',
                 extrema_lengths=lengths if mistake == 'row extrema over real frames' else None)
    dec = [mel_loss(y, d, k, mask, **extra) for k in kinds]
    post = [mel_loss(y, p, k, mask, **extra) for k in kinds]
    return np.stack([gate + sum(dec) + sum(post)] + dec + post + [gate])


MISTAKES = ('gate mean over the row length', 'mask keeps the last real frame', 'mean over frames',
            'row extrema over real frames', 'missing clip', 'swapped finish weights')


def within(got, ref):
    """-> (every output within the bound, the largest |got - ref| / (RTOL |ref| + ATOL))"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ratio = np.abs(got - ref) / (RTOL * np.abs(ref) + ATOL)
    return bool(np.all(np.isfinite(got)) and got.shape == ref.shape and np.all(ratio <= 1.0)), float(ratio.max())


# ---- the cases of the GPU test -----------------------------------------------------------------------------------------------
def make_inputs(lengths, T, seed, *, soft_gate=None, stop=None, pad=PAD):
    """Seeded finite inputs for rows of `lengths` real frames in T: a log-mel-like target in [-10.5, 1.5] with `pad` behind a
    row's frames -- above the pad value, so that the padded frames hold the row's minimum -- predictions a few tenths off
    it, the prepare_data gate (zeros, 1 on the last real frame and on the padding; `soft_gate`: that value instead of 0) and stop
    probabilities in (0.02, 0.98) (`stop`: 'edges' = exactly 0 and 1 alternating, 'logits' = +-100 alternating).
    -> dict(mel_target, gate_target, decoder_output, mel, stop_tokens, lengths), float32."""
    rng = np.random.default_rng(seed)
    B = len(lengths)
    y = rng.uniform(-10.5, 1.5, (B, T, 80))
    d = y + rng.normal(0, 0.4, y.shape)
    p = y + rng.normal(0, 0.25, y.shape)
    g = np.ones((B, T))
    x = rng.uniform(0.02, 0.98, (B, T))
    for b, n in enumerate(lengths):
        assert 1 <= n <= T
        y[b, n:] = pad
        g[b, :n - 1] = 0.0 if soft_gate is None else soft_gate
    if stop == 'edges':
        x = (np.arange(B * T).reshape(B, T) % 2).astype(np.float64)
    elif stop == 'logits':
        x = np.where(np.arange(B * T).reshape(B, T) % 3 == 0, 100.0, -100.0)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(mel_target=f32(y), gate_target=f32(g), decoder_output=f32(d), mel=f32(p), stop_tokens=f32(x),
                lengths=tuple(int(n) for n in lengths))


ALL_KINDS = list(KINDS)
# name -> (lengths, T, make_inputs keywords, loss keywords); the frame-limit case (B = 8, T = 8192) is built by the GPU test alone
CASES = {
    'one_frame': ((1,), 1, {}, {}),
    'three_rows': ((33, 17, 1), 33, {}, {}),                                   # the last row's mask is all zero
    'chunk_minus_1': ((CHUNK - 1, 5), CHUNK - 1, {}, dict(mel_loss_kinds=ALL_KINDS)),
    'chunk': ((CHUNK, CHUNK - 1), CHUNK, {}, dict(mel_loss_kinds=ALL_KINDS)),
    'chunk_plus_1': ((CHUNK + 1, CHUNK), CHUNK + 1, {}, dict(mel_loss_kinds=ALL_KINDS)),
    'two_chunks_plus_1': ((2 * CHUNK + 1, CHUNK + 2), 2 * CHUNK + 1, {}, dict(mel_loss_kinds=ALL_KINDS)),
    'finish_tile': ((FINISH_TILE * CHUNK, 77), FINISH_TILE * CHUNK, {}, dict(mel_loss_kinds=['mse', 'weighted_mae'])),
    'finish_tile_plus_1': ((FINISH_TILE * CHUNK + 1, FINISH_TILE * CHUNK), FINISH_TILE * CHUNK + 1, {},
                           dict(mel_loss_kinds=['mse', 'weighted_mae'])),
    'mse': ((33, 17, 1), 33, {}, dict(mel_loss_kinds='mse')),
    'mae': ((33, 17, 1), 33, {}, dict(mel_loss_kinds='mae')),
    'weighted_mse': ((33, 17, 1), 33, {}, dict(mel_loss_kinds='weighted_mse')),
    'weighted_mae': ((33, 17, 1), 33, {}, dict(mel_loss_kinds='weighted_mae')),
    'all_kinds': ((33, 17, 1), 33, {}, dict(mel_loss_kinds=ALL_KINDS)),
    'other_order': ((33, 17, 1), 33, {}, dict(mel_loss_kinds=['weighted_mae', 'mse'])),
    'no_mask': ((33, 17, 1), 33, {}, dict(mel_loss_kinds=ALL_KINDS, mask_mel_padding=False)),
    'weights_5_half': ((33, 17, 1), 33, {}, dict(finish_weight=5., not_finish_weight=0.5)),
    'soft_gate': ((33, 17, 2), 33, dict(soft_gate=0.25), dict(mel_loss_kinds=ALL_KINDS, finish_weight=5., not_finish_weight=0.5)),
    'stop_edges': ((33, 17, 1), 33, dict(stop='edges'), {}),
    'logits': ((33, 17, 1), 33, dict(stop='logits'), dict(from_logits=True)),
}


def case(name):
    """-> (the inputs dict of make_inputs, the loss keywords)"""
    lengths, T, make_kw, loss_kw = CASES[name]
    return make_inputs(lengths, T, seed=1000 + sorted(CASES).index(name), **make_kw), dict(loss_kw)


def reference(inputs, loss_kw, **extra):
    return tacotron_loss(*(inputs[k] for k in ('mel_target', 'gate_target', 'decoder_output', 'mel', 'stop_tokens')),
                         **loss_kw, **extra)
