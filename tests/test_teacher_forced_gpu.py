"""GPU: HipEngine.tacotron2_forward (tts_hip_tacotron2_forward, the teacher-forced pass) against the float64 numpy restatement
of Tacotron2.call (tests/teacher_forced_ref.py), on all four outputs and over the whole [B, T].

Bound per output and case: tol = max(16 * d32, 64 * 2^-24 * scale) (teacher_forced_ref.bounds: d32 = the float32 restatement's
deviation from the float64 one for that very case, scale = the float64 output's largest magnitude);
tests/test_teacher_forced.py shows it is below a tenth of every planted mistake.  Inputs: synthetic weights, a shifted random
target, the padding value -11.5 past each row's length.

Errors measured on an MI355X, max abs against float64 as decoder_output / mel / stop_tokens / attention (tol in brackets;
DESIGN.md section 4.3d has the same table):
  go_frame_only       1.6e-7 (1.1e-6) / 1.7e-7 (2.8e-6) / 6.5e-9 (2.2e-7) / 3.9e-8 (7.9e-7)
  one_chunk           1.7e-6 (7.8e-6) / 2.1e-6 (2.0e-5) / 8.1e-8 (4.7e-7) / 4.0e-8 (5.0e-7)
  chunk_plus_one      1.5e-6 (8.9e-6) / 1.7e-6 (2.0e-5) / 8.1e-8 (5.7e-7) / 1.4e-7 (1.1e-6)
  five_rows           1.0e-6 (6.2e-6) / 1.4e-6 (1.6e-5) / 7.8e-8 (4.6e-7) / 3.1e-8 (5.9e-7)
  full_tile           1.8e-6 (9.3e-6) / 2.2e-6 (1.9e-5) / 1.5e-7 (7.9e-7) / 5.8e-8 (1.1e-6)
  second_batch_chunk  1.2e-6 (1.4e-5) / 1.2e-6 (1.8e-5) / 7.3e-8 (4.0e-7) / 4.7e-8 (8.6e-7)
  speaker             1.5e-6 (8.2e-6) / 1.6e-6 (1.6e-5) / 3.2e-8 (1.9e-7) / 2.3e-8 (5.1e-7)
  explicit masks      1.6e-6 (8.3e-6) / 1.6e-6 (1.6e-5) / 1.3e-7 (3.9e-7) / 5.6e-8 (1.1e-6)
  self-fed            1.1e-6 (6.3e-6) / 1.5e-6 (1.9e-5) / 7.8e-8 (4.3e-7) / 5.5e-8 (1.1e-6)
  f16 weights         1.9e-4 / 3.2e-4 / 1.2e-5 / 4.7e-6 (MEL_TOL_F16 = 1e-3)
  kept batch, T = 33  1.4e-6 (8.9e-6) / 1.8e-6 (1.9e-5) / 7.1e-8 (6.6e-7) / 9.1e-8 (1.1e-6); T = 31, replayed: the same
(With the projection's bias at the head of the GEMM's k-ordered chain the stop tokens of one_chunk were 6.0e-7 off, above
their bound: the gate bias, -3.0, set the ulp every product was rounded at.  The bias is added behind the sum now.)
"""
import numpy as np
import pytest

import teacher_forced_ref as tf
from oracle import tacotron2_ref

pytestmark = pytest.mark.gpu

MEL_TOL_F16 = 1e-3          # the bound of tests/test_tacotron2_gpu.py for fp16 LSTM weights (4.2e-4 measured free-running)

#        tokens per row (Tin = max)            T   mel_lengths                      speaker width
CASES = {
    'go_frame_only': ((5,), 1, (1,), 0),                                            # one row tile of the LSTM
    'one_chunk': ((21, 14), 32, (32, 31), 0),                                       # B*T = 64: one GEMM row tile; row 1's <= frame
    'chunk_plus_one': ((21, 14, 5), 33, (33, 17, 1), 0),                            # a 4-row tile with an empty slot
    'five_rows': ((37, 30, 23, 16, 9), 13, (13, 9, 6, 2, 1), 0),                    # B*T = 65; an 8-row tile with three empty slots
    'full_tile': ((70, 61, 52, 44, 35, 27, 19, 11), 65, (65, 64, 50, 33, 32, 31, 2, 1), 0),     # two chunks + 1
    'second_batch_chunk': ((21, 19, 17, 15, 13, 12, 10, 8, 6), 8, (8, 7, 6, 5, 4, 3, 2, 1, 8), 0),
    'speaker': ((21, 14), 33, (33, 20), 256),                                       # enc = 768
}


@pytest.fixture(scope='module')
def spk_weights():
    from text_to_speech_amd import weights
    from text_to_speech_amd.config import Tacotron2Config
    cfg = Tacotron2Config(speaker_embedding_dim=256)
    return cfg, weights.synth_tacotron2(cfg, seed=1234)


@pytest.fixture(scope='module')
def spk_engine(spk_weights):
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.load_state(spk_weights[1])
    eng.finalize()
    yield eng
    eng.close()


def _check(out, r32, r64, what):
    tol = tf.bounds(r32, r64)
    err = tf.deviations(out, r64)
    d32 = tf.deviations(r32, r64)
    for n in tf.OUTPUTS:
        print(f'{what}: {n}: gpu err {err[n]:.3e}  d32 {d32[n]:.3e}  tol {tol[n]:.3e}')
    for n in tf.OUTPUTS:
        assert getattr(out, n).shape == getattr(r64, n).shape, n
        assert err[n] <= tol[n], (what, n, err[n], tol[n])


@pytest.fixture(scope='module')
def three_rows(taco_weights, taco_cfg):
    """The 3-row case and its restatements, with and without dropout masks: computed once, shared, never modified."""
    lens, T, ml, _ = CASES['chunk_plus_one']
    tok, x, mel_lengths, _ = tf.make_case(lens, T, ml, seed=33)
    masks = (np.random.default_rng(8).random((len(lens), T, 2, 256)) >= 0.5).astype(np.float32) * 2.0
    refs = {m is not None: tuple(tf.forward(tok, x, mel_lengths, taco_weights, taco_cfg, prenet_masks=m, dtype=dt)
                                 for dt in (np.float32, np.float64)) for m in (None, masks)}
    return tok, x, mel_lengths, masks, refs


@pytest.mark.parametrize('name', list(CASES))
def test_forward_matches_the_float64_restatement(name, gpu_engine, taco_weights, taco_cfg, request):
    lens, T, ml, spk_dim = CASES[name]
    tok, x, mel_lengths, spk = tf.make_case(lens, T, ml, seed=len(lens) * 100 + T, spk_dim=spk_dim)
    if spk_dim:
        eng = request.getfixturevalue('spk_engine')
        cfg, w = request.getfixturevalue('spk_weights')
    else:
        eng, cfg, w = gpu_engine, taco_cfg, taco_weights
    r32, r64 = (tf.forward(tok, x, mel_lengths, w, cfg, speaker_embedding=spk, dtype=dt) for dt in (np.float32, np.float64))
    out = eng.tacotron2_forward(tok, x, mel_lengths, speaker=spk)
    _check(out, r32, r64, name)
    for b, n in enumerate(ml):                                  # the <= mask: frame t == length is kept, later ones are zero
        assert np.all(out.decoder_output[b, n + 1:] == 0)
        if n < T:
            assert np.any(out.decoder_output[b, n] != 0)


def test_explicit_masks(gpu_engine, three_rows):
    tok, x, mel_lengths, masks, refs = three_rows
    out = gpu_engine.tacotron2_forward(tok, x, mel_lengths, prenet_masks=masks)
    _check(out, *refs[True], 'masks')
    plain = gpu_engine.tacotron2_forward(tok, x, mel_lengths)
    assert np.abs(out.mel - plain.mel).max() > 1e-2            # the masks were applied


def test_seed_is_the_explicit_call_with_the_drawn_masks(gpu_engine, three_rows):
    tok, x, mel_lengths, _, _ = three_rows
    B, T = x.shape[:2]
    drawn = gpu_engine.random_prenet_masks(B, T, 77).cpu().numpy()
    a = gpu_engine.tacotron2_forward(tok, x, mel_lengths, seed=77)
    b = gpu_engine.tacotron2_forward(tok, x, mel_lengths, prenet_masks=drawn)
    for n in tf.OUTPUTS:
        assert np.array_equal(getattr(a, n), getattr(b, n)), n
    c = gpu_engine.tacotron2_forward(tok, x, mel_lengths, seed=77, offset=5)
    assert not np.array_equal(a.mel, c.mel)


def test_cuda_tensor_inputs_equal_the_host_call(gpu_engine, three_rows):
    import torch
    tok, x, mel_lengths, masks, _ = three_rows
    host = gpu_engine.tacotron2_forward(tok, x, mel_lengths, prenet_masks=masks)
    dev = gpu_engine.tacotron2_forward(torch.as_tensor(tok).cuda(), torch.as_tensor(x).cuda(), mel_lengths,
                                       prenet_masks=torch.as_tensor(masks).cuda())
    for n in tf.OUTPUTS:
        t = getattr(dev, n)
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), getattr(host, n)), n


def test_f16_weights_within_their_bound_and_really_used(gpu_engine, three_rows):
    tok, x, mel_lengths, _, refs = three_rows
    f32 = gpu_engine.tacotron2_forward(tok, x, mel_lengths)
    f16 = gpu_engine.tacotron2_forward(tok, x, mel_lengths, precision='f16')
    err = tf.deviations(f16, refs[False][1])
    print('f16:', err)
    for n in tf.OUTPUTS:
        assert err[n] <= MEL_TOL_F16, (n, err[n])
    assert not np.array_equal(f16.mel, f32.mel)


def test_a_row_alone_equals_its_row_of_the_batch(gpu_engine, three_rows):
    tok, x, mel_lengths, _, refs = three_rows
    batch = gpu_engine.tacotron2_forward(tok, x, mel_lengths)
    tol = tf.bounds(*refs[False])
    for b in range(tok.shape[0]):
        n_tok = int((tok[b] != 0).sum())
        one = gpu_engine.tacotron2_forward(tok[b:b + 1, :n_tok], x[b:b + 1], mel_lengths[b:b + 1])
        for n in tf.OUTPUTS:
            full = getattr(batch, n)[b]
            if n == 'attention_weights':
                assert np.all(full[:, n_tok:] == 0)
                full = full[:, :n_tok]
            d = float(np.abs(getattr(one, n)[0] - full).max())
            assert d <= tol[n], (b, n, d, tol[n])


def _same(a, b, what):
    for n in tf.OUTPUTS:
        assert np.array_equal(getattr(a, n), getattr(b, n)), (what, n)


def test_shorter_call_in_between_leaves_nothing_behind(gpu_engine, three_rows, taco_weights, taco_cfg):
    """T = 33, 31, 33 on ONE EncodedBatch of one handle.  The batch matters: a call made from tokens encodes into a fresh
    buffer, which empties the handle's graph cache, so it always captures its own chunk graph.  With the batch kept, the three
    calls share a key (one max_len bucket) and the second and third REPLAY the graph the first captured, with T read from the
    device-side state: a stale history, a stale graph or a buffer that moved with T would show."""
    tok, x, mel_lengths, _, refs = three_rows
    short_len = np.minimum(mel_lengths, 31).astype(np.int32)
    enc = gpu_engine.tacotron2_encode(tok)
    try:
        first = gpu_engine.tacotron2_forward(enc, x, mel_lengths)
        short = gpu_engine.tacotron2_forward(enc, x[:, :31], short_len)
        third = gpu_engine.tacotron2_forward(enc, x, mel_lengths)
    finally:
        enc.close()
    _same(first, third, 'first / third')
    _check(first, *refs[False], 'kept batch, T = 33')
    s32, s64 = (tf.forward(tok, x[:, :31], short_len, taco_weights, taco_cfg, dtype=dt) for dt in (np.float32, np.float64))
    _check(short, s32, s64, 'kept batch, T = 31 (replayed)')
    # stop tokens and alignments are not masked and no step looks ahead: they do not depend on T at all
    assert np.array_equal(short.attention_weights, first.attention_weights[:, :31])
    assert np.array_equal(short.stop_tokens, first.stop_tokens[:, :31])
    _same(first, gpu_engine.tacotron2_forward(tok, x, mel_lengths), 'replayed / freshly captured')


def test_every_graph_key_of_one_encoded_batch_is_replayed_right(gpu_engine, three_rows):
    """One EncodedBatch through the four keys a forward graph can have for it (masks or none, f32 or fp16 weights), with a
    decode call of the same batch, bucket and machine layout in between, twice over: the second round replays the graphs of
    the first (the masks change where every later buffer of the plan starts, the precision which matrices the nodes stream,
    and a decode graph must never answer a forward key).  Every result within its bound, the rounds bit-equal."""
    tok, x, mel_lengths, masks, refs = three_rows
    gpu_engine.set_decoder_mode('graph')
    enc = gpu_engine.tacotron2_encode(tok)
    try:
        rounds = []
        for _ in range(2):
            r = {}
            for with_masks in (False, True):
                for precision in ('f32', 'f16'):
                    r[with_masks, precision] = gpu_engine.tacotron2_forward(
                        enc, x, mel_lengths, prenet_masks=masks if with_masks else None, precision=precision)
                r['decode', with_masks] = gpu_engine.tacotron2_decode(
                    enc, max_len=33, early_stopping=False, prenet_masks=masks if with_masks else None)
            rounds.append(r)
    finally:
        enc.close()
        gpu_engine.set_decoder_mode('auto')
    for with_masks in (False, True):
        _check(rounds[0][with_masks, 'f32'], *refs[with_masks], f'kept batch, masks {with_masks}')
        err = tf.deviations(rounds[0][with_masks, 'f16'], refs[with_masks][1])
        for n in tf.OUTPUTS:
            assert err[n] <= MEL_TOL_F16, (with_masks, n, err[n])
        assert not np.array_equal(rounds[0][with_masks, 'f16'].mel, rounds[0][with_masks, 'f32'].mel)
    assert not np.array_equal(rounds[0][True, 'f32'].mel, rounds[0][False, 'f32'].mel)
    for key in rounds[0]:
        _same(rounds[0][key], rounds[1][key], key)
        if key[0] == 'decode':
            assert np.array_equal(rounds[0][key].lengths, rounds[1][key].lengths)


def test_infer_is_unaffected_by_a_forward_call(gpu_engine, three_rows):
    tok, x, mel_lengths, masks, _ = three_rows
    gpu_engine.set_decoder_mode('graph')
    try:
        before = gpu_engine.tacotron2_infer(tok, max_len=40, early_stopping=False)
        gpu_engine.tacotron2_forward(tok, x, mel_lengths, prenet_masks=masks)
        after = gpu_engine.tacotron2_infer(tok, max_len=40, early_stopping=False)
        assert gpu_engine.last_decoder_mode == 'graph'
    finally:
        gpu_engine.set_decoder_mode('auto')
    for n in tf.OUTPUTS + ('lengths',):
        assert np.array_equal(getattr(before, n), getattr(after, n)), n


def test_self_fed_forward_is_the_free_running_oracle(gpu_engine, three_rows, taco_weights, taco_cfg):
    """The engine's forward pass on the oracle's own shifted free-running output, against tacotron2_ref.infer in float64."""
    tok = three_rows[0]
    T = 33
    free32, free64 = (tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=T, early_stopping=False, dtype=dt)
                      for dt in (np.float32, np.float64))
    assert np.array_equal(free32.lengths, free64.lengths)
    x = tf.shift(free64.decoder_output).astype(np.float32)
    lengths = np.clip(free64.lengths, 1, T).astype(np.int32)
    want = np.arange(T)[None] <= free64.lengths[:, None]
    assert np.array_equal(np.arange(T)[None] <= lengths[:, None], want)        # the clip changed no mask
    # the bound's d32 for THIS case: the float32 restatement on the same input against the float64 free-running oracle
    r32 = tf.forward(tok, x, lengths, taco_weights, taco_cfg)
    out = gpu_engine.tacotron2_forward(tok, x, lengths)
    _check(out, r32, free64, 'self-fed')
