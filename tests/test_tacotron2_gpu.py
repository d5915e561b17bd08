"""GPU parity: HIP Tacotron2 (through the C ABI) vs the numpy oracle on the same seeded inputs.

Tolerance (BASELINE.json north_star): mel spectrogram within 1e-3 abs (fp32); integer outputs (lengths) exact.
"""
import numpy as np
import pytest

from decoder_cases import pick_variant

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3


def _tokens(B, Tin, lens, seed=0):
    rng = np.random.default_rng(seed)
    tok = rng.integers(1, 148, (B, Tin)).astype(np.int32)
    for b, n in enumerate(lens):
        tok[b, n:] = 0
    return tok


def _check(out, ref, steps=None):
    assert np.array_equal(out.lengths, ref.lengths), (out.lengths, ref.lengths)
    for name in ('decoder_output', 'mel', 'stop_tokens', 'attention_weights'):
        a, r = getattr(out, name), getattr(ref, name)
        assert a.shape == r.shape, name
        err = np.abs(a - r).max()
        print(f'{name}: max abs err {err:.3e}')
        assert err <= MEL_TOL, name


MODE = 'persistent'


def _assert_machine(eng, tok, enc=512, precision='f32'):
    """The requested machine ran wherever its shape rule accepts the call (tests/decoder_cases.py), the graph otherwise."""
    v = pick_variant(MODE, tok.shape[0], tok.shape[1], enc, precision)
    want = v.machine if v is not None else 'graph'
    msg = eng._lib.tts_hip_last_error(eng._h)
    assert eng.last_decoder_mode == want, (MODE, want, eng.last_decoder_mode, msg)


@pytest.fixture(autouse=True, params=['persistent', 'fused', 'graph'])
def decoder_mode(request, gpu_engine):
    """Every test of this file runs three times: through the persistent weight-stationary decoder kernel (taken when the
    call shape allows it: batch <= 4 and B * Tin small enough for LDS), through the fused two-kernel step (batch <= 8,
    at most 256 tokens) -- larger shapes fall back by themselves -- and through the per-step hipGraph of 7 kernels."""
    global MODE
    MODE = request.param
    gpu_engine.set_decoder_mode(MODE)
    yield MODE
    gpu_engine.set_decoder_mode('auto')


def _engine(weights):
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.load_state(weights)
    eng.finalize()
    eng.set_decoder_mode(MODE)
    return eng


def test_the_requested_decoder_path_is_the_one_that_runs(gpu_engine, taco_weights, taco_cfg):
    """Guards the parametrisation above: small shapes really take the requested machine, and the paths agree far inside
    the mel tolerance (they differ by fp32 re-association only)."""
    tok = _tokens(2, 40, [40, 29], seed=11)
    masks = (np.random.default_rng(5).random((2, 30, 2, 256)) >= 0.5).astype(np.float32) * 2.0
    out = gpu_engine.tacotron2_infer(tok, max_len=30, early_stopping=False, prenet_masks=masks)
    assert gpu_engine.last_decoder_mode == MODE
    for other_mode in ('persistent', 'fused', 'graph'):
        if other_mode == MODE:
            continue
        gpu_engine.set_decoder_mode(other_mode)
        other = gpu_engine.tacotron2_infer(tok, max_len=30, early_stopping=False, prenet_masks=masks)
        assert gpu_engine.last_decoder_mode == other_mode
        d = float(np.abs(out.mel - other.mel).max())
        print(f'{MODE} vs {other_mode} decoder: mel max abs diff {d:.2e}')
        assert d <= 1e-4 and np.array_equal(out.lengths, other.lengths)
    big = _tokens(11, 16, [16] * 11, seed=3)                          # batch 11 > 8: always the per-step graph
    for m in ('persistent', 'fused', 'auto'):
        gpu_engine.set_decoder_mode(m)
        gpu_engine.tacotron2_infer(big, max_len=4, early_stopping=False)
        assert gpu_engine.last_decoder_mode == 'graph'
    gpu_engine.set_decoder_mode('auto')                               # the default: 1 - 2 rows persistent, 3 - 8 rows fused
    gpu_engine.tacotron2_infer(tok, max_len=4, early_stopping=False)
    assert gpu_engine.last_decoder_mode == 'persistent'
    gpu_engine.tacotron2_infer(_tokens(6, 24, [24, 20, 24, 7, 24, 11], seed=4), max_len=4, early_stopping=False)
    assert gpu_engine.last_decoder_mode == 'fused'


def test_fixed_steps_deterministic_b1(gpu_engine, taco_weights, taco_cfg):
    from oracle import tacotron2_ref
    tok = _tokens(1, 24, [24])
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=40, early_stopping=False)
    out = gpu_engine.tacotron2_infer(tok, max_len=40, early_stopping=False)
    _assert_machine(gpu_engine, tok)
    assert gpu_engine.last_steps == 40
    _check(out, ref)


def test_ragged_batch_with_dropout_masks(gpu_engine, taco_weights, taco_cfg):
    from oracle import tacotron2_ref
    B, Tin, T = 3, 37, 45
    tok = _tokens(B, Tin, [37, 20, 9], seed=1)
    masks = (np.random.default_rng(3).random((B, T, 2, 256)) >= 0.5).astype(np.float32) * 2.0
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=T, early_stopping=False, prenet_masks=masks)
    out = gpu_engine.tacotron2_infer(tok, max_len=T, early_stopping=False, prenet_masks=masks)
    _assert_machine(gpu_engine, tok)
    _check(out, ref)
    # masked softmax: padded token positions get exactly zero attention
    assert np.all(out.attention_weights[1, :, 20:] == 0)
    np.testing.assert_allclose(out.attention_weights.sum(-1), 1.0, atol=1e-5)


def test_early_stopping_lengths(taco_cfg):
    """Rows stop at different steps; loop ends when all have fired; `lengths` excludes the firing frame (:664-665)."""
    from oracle import tacotron2_ref
    from text_to_speech_amd import weights
    # gate kernel x10 and bias -6.55 script staggered stops: the oracle gives lengths [7, 3, 5, 37] (two graph chunks)
    w = weights.synth_tacotron2(taco_cfg, seed=1234, gate_bias=-6.55)
    w['tacotron2/decoder/gate_output/kernel'] = w['tacotron2/decoder/gate_output/kernel'] * 10
    tok = _tokens(4, 30, [30, 25, 18, 12], seed=2)
    ref = tacotron2_ref.infer(tok, w, taco_cfg, max_length=100, early_stopping=True)
    print('oracle lengths', ref.lengths)
    assert ref.lengths.max() < 99 and len(set(ref.lengths.tolist())) > 1, 'test weights must give staggered stops'
    eng = _engine(w)
    try:
        # The last row fires on the loop's final step.  Every block of that step's projection launch must still store its
        # frame (the `done` decision of a launch is latched per step, DecState::n_fin parity slots): frame lengths[b] is
        # inside the postnet mask (t <= lengths) and feeds the last mel frames.
        out = eng.tacotron2_infer(tok, max_len=100, early_stopping=True)
        _assert_machine(eng, tok)
        assert eng.last_steps == int(ref.lengths.max()) + 1
        _check(out, ref)
        for b2, n in enumerate(ref.lengths):
            assert np.abs(out.decoder_output[b2, n] - ref.decoder_output[b2, n]).max() <= MEL_TOL
            assert np.abs(out.decoder_output[b2, n]).max() > 0
            assert np.abs(out.mel[b2, n - 2:n + 1] - ref.mel[b2, n - 2:n + 1]).max() <= MEL_TOL
        # frames after the loop ended are untouched zeros
        assert np.all(out.decoder_output[:, eng.last_steps:] == 0)
    finally:
        eng.close()


def test_speaker_embedding_enc768():
    from oracle import tacotron2_ref
    from text_to_speech_amd import weights
    from text_to_speech_amd.config import Tacotron2Config
    cfg = Tacotron2Config(speaker_embedding_dim=256)
    w = weights.synth_tacotron2(cfg, seed=99)
    tok = _tokens(2, 21, [21, 15], seed=4)
    spk = np.random.default_rng(5).standard_normal((2, 256)).astype(np.float32)
    spk /= np.linalg.norm(spk, axis=1, keepdims=True)
    ref = tacotron2_ref.infer(tok, w, cfg, speaker_embedding=spk, max_length=30, early_stopping=False)
    eng = _engine(w)
    try:
        out = eng.tacotron2_infer(tok, speaker=spk, max_len=30, early_stopping=False)
        _assert_machine(eng, tok, enc=768)
        _check(out, ref)
    finally:
        eng.close()


def test_attention_window(gpu_engine, taco_weights, taco_cfg):
    from oracle import tacotron2_ref
    tok = _tokens(2, 40, [40, 33], seed=6)
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=25, early_stopping=False,
                              attn_mask_win_len=12, attn_mask_offset=0.5)
    out = gpu_engine.tacotron2_infer(tok, max_len=25, early_stopping=False, attn_mask_win_len=12, attn_mask_offset=6)
    _assert_machine(gpu_engine, tok)
    _check(out, ref)


def test_batch_larger_than_lstm_chunk(gpu_engine, taco_weights, taco_cfg):
    """B = 11 exercises the second batch chunk (NB = 8) of the LSTM step kernel."""
    from oracle import tacotron2_ref
    lens = [16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6]
    tok = _tokens(11, 16, lens, seed=7)
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=12, early_stopping=False)
    out = gpu_engine.tacotron2_infer(tok, max_len=12, early_stopping=False)
    _assert_machine(gpu_engine, tok)
    _check(out, ref)


# ---- fp16 decoder-LSTM weights (tts_hip_tacotron2_infer_f16; BASELINE configs 3 / 5) --------------------------------
# Only the two LSTM weight matrices are rounded to fp16 (relative error 2^-12 per weight); inputs, recurrent state and all
# accumulation stay fp32.  The mel tolerance of 1e-3 is an fp32 statement; the bound below is the measured error (printed)
# with margin.  Integer outputs must still agree.
MEL_TOL_F16 = 1e-3          # measured at most 4.16e-4 (B = 8; 48 steps, synthetic weights, all three machines)


@pytest.mark.parametrize('B', [1, 3, 8])
def test_fp16_lstm_weights_close_to_fp32_oracle(gpu_engine, taco_weights, taco_cfg, B):
    from oracle import tacotron2_ref
    lens = [31, 24, 17, 31, 9, 28, 30, 12][:B]
    tok = _tokens(B, 31, lens, seed=4)
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=48, early_stopping=False)
    out = gpu_engine.tacotron2_infer(tok, max_len=48, early_stopping=False, precision='f16')
    _assert_machine(gpu_engine, tok, precision='f16')
    exact = gpu_engine.tacotron2_infer(tok, max_len=48, early_stopping=False)
    _assert_machine(gpu_engine, tok)
    assert np.array_equal(out.lengths, ref.lengths)
    err = np.abs(out.mel - ref.mel).max()
    err_att = np.abs(out.attention_weights - ref.attention_weights).max()
    print(f'f16 LSTM weights B={B}: mel max abs err {err:.3e}, attention {err_att:.3e} '
          f'(fp32 path: {np.abs(exact.mel - ref.mel).max():.3e})')
    assert err <= MEL_TOL_F16 and err_att <= MEL_TOL_F16
    assert np.abs(exact.mel - ref.mel).max() <= MEL_TOL < 1e3 * max(err, 1e-12)   # and the flag is not ignored
    assert not np.array_equal(out.mel, exact.mel)


@pytest.mark.parametrize('Tin,lens,win', [(70, [70, 41], None), (130, [130, 97], 24), (300, [300, 257], None),
                                           (515, [515, 64], 40)])
def test_long_inputs_cover_every_attention_path(gpu_engine, taco_weights, taco_cfg, Tin, lens, win):
    """Token counts above 64 / 256 / 512 exercise the strided lane loops of the attention kernels, the prefetch limit of
    softmax_ctx (32 x 8 rows) with its tail loop, and the second 256-stride of the weight writer; BiLSTM runs Tin steps."""
    from oracle import tacotron2_ref
    tok = _tokens(2, Tin, lens, seed=Tin)
    kw = {} if win is None else dict(attn_mask_win_len=win, attn_mask_offset=0.5)
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=6, early_stopping=False, **kw)
    gkw = {} if win is None else dict(attn_mask_win_len=win, attn_mask_offset=win // 2)
    out = gpu_engine.tacotron2_infer(tok, max_len=6, early_stopping=False, **gkw)
    _assert_machine(gpu_engine, tok)
    _check(out, ref)
    assert np.all(out.attention_weights[1, :, lens[1]:] == 0)


@pytest.mark.parametrize('B,Tin', [(5, 45), (7, 150), (6, 128)])
def test_partially_filled_row_tiles(gpu_engine, taco_weights, taco_cfg, B, Tin):
    """Batch 5 - 7 runs the 8-row kernels of the fused step with empty rows: fewer (row, position) pairs than role waves and
    fewer context units than slots, so some waves of a block publish nothing (the hop stamps are then left by the block's last
    real publisher, csrc/taco_fused.hip `stamp_last`); 150 tokens add the two-positions-per-wave template."""
    from oracle import tacotron2_ref
    lens = [Tin, Tin - 7, max(3, Tin // 3), Tin - 1, max(2, Tin // 2), Tin - 20, 5][:B]
    tok = _tokens(B, Tin, lens, seed=B * 1000 + Tin)
    masks = (np.random.default_rng(B).random((B, 14, 2, 256)) >= 0.5).astype(np.float32) * 2.0
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=14, early_stopping=False, prenet_masks=masks)
    out = gpu_engine.tacotron2_infer(tok, max_len=14, early_stopping=False, prenet_masks=masks)
    _assert_machine(gpu_engine, tok)
    _check(out, ref)
    for b in range(B):
        assert np.all(out.attention_weights[b, :, lens[b]:] == 0)


def test_padding_and_batch_composition_do_not_change_a_row(gpu_engine):
    """Properties the reference's masking guarantees, independent of any oracle (location_sensitive_attention.py:96-102,
    tacotron2_arch.py:625-627): a sentence gives the same frames whether its token row is padded to 40 or to 120 positions,
    and whether it is decoded alone or next to other sentences -- the padded positions get exactly zero attention."""
    rng = np.random.default_rng(9)
    real = rng.integers(1, 148, 37).astype(np.int32)
    T = 24
    masks = (rng.random((3, T, 2, 256)) >= 0.5).astype(np.float32) * 2.0
    outs = []
    for Tin in (40, 120):
        tok = np.zeros((1, Tin), np.int32)
        tok[0, :37] = real
        outs.append(gpu_engine.tacotron2_infer(tok, max_len=T, early_stopping=False, prenet_masks=masks[:1]))
        _assert_machine(gpu_engine, tok)
    a, b = outs
    assert np.abs(a.mel - b.mel).max() <= 2e-5
    assert (b.attention_weights[0, :, 37:] == 0).all() and (a.attention_weights[0, :, 37:] == 0).all()
    np.testing.assert_allclose(a.attention_weights[0, :, :37], b.attention_weights[0, :, :37], atol=2e-6)
    np.testing.assert_allclose(b.attention_weights[0].sum(-1), 1.0, atol=1e-5)
    # the same sentence as row 1 of a batch of three
    tok3 = np.zeros((3, 64), np.int32)
    tok3[0, :64] = rng.integers(1, 148, 64)
    tok3[1, :37] = real
    tok3[2, :9] = rng.integers(1, 148, 9)
    m3 = masks.copy()
    m3[1] = masks[0]
    c = gpu_engine.tacotron2_infer(tok3, max_len=T, early_stopping=False, prenet_masks=m3)
    _assert_machine(gpu_engine, tok3)
    assert np.abs(c.mel[1] - a.mel[0]).max() <= 2e-5
    assert (c.attention_weights[1, :, 37:] == 0).all() and (c.attention_weights[2, :, 9:] == 0).all()
