"""CPU: the teacher-forced pass (Tacotron2.call) -- its numpy restatement against the free-running oracle, the bound the GPU
tests use against planted mistakes, and the host logic of Tacotron2.teacher_forced.  (The call's front end, csrc/taco_call.h,
is tested with its siblings in tests/test_taco_call.py.)

Measured here (synth_tacotron2(seed=1234), B = 3, 21 / 14 / 5 tokens, T = 70, mel_lengths 70 / 37 / 1), as dec / stop / attention:
  self-fed restatement vs tacotron2_ref.infer      1.3e-6 / 4.5e-8 / 0.0 (mel 1.6e-6)
  d32 (float32 restatement vs float64)             6.1e-7 / 4.3e-8 / 1.2e-7 (mel 1.2e-6); with dropout masks 6.0e-7 / 3.5e-8 / 1.3e-7
  planted: input not shifted                       0.15 / 4.4e-3 / 1.0e-2 (with masks 0.41 / 1.7e-2 / 2.2e-2)
  planted: mask < for <=                           0.82 / 0 / 0
  planted: dropout mask of step t - 1              0.41 / 2.0e-2 / 1.0e-1
"""
from collections import namedtuple

import numpy as np
import pytest

import teacher_forced_ref as tf
from oracle import tacotron2_ref

LENS, T, MEL_LENGTHS = (21, 14, 5), 70, (70, 37, 1)


@pytest.fixture(scope='module')
def case():
    return tf.make_case(LENS, T, MEL_LENGTHS, seed=3)


@pytest.fixture(scope='module')
def masks():
    return (np.random.default_rng(7).random((len(LENS), T, 2, 256)) >= 0.5).astype(np.float32) * 2.0


@pytest.fixture(scope='module')
def refs(case, masks, taco_weights, taco_cfg):
    """{with masks?: (float32 restatement, float64 restatement)}: computed once, shared, never modified."""
    tok, x, lens, _ = case
    return {m is not None: tuple(tf.forward(tok, x, lens, taco_weights, taco_cfg, prenet_masks=m, dtype=dt)
                                 for dt in (np.float32, np.float64)) for m in (None, masks)}


def test_self_fed_restatement_is_the_free_running_oracle(taco_weights, taco_cfg):
    """Fed the free-running oracle's own decoder output, shifted by one, the teacher-forced restatement must reproduce it:
    the inputs of every step are then the ones infer saw.  What is left is BLAS batching (the projection over all steps)."""
    tok = tf.make_case(LENS, T, MEL_LENGTHS, seed=3)[0]
    free = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=T, early_stopping=False)
    out = tf.forward(tok, tf.shift(free.decoder_output), free.lengths, taco_weights, taco_cfg)
    # free.lengths counts the steps before a row's stop token fired; the mask t <= lengths is the one infer applied (:745)
    d = tf.deviations(out, free)
    print('self-fed vs infer:', d)
    # both sides are float32 numpy on the same inputs: a few ulp of the output's magnitude (the floor of tf.bounds)
    for n in tf.OUTPUTS:
        assert d[n] <= 64.0 * 2.0 ** -24 * float(np.abs(getattr(free, n)).max()), (n, d[n])


@pytest.mark.parametrize('with_masks', [False, True])
def test_bound_is_far_below_every_planted_error(case, masks, refs, taco_weights, taco_cfg, with_masks):
    tok, x, lens, _ = case
    m = masks if with_masks else None
    r32, r64 = refs[with_masks]
    tol = tf.bounds(r32, r64)
    print('d32:', tf.deviations(r32, r64), 'tol:', tol)
    moved = {'unshifted': ('decoder_output', 'mel', 'stop_tokens', 'attention_weights'), 'mask_lt': ('decoder_output', 'mel'),
             'mask_prev': ('decoder_output', 'mel', 'stop_tokens', 'attention_weights')}
    for planted, names in moved.items():
        if planted == 'mask_prev' and not with_masks:
            continue
        bad = tf.forward(tok, x, lens, taco_weights, taco_cfg, prenet_masks=m, dtype=np.float64, planted=planted)
        d = tf.deviations(bad, r64)
        print(planted, d)
        for n in names:
            assert tol[n] < 0.1 * d[n], (planted, n, tol[n], d[n])
        for n in set(tf.OUTPUTS) - set(names):
            assert d[n] == 0.0, (planted, n)


def test_semantics_of_the_restatement(case, refs):
    """Frames past a row's length + 1 are zero in decoder_output (the <= keeps frame t == length), stop tokens are not masked."""
    _, _, lens, _ = case
    r32 = refs[False][0]
    for b, n in enumerate(lens):
        assert np.all(r32.decoder_output[b, n + 1:] == 0)
        if n < T:
            assert np.any(r32.decoder_output[b, n] != 0)
    assert np.all((r32.stop_tokens > 0) & (r32.stop_tokens < 1))
    np.testing.assert_allclose(r32.attention_weights.sum(-1), 1.0, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------ host logic
def test_attention_durations():
    from text_to_speech_amd.tacotron2 import attention_durations
    att = np.zeros((6, 4), np.float32)
    for t, i in enumerate([0, 0, 1, 3, 3, 2]):
        att[t, i] = 0.6
        att[t, (i + 1) % 4] = 0.4
    assert attention_durations(att).tolist() == [2, 1, 1, 2]
    assert attention_durations(att, 4).tolist() == [2, 1, 0, 1]          # only frames t < length count
    assert attention_durations(att, 0).tolist() == [0, 0, 0, 0]
    tie = np.full((3, 5), 0.2, np.float32)
    assert attention_durations(tie).tolist() == [3, 0, 0, 0, 0]          # first index on ties, as the device's argmax
    for n in range(7):
        assert attention_durations(att, n).sum() == n
    with pytest.raises(ValueError):
        attention_durations(att, 7)
    with pytest.raises(ValueError):
        attention_durations(att[0])


def test_shift_mel_target_is_prepare_data():
    from text_to_speech_amd.tacotron2 import shift_mel_target
    mel = np.arange(5 * 80, dtype=np.float32).reshape(5, 80) + 1
    x = shift_mel_target(mel)
    padded = np.pad(mel, [(1, 0), (0, 0)])                                # prepare_output; prepare_data feeds padded[:-1]
    assert np.array_equal(x, padded[:-1]) and x.shape == mel.shape and len(padded) - 1 == len(x)
    assert np.array_equal(shift_mel_target(mel[:1]), np.zeros((1, 80), np.float32))
    with pytest.raises(ValueError):
        shift_mel_target(np.zeros((0, 80), np.float32))


class _FakeRuntime:
    """Stands for HipRuntime: records the call, answers with a diagonal alignment."""
    Out = namedtuple('Out', ['decoder_output', 'mel', 'stop_tokens', 'attention_weights'])

    def __init__(self):
        self.calls = []

    def tacotron2_forward(self, inputs, mel_input, mel_lengths, **kwargs):
        self.calls.append((inputs, mel_input, mel_lengths, kwargs))
        tokens = inputs[0] if isinstance(inputs, tuple) else inputs
        B, T, Tin = mel_input.shape[0], mel_input.shape[1], tokens.shape[1]
        att = np.zeros((B, T, Tin), np.float32)
        att[0, np.arange(T), np.minimum(np.arange(T) // 2, Tin - 1)] = 1.0
        return self.Out(mel_input + 1, mel_input + 2, np.full((B, T), 0.25, np.float32), att)


def test_teacher_forced_host_logic():
    from text_to_speech_amd.tacotron2 import SV2TTSTacotron2, Tacotron2, shift_mel_target
    rt = _FakeRuntime()
    model = Tacotron2(rt, lang='en')
    target = np.random.default_rng(0).uniform(-8, 1, (9, 80)).astype(np.float32)
    res = model.teacher_forced('Hello, World!', mel=target)
    (inputs, mel_input, mel_lengths, kwargs), = rt.calls
    cleaned = model.clean_text('Hello, World!')
    assert res['text'] == 'Hello, World!' and res['cleaned'] == cleaned
    assert np.array_equal(inputs, np.asarray(model.encode_text(cleaned, cleaned=True), np.int32)[None])
    assert mel_input.shape == (1, 9, 80) and np.array_equal(mel_input[0], shift_mel_target(target))
    assert np.all(mel_input[0, 0] == 0) and np.array_equal(mel_input[0, 1:], target[:-1])
    assert mel_lengths.tolist() == [9] and kwargs == {'deterministic': True}
    Tin = inputs.shape[1]
    assert res['mel'].shape == (9, 80) and np.array_equal(res['mel'], mel_input[0] + 2)
    assert np.array_equal(res['decoder_output'], mel_input[0] + 1)
    assert res['stop_tokens'].shape == (9,) and res['attention'].shape == (9, Tin)
    assert res['durations'].tolist() == [2, 2, 2, 2, 1] + [0] * (Tin - 5) and res['durations'].sum() == 9
    assert model.teacher_forced('Hello', mel=target[None], deterministic=False)['mel'].shape == (9, 80)
    assert rt.calls[-1][3] == {'deterministic': False}
    with pytest.raises(ValueError):
        model.teacher_forced('Hello')                                     # neither mel nor audio
    with pytest.raises(ValueError):
        model.teacher_forced('Hello', mel=target, audio=np.zeros(4000, np.float32))
    with pytest.raises(ValueError):
        Tacotron2(object(), lang='en').teacher_forced('Hello', mel=target)     # no tacotron2_forward behind the model
    spk = np.random.default_rng(1).standard_normal((3, 256)).astype(np.float32)
    sv = SV2TTSTacotron2(rt, lang='en', embeddings=spk)
    sv.teacher_forced('Hello', mel=target, embeddings=2)
    tokens, emb = rt.calls[-1][0]
    assert tokens.shape[0] == 1 and np.array_equal(emb, spk[2][None])


def test_runtime_forward_uses_seed_and_running_offset_like_infer():
    from text_to_speech_amd.runtime import MASK_STREAM, HipRuntime

    class Eng:
        def __init__(self):
            self.calls = []

        def tacotron2_forward(self, tokens, mel_input, mel_lengths, **kw):
            self.calls.append(kw)
            return 'out'

    eng = Eng()
    rt = HipRuntime('synthetic', engine=eng, seed=11)
    tok, x = np.ones((2, 5), np.int32), np.zeros((2, 6, 80), np.float32)
    assert rt.tacotron2_forward(tok, x, [6, 3]) == 'out'
    rt.tacotron2_forward(tok, x, [6, 3])
    rt.tacotron2_forward(tok, x, [6, 3], seed=5)
    rt.tacotron2_forward(tok, x, [6, 3], deterministic=True)
    rt.tacotron2_forward((tok, np.zeros((2, 256), np.float32)), x, [6, 3], prenet_masks=np.ones((2, 6, 2, 256), np.float32))
    key = (11 ^ MASK_STREAM) & ((1 << 64) - 1)
    step = (2 * 6 * 512 + 3) // 4
    assert (eng.calls[0]['seed'], eng.calls[0]['offset']) == (key, 0)
    assert (eng.calls[1]['seed'], eng.calls[1]['offset']) == (key, step)          # the running offset advanced
    assert (eng.calls[2]['seed'], eng.calls[2]['offset']) == ((5 ^ MASK_STREAM) & ((1 << 64) - 1), 0)
    assert 'seed' not in eng.calls[3] and eng.calls[3]['prenet_masks'] is None
    assert 'seed' not in eng.calls[4] and eng.calls[4]['speaker'] is not None
    assert rt._offset == 2 * step                                                  # seeded / deterministic / explicit: untouched
    before = rt._offset                                                            # the same bookkeeping as tacotron2_infer
    assert all(c['precision'] == 'f32' for c in eng.calls) and before == 2 * step


def test_runtime_forward_runs_on_the_kept_encoded_batch_and_refuses_unknown_keywords():
    """Like tacotron2_infer, the forward call encodes INTO the runtime's one EncodedBatch (no new buffer, so the handle's
    cached chunk graphs survive both calls) and reuses it while the tokens stay the same."""
    from text_to_speech_amd.runtime import HipRuntime

    class Eng:
        def __init__(self):
            self.encodes, self.forwards, self.decodes = [], [], []

        def tacotron2_encode(self, tokens, speaker=None, into=None):
            self.encodes.append(into)
            return into if into is not None else object()

        def tacotron2_forward(self, encoded, mel_input, mel_lengths, **kw):
            self.forwards.append((encoded, kw))
            return 'out'

        def tacotron2_decode(self, encoded, **kw):
            self.decodes.append(encoded)
            return 'dec'

    eng = Eng()
    rt = HipRuntime('synthetic', engine=eng, seed=1)
    tok, other = np.ones((1, 5), np.int32), np.full((1, 5), 2, np.int32)
    x = np.zeros((1, 6, 80), np.float32)
    rt.tacotron2_forward(tok, x, [6], deterministic=True)
    rt.tacotron2_forward(tok, x, [6], deterministic=True)                  # same tokens: the encoder does not run again
    rt.tacotron2_infer(tok, max_length=4, deterministic=True)              # ... nor for infer on them
    rt.tacotron2_forward(other, x, [6], deterministic=True)                # other tokens: encoded INTO the kept batch
    batch = eng.forwards[0][0]
    assert eng.encodes == [None, batch] and rt.encoder_reuses == 2
    assert [f[0] for f in eng.forwards] == [batch] * 3 and eng.decodes == [batch]
    assert 'speaker' not in eng.forwards[0][1] and eng.forwards[0][1]['prenet_masks'] is None
    with pytest.raises(TypeError):
        rt.tacotron2_forward(tok, x, [6], deterministc=True)               # a misspelt keyword must not draw dropout unnoticed
