"""GPU: what stands on the ragged WaveGlow call -- `TTSPipeline.synthesize_tokens(ragged=True)` against the oracle on each
row's own mel, and `stream(batch_backlog=8)` against the sequential stream on the same engine."""
import queue

import numpy as np
import pytest

from conftest import rms
from stop_script import script_stop_tokens

pytestmark = pytest.mark.gpu

MEL_TOL, WAVE_RMS_TOL = 1e-3, 1e-4                  # fp32 (north_star; tests/test_configs_gpu.py)
CONFIG3_TOKENS = [50, 70, 90, 110, 130, 150, 170, 200]

_WORDS = ('the quick brown fox jumps over a lazy dog while seven wizards quietly box with five jumping zebras and '
          'every good vocoder makes sharp clear audio from a plain spectrogram without any audible glitch').split()


def _sentences(n, seed=0):
    """n pseudo sentences whose character counts cycle through the config-3 set (50 .. 200)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        want, words = CONFIG3_TOKENS[i % len(CONFIG3_TOKENS)], []
        while sum(len(w) + 1 for w in words) < want - 1:
            words.append(_WORDS[int(rng.integers(len(_WORDS)))])
        s = ' '.join(words)[:want - 1].rstrip()
        s += 's' * (want - 1 - len(s)) + '.'
        out.append(s[0].upper() + s[1:])
    return out


def test_pipeline_ragged_rows_match_the_oracle_on_their_own_mel(taco_cfg, taco_weights, wg_weights, wg_cfg):
    """Config 3's recipe (batch 8, 50 .. 200 tokens, scripted stops at 12 .. 40 frames) in fp32 with `ragged=True`: the
    shortest and the longest row against oracle Tacotron2 -> oracle WaveGlow on the row's OWN frames (no -11 tail), at the
    fp32 waveform tolerance; `ragged=False` stays the padded path, bit for bit."""
    from oracle import tacotron2_ref, waveglow_ref
    from text_to_speech_amd.engine import HipEngine
    from text_to_speech_amd.pipeline import PAD_MEL_VALUE, TTSPipeline
    tok = np.zeros((8, 256), np.int32)
    for i, n in enumerate(CONFIG3_TOKENS):
        tok[i, :n] = np.random.default_rng(6 + i).integers(1, 148, n)
    targets = [12, 17, 23, 21, 28, 33, 37, 40]
    tw, _, _ = script_stop_tokens(taco_weights, taco_cfg, tok, targets)
    ref = tacotron2_ref.infer(tok, tw, taco_cfg, max_length=64, early_stopping=True)
    assert ref.lengths.tolist() == targets
    z = np.random.default_rng(11).standard_normal((8, 40 * 32, 8)).astype(np.float32)
    eng = HipEngine(0)
    try:
        eng.load_state(tw)
        eng.load_state(wg_weights)
        eng.finalize()
        pipe = TTSPipeline(eng)
        audios, n, steps = pipe.synthesize_tokens(tok, max_length=64, deterministic=True, z=z, ragged=True)
        assert n.tolist() == targets and steps == max(targets) + 1
        for b in (0, 7):
            t = targets[b]
            ref_audio = waveglow_ref.infer(ref.mel[b:b + 1, :t], wg_weights, wg_cfg, z=z[b:b + 1, :t * 32])[0]
            assert audios[b].shape == ref_audio.shape == (t * 256,)
            e = rms(audios[b] - ref_audio)
            print(f'ragged pipeline: row {b} ({t} frames) waveform RMS err vs its own oracle {e:.2e}')
            assert e <= WAVE_RMS_TOL
        assert all(a.shape == (targets[b] * 256,) and np.isfinite(a).all() for b, a in enumerate(audios))
        # ragged=False (the default): the padded call spelled out
        padded, n2, _ = pipe.synthesize_tokens(tok, max_length=64, deterministic=True, z=z, ragged=False)
        default, _, _ = pipe.synthesize_tokens(tok, max_length=64, deterministic=True, z=z)
        out = eng.tacotron2_infer(tok, max_len=64, early_stopping=True, want_attention=False)
        mel = out.mel[:, :40].copy()
        for b in range(8):
            mel[b, targets[b]:] = PAD_MEL_VALUE
        today = eng.waveglow_infer(mel, z=z)
        for b in range(8):
            assert np.array_equal(padded[b], today[b, :targets[b] * 256]) and np.array_equal(default[b], padded[b])
        d = rms(padded[0] - audios[0])
        print(f'row 0: padded vs ragged waveform RMS difference {d:.2e}')
        assert d > 100 * WAVE_RMS_TOL                                    # what the padded batch does to its shortest row
    finally:
        eng.close()


def test_stream_backlog_against_the_sequential_stream(gpu_engine):
    """16 sentences (50 .. 200 characters), fp32, deterministic: `batch_backlog=8` delivers the same texts in the same
    order with the same sample counts; groups run the fused decoder step; each mel within MEL_TOL of the sequential stream's
    (the bound batch-8 rows are held to against batch-1 runs); each waveform within 5e-6 RMS of a batch-1 vocoding of its own
    backlog mel (the vocoder's ragged contract).  The audio difference to the sequential stream -- the decoder machines'
    re-association seen through WaveGlow -- is printed, not gated.  A queue that never holds a backlog gives the sequential
    stream's audio bit for bit."""
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2, stream
    from text_to_speech_amd.waveglow import WaveGlow
    model = Tacotron2(HipRuntime('t6', model='tacotron2', engine=gpu_engine, seed=0))
    voc = WaveGlow(HipRuntime('w6', model='waveglow', engine=gpu_engine, seed=0))
    texts = _sentences(16)
    assert len(set(texts)) == 16
    run_kw = dict(model=model, vocoder=voc, max_length=3., deterministic=True, save=False)

    def record(rec):
        return [lambda text, audio, mel, **_: rec.append((text, np.asarray(audio).copy(), [np.asarray(m).copy() for m in mel],
                                                          gpu_engine.last_decoder_mode))]

    seq, back, slow = [], [], []
    stream(iter(texts), callbacks=record(seq), **run_kw)
    stream(iter(texts), callbacks=record(back), batch_backlog=8, **run_kw)
    assert [r[0] for r in seq] == [r[0] for r in back] == texts
    assert all(r[3] == 'fused' for r in back)
    n_tok = [len(model.encode_text(model.clean_text(t), cleaned=True)) for t in texts]
    worst_mel = worst_own = worst_seq = 0.0
    for (t, a, m, _), (_, b, mb, _), n in zip(seq, back, n_tok):
        frames = int(np.float32(n) * np.float32(3.))
        assert a.shape == b.shape == (frames * 256,) and np.isfinite(b).all()
        assert len(m) == len(mb) == 1 and m[0].shape == mb[0].shape == (frames, 80)
        worst_mel = max(worst_mel, float(np.abs(m[0] - mb[0]).max()))
        own = np.asarray(voc(mb[0][None], deterministic=True))[0]
        worst_own = max(worst_own, rms(own - b))
        worst_seq = max(worst_seq, rms(a - b))
    print(f'backlog stream vs sequential: mel max abs diff {worst_mel:.2e}; audio RMS diff to a batch-1 vocoding of the own '
          f'mel {worst_own:.2e}; audio RMS diff to the sequential stream (not gated) {worst_seq:.2e}')
    assert worst_mel <= MEL_TOL
    assert worst_own <= 5e-6
    # fed one sentence at a time: no backlog, the old path
    q = queue.Queue()
    q.put(texts[0])
    fed = iter(texts[1:5] + [None])
    stream(q, callbacks=record(slow) + [lambda **_: q.put(next(fed))], batch_backlog=8, **run_kw)
    assert [r[0] for r in slow] == texts[:5]
    for (_, a, _, _), (_, b, _, _) in zip(seq, slow):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        stream(iter(texts[:2]), batch_backlog=8, overlap=True, **run_kw)
