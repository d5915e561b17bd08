"""CPU: `predict(batch_backlog=k)` / `stream(batch_backlog=k)` host logic with a fake synthesizer and vocoder -- grouping of
what is waiting, callback order, per-row frame caps and retries, repeats and cached texts, the refusal of `overlap=True` --
and the argument checking / C ABI presence of the ragged WaveGlow entry points it stands on."""
import queue

import numpy as np
import pytest

from text_to_speech_amd.engine import Tacotron2InferenceOutput


class BatchSynth:
    """compiled_infer stand-in for token batches: row b runs `frames(n_tok_b, call_index, row_tokens)` frames (default:
    never stops, i.e. the runtime's cap for the LONGEST row, as synthetic weights do); mel[b, t, 0] = t,
    mel[b, t, 1] = the row's token count, so that a waveform can be traced to its row and frame."""

    def __init__(self, frames=None):
        self.frames = frames
        self.calls = []

    def __call__(self, inputs, max_length=None, **kwargs):
        tok = np.asarray(inputs[0] if isinstance(inputs, tuple) else inputs)
        self.calls.append((tok.copy(), max_length, kwargs, inputs[1] if isinstance(inputs, tuple) else None))
        n_tok = (tok != 0).sum(1)
        cap = max(1, int(np.float32(n_tok.max()) * np.float32(max_length)))
        lengths = np.full(len(tok), cap, np.int32)
        if self.frames is not None:
            lengths = np.asarray([min(cap, self.frames(int(n), len(self.calls) - 1, tok[b])) for b, n in enumerate(n_tok)], np.int32)
        mel = np.zeros((len(tok), cap, 80), np.float32)
        mel[:, :, 0] = np.arange(cap)
        mel[:, :, 1] = n_tok[:, None]
        return Tacotron2InferenceOutput(decoder_output=mel, mel=mel, stop_tokens=np.zeros((len(tok), cap), np.float32),
                                        attention_weights=np.zeros((len(tok), cap, tok.shape[1]), np.float32), lengths=lengths)


class RaggedVocoder:
    """WaveGlow.compiled_infer stand-in with the ragged contract: sample k of frame t of a row = mel[t, 1] * 1000 + t + k / 256
    inside the row's length, 0 beyond it."""

    def __init__(self):
        self.calls = []

    def __call__(self, mel, lengths=None, **kwargs):
        mel = np.asarray(mel)
        B, T = mel.shape[:2]
        self.calls.append((B, T, None if lengths is None else list(map(int, lengths))))
        t = np.repeat(np.arange(T), 256) + np.tile(np.arange(256) / 256., T)
        out = np.repeat(mel[:, :, 1], 256, axis=1) * 1000 + t[None]
        if lengths is not None:
            for b, n in enumerate(lengths):
                out[b, int(n) * 256:] = 0
        return out.astype(np.float32)


def _texts(n):
    return [f'sentence number {i:02d} ' + 'ab' * (i % 7 + 1) + '.' for i in range(n)]


def _n_tok(texts):
    from text_to_speech_amd.tacotron2 import Tacotron2
    m = Tacotron2(None)
    return [len(m.encode_text(m.clean_text(t), cleaned=True)) for t in texts]


def _models():
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    synth, voc = BatchSynth(), RaggedVocoder()
    return Tacotron2(synth), WaveGlow(voc), synth, voc


def _run(texts, **kw):
    model, voc, synth, fake_voc = _models()
    rec = []
    res = model.predict(texts, vocoder=voc, save=False, max_length=3.,
                        callbacks=[lambda text, audio=None, **_: rec.append((text, None if audio is None else np.asarray(audio).copy()))],
                        **kw)
    return res, rec, synth, fake_voc


def test_backlog_groups_take_what_is_waiting():
    from text_to_speech_amd.tacotron2 import _backlog_groups
    sizes = lambda src, k=8: [len(g) for g in _backlog_groups(src, k)]
    for n, want in ((1, [1]), (3, [3]), (20, [8, 8, 4])):
        q = queue.Queue()
        for t in _texts(n) + [None]:
            q.put(t)
        assert sizes(q) == want and q.empty()
        assert sizes(_texts(n)) == want and sizes(iter(_texts(n))) == want
    # the terminator ends the stream even when more follows; dict inputs are grouped by their text
    q = queue.Queue()
    for t in ['a.', {'text': 'b.'}, None, 'c.']:
        q.put(t)
    assert [[t for _, t in g] for g in _backlog_groups(q, 8)] == [['a.', 'b.']] and q.get_nowait() == 'c.'
    # a repeat closes the group; cached texts ride along without counting
    assert [[t for _, t in g] for g in _backlog_groups(['a', 'b', 'a', 'c'], 8)] == [['a', 'b'], ['a', 'c']]
    assert sizes(['x', 'a', 'b', 'c'], 2) == [2, 2]
    assert [len(g) for g in _backlog_groups(['x', 'a', 'b', 'c'], 2, lambda t: t == 'x')] == [3, 1]


def test_backlog_equals_the_sequential_path_in_results_and_callback_order():
    texts = _texts(20)
    seq_res, seq_rec, seq_synth, seq_voc = _run(texts)
    res, rec, synth, voc = _run(texts, batch_backlog=8)
    assert [t for t, _ in rec] == [t for t, _ in seq_rec] == texts
    assert [r['text'] for r in res] == texts and len(res) == len(seq_res)
    for (_, a), (_, b), r, s in zip(rec, seq_rec, res, seq_res):
        assert a.shape == b.shape and np.array_equal(a, b)              # per-row caps: every sentence ends where it ends alone
        assert set(r) == set(s) and r['cleaned'] == s['cleaned'] and r['splitted'] == s['splitted'] and r['time'] == s['time']
        assert len(r['mel']) == 1 and np.array_equal(r['mel'][0], s['mel'][0])
        assert r['attention'][0].shape == s['attention'][0].shape
    # 20 sentences: decoder batches of 8, 8, 4 rows and one ragged vocoder call per group
    assert [len(c[0]) for c in synth.calls] == [8, 8, 4] and len(seq_synth.calls) == 20
    assert [c[0] for c in voc.calls] == [8, 8, 4] and all(c[2] is not None for c in voc.calls)
    assert all(c[2] is None for c in seq_voc.calls)
    n_tok = _n_tok(texts[:8])
    assert voc.calls[0][2] == [int(np.float32(n) * np.float32(3.)) for n in n_tok] and voc.calls[0][1] == max(voc.calls[0][2])
    # batch_backlog None / 1: today's loop
    _, rec1, synth1, _ = _run(texts[:3], batch_backlog=1)
    assert len(synth1.calls) == 3 and [t for t, _ in rec1] == texts[:3]


def test_backlog_queue_stream_and_lone_sentences():
    from text_to_speech_amd.tacotron2 import stream
    model, voc, synth, fake_voc = _models()
    texts = _texts(11)
    q = queue.Queue()
    for t in texts + [None]:
        q.put(t)
    rec = []
    assert stream(q, model=model, vocoder=voc, save=False, max_length=3., batch_backlog=8,
                  callbacks=[lambda text, **_: rec.append(text)]) == []
    assert rec == texts
    # the two warm-up sentences of precompile_for_stream, then groups of 8 and 3
    assert [len(c[0]) for c in synth.calls] == [1, 1, 8, 3]
    # a queue fed one item at a time never has a backlog: every sentence takes the batch-1 path
    model, voc, synth, fake_voc = _models()
    q = queue.Queue()
    q.put(texts[0])
    fed = iter(texts[1:4] + [None])
    model.predict(q, vocoder=voc, save=False, max_length=3., batch_backlog=8, return_results=False,
                  callbacks=[lambda **_: q.put(next(fed))])
    assert [len(c[0]) for c in synth.calls] == [1, 1, 1, 1] and all(c[2] is None for c in fake_voc.calls)


def test_backlog_retries_only_the_rows_that_fail_the_ratio(caplog):
    import logging
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    texts = _texts(4)
    n_tok = _n_tok(texts)
    assert len(set(n_tok)) == 4
    # row 2 gives one frame per token on the first call (ratio 1 <= min_fpt_ratio 2), then behaves
    synth = BatchSynth(lambda n, call, row: n if (call == 0 and n == n_tok[2]) else 10 ** 6)
    fake_voc = RaggedVocoder()
    with caplog.at_level(logging.INFO, logger='text_to_speech_amd.tacotron2'):
        res = Tacotron2(synth).predict(texts, vocoder=WaveGlow(fake_voc), save=False, max_length=3., batch_backlog=8)
    assert [len(c[0]) for c in synth.calls] == [4, 1] and (synth.calls[1][0] != 0).sum() == n_tok[2]
    assert sum('Inference failed (lengths' in r.message for r in caplog.records) == 1
    assert [r['mel'][0].shape[0] for r in res] == [int(np.float32(n) * np.float32(3.)) for n in n_tok]
    # a row that never passes is decoded max_trial times and keeps its last result, with the sequential path's warning
    synth = BatchSynth(lambda n, call, row: n if n == n_tok[1] else 10 ** 6)
    with caplog.at_level(logging.INFO, logger='text_to_speech_amd.tacotron2'):
        caplog.clear()
        res = Tacotron2(synth).predict(texts, vocoder=WaveGlow(fake_voc), save=False, max_length=3., batch_backlog=8, max_trial=3)
    assert [len(c[0]) for c in synth.calls] == [4, 1, 1] and res[1]['mel'][0].shape[0] == n_tok[1]
    assert sum('failed too much time' in r.message for r in caplog.records) == 1
    # an integer max_length caps every row alike
    synth = BatchSynth()
    res = Tacotron2(synth).predict(texts, save=False, max_length=3., batch_backlog=2)
    assert [len(c[0]) for c in synth.calls] == [2, 2] and 'audio' not in res[0]


def test_backlog_repeats_and_cached_texts_are_served_like_the_sequential_stream():
    texts = _texts(3)
    order = [texts[0], texts[1], texts[0], texts[2], texts[1]]
    seq_res, seq_rec, seq_synth, _ = _run(order)
    res, rec, synth, voc = _run(order, batch_backlog=8)
    assert [t for t, _ in rec] == [t for t, _ in seq_rec] == order
    # the first occurrences are synthesized (groups [0, 1] and [2]: the repeat of text 0 closed the first group and is a cache
    # hit by then), the repeats replayed from `predicted`: the same number of synthesized rows as the sequential stream
    assert sum(len(c[0]) for c in synth.calls) == len(seq_synth.calls) == 3
    assert [len(c[0]) for c in synth.calls] == [2, 1]
    for (_, a), (_, b) in zip(rec, seq_rec):                             # (a replayed entry carries no waveform)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    assert [a is None for _, a in rec] == [False, False, True, False, True]
    # texts already in the caller's `predicted` map are not synthesized
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    synth, seen = BatchSynth(), []
    predicted = {texts[1]: {'text': texts[1], 'audio': 'kept.wav'}}
    out = Tacotron2(synth).predict(texts, vocoder=WaveGlow(RaggedVocoder()), predicted=predicted, max_length=3., batch_backlog=8,
                                   callbacks=[lambda text, **kw: seen.append((text, kw.get('audio')))], return_output=False)
    assert [len(c[0]) for c in synth.calls] == [2] and [t for t, _ in seen] == texts and seen[1][1] == 'kept.wav'
    assert out[1] == predicted[texts[1]]


def test_backlog_refuses_overlap_and_bad_values():
    model, voc, _, _ = _models()
    with pytest.raises(ValueError, match='overlap'):
        model.predict(_texts(2), vocoder=voc, save=False, batch_backlog=4, overlap=True)
    with pytest.raises(ValueError):
        model.predict(_texts(2), vocoder=voc, save=False, batch_backlog=0)


def test_backlog_sv2tts_selects_one_embedding_per_call():
    from text_to_speech_amd.tacotron2 import SV2TTSTacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    synth = BatchSynth()
    pool = np.arange(12, dtype=np.float32).reshape(3, 4)
    model = SV2TTSTacotron2(synth, lang='en', embeddings=pool, embedding_dim=4)
    model.predict(_texts(3), vocoder=WaveGlow(RaggedVocoder()), save=False, max_length=3., batch_backlog=8, embeddings=2)
    assert len(synth.calls) == 1 and synth.calls[0][3].shape == (3, 4) and (synth.calls[0][3] == pool[2]).all()


def test_waveglow_infer_checks_lengths_before_any_device_call():
    from text_to_speech_amd import _lib
    from text_to_speech_amd.engine import HipEngine
    assert HipEngine._frame_lengths([3, 0, 5], 3, 5).tolist() == [3, 0, 5]
    assert HipEngine._frame_lengths(np.asarray([2], np.int64), 1, 2).dtype == np.int32
    for bad, B, T in (([6, 1], 2, 5), ([-1, 1], 2, 5), ([1], 2, 5), ([1.0, 2.0], 2, 5), ([[1, 2]], 2, 5)):
        with pytest.raises(ValueError):
            HipEngine._frame_lengths(bad, B, T)
    eng = HipEngine.__new__(HipEngine)                 # no handle: the check must come before the library is called
    eng._lib, eng._h = _lib.load_library(), None
    with pytest.raises(ValueError, match='lengths'):
        eng.waveglow_infer(np.zeros((2, 5, 80), np.float32), lengths=[5, 6])


def test_ragged_entry_points_are_declared_bound_and_exported():
    import ctypes
    import os
    import re
    from text_to_speech_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'tts_hip.h')).read()
    lib = _lib.load_library()
    for name in ('tts_hip_waveglow_infer_ragged', 'tts_hip_waveglow_infer_ragged_async'):
        assert re.search(r'\bint\s+%s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == 10
    assert lib.tts_hip_abi_version() == 13            # additions only
    assert lib.tts_hip_waveglow_infer_ragged(None, None, 1, 1, None, None, ctypes.c_float(1.0), None, 0, 0) == -1
