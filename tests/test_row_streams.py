"""CPU: per-row random streams -- the key function against its known answers, the C ABI presence of the three rows calls,
the ids that `predict(sentence_streams=True)` hands the models on every host path (sequential, overlapped, backlog, packed
backlog), and `synthesize_sharded(with_ids=True)` on a gloo world of 2."""
import os
import re
import socket
from collections import Counter

import numpy as np
import pytest

from text_to_speech_amd.engine import Tacotron2InferenceOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
NEW_CALLS = ('tts_hip_random_fill_rows', 'tts_hip_waveglow_infer_rows_seeded', 'tts_hip_waveglow_infer_rows_seeded_async',
             'tts_hip_tacotron2_decode_rows_seeded')


# ---- 1. keys ---------------------------------------------------------------------------------------------------------------
def _mix64_plain(x):
    x = (x + 0x9E3779B97F4A7C15) % 2 ** 64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    return x ^ (x >> 31)


def _stream_key_plain(seed, purpose, utterance, part, trial):
    k = _mix64_plain(seed ^ purpose)
    for v in (utterance, part, trial):
        k = _mix64_plain(k ^ v)
    return k


def test_stream_key_known_answers():
    from oracle import philox_ref
    from text_to_speech_amd.runtime import MASK_STREAM, NOISE_STREAM, _mix64, stream_key
    assert _mix64(0) == _mix64_plain(0) == 0xe220a8397b1dcdaf          # splitmix64's first output from state 0
    known = [((0, MASK_STREAM, 0, 0, 0), 0x873d084d43f12818),
             ((0, NOISE_STREAM, 0, 0, 0), 0x57027f09e4a2f549),
             ((1234, MASK_STREAM, 7, 1, 2), 0x6d386fd6ef20a096),
             ((1234, NOISE_STREAM, 7, 1, 0), 0xea8b672aa9924f66),
             ((U64, NOISE_STREAM, U64, 0, 0), 0xd8e410e7de8f79d7)]
    for args, want in known:
        assert _stream_key_plain(*args) == want, args
        assert stream_key(*args) == want, args
    assert stream_key(0, MASK_STREAM) == known[0][1]                     # utterance / part / trial default to 0
    assert philox_ref.prenet_masks(16, 0x6d386fd6ef20a096).tolist() == [2, 2, 2, 2, 0, 0, 2, 0, 0, 0, 2, 2, 2, 0, 2, 0]
    rng = np.random.default_rng(0)
    for _ in range(200):
        args = tuple(int(v) for v in rng.integers(0, 2 ** 63, 5))
        assert stream_key(*args) == _stream_key_plain(*args)


def test_distinct_ids_give_distinct_keys():
    from text_to_speech_amd.runtime import MASK_STREAM, NOISE_STREAM, stream_key
    ids = [(u, p, t) for u in range(400) for p in range(5) for t in range(5)]
    assert len(ids) == 10000
    masks = {stream_key(1234, MASK_STREAM, *i) for i in ids}
    noise = {stream_key(1234, NOISE_STREAM, *i) for i in ids}
    assert len(masks) == len(noise) == 10000 and not masks & noise
    assert all(0 <= k <= U64 for k in masks)


# ---- 2. C ABI --------------------------------------------------------------------------------------------------------------
def test_rows_calls_are_declared_bound_and_exported():
    from text_to_speech_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load_library()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tts_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(tts_hip_\w+)\s*\(', src))
    for name in NEW_CALLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tts_hip_abi_version() == 13 == _lib.ABI_VERSION
    # a NULL handle is refused before anything else is looked at
    assert lib.tts_hip_random_fill_rows(None, 0, None, None, 1, 4, None, None, None) == -1
    assert lib.tts_hip_waveglow_infer_rows_seeded(None, None, 1, 1, None, None, None, 1.0, None, 0, 0, 0) == -1
    assert lib.tts_hip_tacotron2_decode_rows_seeded(None, None, 1, 0, None, None, 0, 0, 0, None, None, None, None, None, None,
                                                    0, None) == -1


# ---- 3. host logic ---------------------------------------------------------------------------------------------------------
class RecordingSynth:
    """compiled_infer stand-in that records the keyword arguments of every call.  Every row runs its cap (3 frames a token:
    inside the frame / token window) except rows equal to `failing`, whose first two decodes return one frame."""

    def __init__(self, failing):
        self.failing, self.attempts, self.calls = tuple(int(t) for t in failing), 0, []

    def __call__(self, inputs, max_length=None, **kwargs):
        tok = np.asarray(inputs[0] if isinstance(inputs, tuple) else inputs)
        self.calls.append((tok.copy(), kwargs))
        n_tok = (tok != 0).sum(1)
        cap = max(1, int(np.float32(n_tok.max()) * np.float32(max_length)))
        lengths = np.asarray([max(1, int(np.float32(n) * np.float32(max_length))) for n in n_tok], np.int32)
        for b in range(len(tok)):
            if tuple(int(t) for t in tok[b, :n_tok[b]]) == self.failing:
                if self.attempts < 2:
                    lengths[b] = 1
                self.attempts += 1
        mel = np.zeros((len(tok), cap, 80), np.float32)
        return Tacotron2InferenceOutput(decoder_output=mel, mel=mel, stop_tokens=np.zeros((len(tok), cap), np.float32),
                                        attention_weights=np.zeros((len(tok), cap, tok.shape[1]), np.float32), lengths=lengths)


class RecordingVocoder:
    def __init__(self):
        self.calls = []

    def __call__(self, mel, lengths=None, **kwargs):
        mel = np.asarray(mel)
        self.calls.append((mel.shape[0], None if lengths is None else [int(n) for n in lengths], kwargs))
        return np.zeros((mel.shape[0], mel.shape[1] * 256), np.float32)


TEXTS = ['alpha one.', 'bravo two two.', 'charlie goes first here. charlie goes second there.', 'delta fails twice.',
         'bravo two two.', 'echo five.', 'foxtrot six six six.']
MASK_IDS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (3, 0, 0), (3, 0, 1), (3, 0, 2), (5, 0, 0), (6, 0, 0)]
NOISE_IDS = [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (5, 0), (6, 0)]


def _run(**kw):
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    probe = Tacotron2(None)
    synth = RecordingSynth(probe.encode_text(probe.clean_text(TEXTS[3]), cleaned=True))
    fake_voc = RecordingVocoder()
    seen = []
    res = Tacotron2(synth).predict(list(TEXTS), vocoder=WaveGlow(fake_voc), save=False, max_length=3., max_text_length=30,
                                   seed=5, callbacks=[lambda text, **_: seen.append(text)], **kw)
    assert seen == TEXTS and len(res) == len(TEXTS)
    assert [len(r['splitted']) for r in res] == [1, 1, 2, 1, 1, 1, 1]
    return synth, fake_voc


def _ids(calls, kwargs_at):
    out = []
    for call in calls:
        kwargs = call[kwargs_at]
        assert kwargs.get('seed') == 5                               # the key base travels with the ids
        out.extend(tuple(i) for i in kwargs['streams'])
        n_rows = len(call[0]) if kwargs_at == 1 else call[0]
        assert len(kwargs['streams']) == n_rows                      # one id per row
    return out


@pytest.mark.parametrize('mode', [{}, {'batch_backlog': 3}, {'batch_backlog': 3, 'pack_vocoder': True}, {'overlap': True}],
                         ids=['sequential', 'backlog', 'packed-backlog', 'overlap'])
def test_every_host_path_hands_the_models_the_same_ids(mode):
    """7 inputs: one split into two parts, one repeated (served from the cache: it consumes utterance number 4), one whose
    first two trials fail the frame / token ratio test."""
    synth, voc = _run(sentence_streams=True, **mode)
    assert Counter(_ids(synth.calls, 1)) == Counter(MASK_IDS)
    assert Counter(_ids(voc.calls, 2)) == Counter(NOISE_IDS)
    assert synth.attempts == 3
    if 'batch_backlog' in mode:
        assert max(len(tok) for tok, _ in synth.calls) == 3 and any(c[0] > 1 for c in voc.calls)
        assert all(bool(c[2].get('packed')) == bool(mode.get('pack_vocoder')) for c in voc.calls if c[0] > 1)
        # the failing row was first decoded beside its neighbours, then again alone: only its own trial advanced
        first = next(kw['streams'] for _, kw in synth.calls if (3, 0, 0) in [tuple(i) for i in kw['streams']])
        assert sorted(tuple(i) for i in first) == [(3, 0, 0), (5, 0, 0), (6, 0, 0)]
        retries = [[tuple(i) for i in kw['streams']] for _, kw in synth.calls if any(tuple(i)[2] > 0 for i in kw['streams'])]
        assert retries == [[(3, 0, 1)], [(3, 0, 2)]]
    else:
        assert all(len(tok) == 1 for tok, _ in synth.calls)


@pytest.mark.parametrize('mode', [{}, {'batch_backlog': 3}, {'overlap': True}], ids=['sequential', 'backlog', 'overlap'])
def test_without_sentence_streams_no_streams_keyword_is_passed(mode):
    synth, voc = _run(**mode)
    assert synth.calls and voc.calls
    assert all('streams' not in kw and 'utterance' not in kw and 'sentence_streams' not in kw for _, kw in synth.calls)
    assert all('streams' not in c[2] and 'utterance' not in c[2] and 'sentence_streams' not in c[2] for c in voc.calls)


def test_runtime_turns_ids_into_row_keys():
    """`HipRuntime(streams=...)` on a recording engine: one key per row from (seed or the runtime's seed, purpose, id) at
    offset 0; the running offset is neither used nor advanced; exclusive with explicit draws and deterministic=True."""
    from text_to_speech_amd.runtime import MASK_STREAM, NOISE_STREAM, HipRuntime, stream_key

    class Engine:
        def __init__(self):
            self.calls = []

        def waveglow_infer(self, mel, **kw):
            self.calls.append(('wg', kw))
            return np.zeros((mel.shape[0], mel.shape[1] * 256), np.float32)

        def tacotron2_infer(self, tokens, **kw):
            self.calls.append(('taco', kw))
            return None

    eng = Engine()
    rt = HipRuntime('none', engine=eng, seed=77)
    mel = np.zeros((2, 3, 80), np.float32)
    rt.waveglow_infer(mel, streams=[(4, 1), 9], lengths=[3, 2], packed=True)
    rt.waveglow_infer(mel, streams=[(4, 1), (9, 0)], seed=5)
    tok = np.ones((2, 6), np.int32)
    rt.tacotron2_infer(tok, max_length=8, streams=[(4, 1, 2), (9,)])
    rt.tacotron2_infer(tok, max_length=8, streams=[(4, 1, 2), (9, 0, 0)], seed=5)
    assert rt._offset == 0
    (_, a), (_, b), (_, c), (_, d) = eng.calls
    assert a['row_seeds'] == ([stream_key(77, NOISE_STREAM, 4, 1, 0), stream_key(77, NOISE_STREAM, 9, 0, 0)], [0, 0])
    assert a['packed'] is True and list(a['lengths']) == [3, 2] and 'seed' not in a and 'z' not in a
    assert b['row_seeds'] == ([stream_key(5, NOISE_STREAM, 4, 1, 0), stream_key(5, NOISE_STREAM, 9, 0, 0)], [0, 0])
    assert c['row_mask_seeds'] == ([stream_key(77, MASK_STREAM, 4, 1, 2), stream_key(77, MASK_STREAM, 9, 0, 0)], [0, 0])
    assert d['row_mask_seeds'] == ([stream_key(5, MASK_STREAM, 4, 1, 2), stream_key(5, MASK_STREAM, 9, 0, 0)], [0, 0])
    assert c.get('prenet_masks') is None
    for bad in (dict(streams=[(0, 0)]), dict(streams=[(0, 0), (1, 0)], deterministic=True),
                dict(streams=[(0, 0), (1, 0)], z=np.zeros((2, 96, 8), np.float32)), dict(streams=[(0, 0, 0, 0), (1,)])):
        with pytest.raises(ValueError):
            rt.waveglow_infer(mel, **bad)
    for bad in (dict(streams=[(0,)]), dict(streams=[(0,), (1,)], deterministic=True),
                dict(streams=[(0,), (1,)], prenet_masks=np.zeros((2, 8, 2, 256), np.float32))):
        with pytest.raises(ValueError):
            rt.tacotron2_infer(tok, max_length=8, **bad)
    assert len(eng.calls) == 4 and rt._offset == 0


# ---- 4. sharding -----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ids_worker(rank, world, port, n_utt, ret):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from text_to_speech_amd.distributed import partition, synthesize_sharded
    rng = np.random.default_rng(0)
    lens = rng.integers(3, 20, n_utt)
    tok = np.zeros((n_utt, 24), np.int32)
    for i, n in enumerate(lens):
        tok[i, :n] = rng.integers(1, 148, n)
    got = []

    def synth(local_tok, local_spk, ids):
        """utterance `i` with n tokens -> n * 7 samples of value i"""
        got.append(list(ids))
        t = local_tok.cpu().numpy()
        n = (t != 0).sum(1)
        audio = np.zeros((t.shape[0], max(1, int(n.max()) * 7)), np.float32)
        for r, i in enumerate(ids):
            audio[r, :n[r] * 7] = i
        return audio, n * 7

    out = synthesize_sharded(tok if rank == 0 else None, synth, with_ids=True)
    mine = partition(lens.tolist(), world)[rank]
    ok = got == ([mine] if mine else []) and all(isinstance(i, int) for ids in got for i in ids)
    if rank == 0:
        ok &= len(out) == n_utt
        for i in range(n_utt):
            ok &= out[i].shape == (lens[i] * 7,) and bool(np.all(out[i] == i))          # gathered in input order
    else:
        ok &= out is None
    ret.put(bool(ok))
    dist.destroy_process_group()


@pytest.mark.parametrize('n_utt', [7, 1])
def test_sharded_synth_gets_its_global_indices_world2(n_utt):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    ret = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_ids_worker, args=(r, 2, port, n_utt, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert ret.get() is True and ret.get() is True


def test_pipeline_row_ids_use_the_unranked_job_seed():
    """`synthesize_tokens(row_ids=...)` on a recording engine: keys from the job seed as given, whatever the rank."""
    torch = pytest.importorskip('torch')
    from text_to_speech_amd.pipeline import TTSPipeline
    from text_to_speech_amd.runtime import MASK_STREAM, stream_key

    class Stop(Exception):
        pass

    class Engine:
        device = 0

        def tacotron2_infer(self, tok, **kw):
            self.kw = kw
            raise Stop

    seen = []
    for rank in (0, 3):
        eng = Engine()
        pipe = TTSPipeline(eng, seed=9, rank=rank)
        real = torch.device
        try:
            torch.device = lambda *a, **k: real('cpu')                       # no GPU here: the tensors stay on the host
            with pytest.raises(Stop):
                pipe.synthesize_tokens(np.ones((2, 5), np.int32), max_length=4, row_ids=[11, 2])
            with pytest.raises(ValueError):
                pipe.synthesize_tokens(np.ones((2, 5), np.int32), max_length=4, row_ids=[11, 2], deterministic=True)
            with pytest.raises(ValueError):
                pipe.synthesize_tokens(np.ones((2, 5), np.int32), max_length=4, row_ids=[11])
        finally:
            torch.device = real
        assert pipe._offset == 0 and eng.kw.get('prenet_masks') is None
        seen.append(eng.kw['row_mask_seeds'])
    assert seen[0] == seen[1] == ([stream_key(9, MASK_STREAM, 11), stream_key(9, MASK_STREAM, 2)], [0, 0])
