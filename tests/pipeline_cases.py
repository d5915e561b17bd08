"""The sentence pipeline (`Tacotron2.predict / infer / stream`, `SV2TTSTacotron2`, `HipRuntime`, `TTSPipeline`) over fake
models: the scenarios of tests/golden/pipeline_trace.json and the `trace()` that runs them.

`trace()` returns plain JSON-able data, scenario by scenario: what the fake synthesizer, vocoder and engine were called
with, what the callbacks and savers saw, what came back and what the `predicted` map held at the end.  The fakes produce
integers and dyadic fractions only, so the float64 sum of an array is an exact checksum.  Synthesizer and vocoder calls
are recorded in separate lists: how they interleave under `overlap=True` is thread timing, not behaviour.
A synthesizer call is recorded as [tokens, max_length, keywords, speaker], a vocoder call as [mel shape, lengths, keywords],
an event as ['call', text, audio] / ['save', file name, audio] / ['join'], a waveform as [samples, sum], `gave_up` counts the
warnings (one per row that never passed the frame / token test), a runtime step as
[name, the engine's calls, what was raised, the running offset after it, encoder_reuses, whether an encoded batch is held].
scripts/make_pipeline_fixture.py writes the fixture; tests/test_pipeline_trace.py compares against it.
"""
import logging
import queue
import random

import numpy as np

from text_to_speech_amd.engine import Tacotron2InferenceOutput


def _cap(n_tok, max_length, default=2000):
    """The frame budget the runtime gives a batch whose longest row has `n_tok` tokens (written out here on purpose)."""
    if max_length is None:
        return default
    if isinstance(max_length, float):
        return max(1, int(np.float32(n_tok) * np.float32(max_length)))
    return max(1, int(max_length))


def _plain(x):
    """Keyword values -> JSON: tuples become lists, arrays a string of their type, shape and exact sum."""
    if isinstance(x, dict):
        return {str(k): _plain(x[k]) for k in sorted(x)}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        return f'{x.dtype}{list(x.shape)} sum {float(np.asarray(x, np.float64).sum())!r}'
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return type(x).__name__


def _wave(a):
    """A waveform -> [samples, exact sum]."""
    a = np.asarray(a)
    return [int(a.shape[0]), float(a.astype(np.float64).sum())]


# ---- fakes -----------------------------------------------------------------------------------------------------------------
class FakePostnetEngine:
    """The `engine` of a synthesizer that can redo the postnet of cut rows: the redone mel is the decoder output with 0.25 in
    channel 3, where the batch's own postnet wrote 0.5."""

    def __init__(self):
        self.calls = []

    def tacotron2_postnet(self, dec, last):
        dec = np.array(dec, np.float32)
        self.calls.append({'shape': list(dec.shape), 'last': [int(n) for n in last]})
        dec[:, :, 3] = 0.25
        return dec


class FakeSynth:
    """compiled_infer stand-in for token batches.  Row b runs `frames(n_tok_b, attempt, row_tokens)` frames, capped by the
    batch's budget (`attempt`: how often these tokens were decoded before); the default is the row's own budget, 'never'
    the batch's (what synthetic weights do: the stop token never fires).  decoder_output[b, t] = (t, n_tok_b, 0, 0, ...); mel
    is that with 0.5 in channel 3."""

    def __init__(self, frames=None, postnet=False):
        self.frames, self.calls, self.attempts = frames, [], {}
        if postnet:
            self.engine = FakePostnetEngine()

    def __call__(self, inputs, max_length=None, **kwargs):
        tok = np.asarray(inputs[0] if isinstance(inputs, tuple) else inputs)
        speaker = None if not isinstance(inputs, tuple) else np.asarray(inputs[1]).tolist()
        self.calls.append([tok.tolist(), max_length, _plain(kwargs), speaker])        # SYNTH_CALL
        n_tok = (tok != 0).sum(1)
        cap = _cap(int(n_tok.max()), max_length)
        lengths = []
        for b, n in enumerate(n_tok):
            key = tuple(int(t) for t in tok[b, :n])
            attempt = self.attempts.get(key, 0)
            self.attempts[key] = attempt + 1
            want = cap if self.frames == 'never' else _cap(int(n), max_length) if self.frames is None \
                else self.frames(int(n), attempt, key)
            lengths.append(min(cap, want))
        dec = np.zeros((len(tok), cap, 80), np.float32)
        dec[:, :, 0] = np.arange(cap)
        dec[:, :, 1] = n_tok[:, None]
        mel = dec.copy()
        mel[:, :, 3] = 0.5
        return Tacotron2InferenceOutput(decoder_output=dec, mel=mel, stop_tokens=np.zeros((len(tok), cap), np.float32),
                                        attention_weights=np.zeros((len(tok), cap, tok.shape[1]), np.float32),
                                        lengths=np.asarray(lengths, np.int32))


class FakeVocoder:
    """WaveGlow.compiled_infer stand-in with the ragged contract: sample k of frame t of a row = mel[t, 1] * 1000 + t + k / 256
    inside the row's length, 0 beyond it."""

    def __init__(self):
        self.calls = []

    def __call__(self, mel, lengths=None, **kwargs):
        mel = np.asarray(mel)
        B, T = mel.shape[:2]
        self.calls.append([list(mel.shape), None if lengths is None else [int(n) for n in lengths], _plain(kwargs)])
        t = np.repeat(np.arange(T), 256) + np.tile(np.arange(256) / 256., T)
        out = np.repeat(mel[:, :, 1], 256, axis=1) * 1000 + t[None]
        if lengths is not None:
            for b, n in enumerate(lengths):
                out[b, int(n) * 256:] = 0
        return out.astype(np.float32)


def _recorders(events):
    """A function callback (sees every result, replays included), a file saver (skipped when a cached entry is replayed with
    save=False; it writes its file name into the entry) and a callback whose `join` is recorded."""
    from text_to_speech_amd.callbacks import Callback, FileSaver, FunctionCallback

    def seen(text, audio=None, **_):
        events.append(['call', text, audio if audio is None or isinstance(audio, str) else _wave(audio)])

    def save(filename, data, **_):
        events.append(['save', filename, _wave(data)])

    class Joined(Callback):
        def apply(self, infos, output, **_):
            return None

        def join(self):
            events.append(['join'])

    return [FunctionCallback(seen), FileSaver('audio', 'audio-{}.mem', index=0, save_fn=save), Joined()]


ALL_KEYS = 'attention audio cleaned mel rate splitted text time'


def _result(r):
    """A result dict -> [its keys ('all': ALL_KEYS), text, splitted, time, per part [mel shape, mel sum, attention shape],
    audio]."""
    parts = None
    if 'mel' in r:
        parts = [[list(np.shape(m)), float(np.asarray(m, np.float64).sum()), list(np.shape(a))]
                 for m, a in zip(r['mel'], r['attention'])]
    audio, keys, seconds = r.get('audio'), ' '.join(sorted(r)), r.get('time')
    if audio is not None and not isinstance(audio, str):
        audio = _wave(audio)
        if seconds == audio[0] / 22050:
            seconds = 'samples / 22050'
    return ['all' if keys == ALL_KEYS else keys, r.get('text'), r.get('splitted'), seconds, parts, audio]


# ---- the sentences -----------------------------------------------------------------------------------------------------------
A, B, C = 'ab.', 'abcd.', 'abcdef.'
D = 'ab cd. ef ghi. jk lmno.'                                                   # 3 parts at max_text_length=9 and -2
E, F, G = '...', 'abcdefgh.', 'abcdefghij.'
# dict inputs, a text that cleans to nothing, a text in 3 parts and a repeat (5 inputs behind its first occurrence: far
# enough that the overlapped producer finds it cached whatever the threads do)
INPUTS = [A, {'text': B}, {'content': C}, D, E, A, F, G]
MODES = {'sequential': {}, 'overlap': {'overlap': True}, 'backlog2': {'batch_backlog': 2}, 'backlog3': {'batch_backlog': 3},
         'backlog8': {'batch_backlog': 8}, 'backlog8_packed': {'batch_backlog': 8, 'pack_vocoder': True}}


def _n_tok(text):
    from text_to_speech_amd.tacotron2 import Tacotron2
    m = Tacotron2(None)
    return len(m.encode_text(m.clean_text(text), cleaned=True))


class _Warnings(logging.Handler):
    """Counts the warnings of the wrapper: one per row that is still outside the frame / token window after `max_trial`."""

    def __init__(self):
        super().__init__(logging.WARNING)
        self.count = 0

    def emit(self, record):
        self.count += 1


def run(inputs, *, method='predict', model=None, frames=None, postnet=False, as_queue=False, recorders=True,
        own_predicted=None, keep=None, **kwargs):
    """One scenario: `model.predict(inputs, ...)` (or `stream`) over fresh fakes -> its record (`keep`: only these fields)."""
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    synth, voc, events = FakeSynth(frames, postnet), FakeVocoder(), []
    model = Tacotron2(synth) if model is None else model(synth)
    if as_queue:
        q = queue.Queue()
        for item in list(inputs) + [None]:
            q.put(item)
        inputs = q
    kwargs.setdefault('max_length', 3.)
    if kwargs.pop('no_vocoder', False):
        vocoder = {}
    else:
        vocoder = {'vocoder': WaveGlow(voc)}
    if recorders:
        kwargs['callbacks'] = _recorders(events)
    if own_predicted is not None:
        kwargs['predicted'] = own_predicted
    else:
        kwargs.setdefault('save', False)
    random.seed(0)
    warnings = _Warnings()
    logging.getLogger('text_to_speech_amd.tacotron2').addHandler(warnings)
    try:
        res = getattr(model, method)(inputs, **vocoder, **kwargs)
    finally:
        logging.getLogger('text_to_speech_amd.tacotron2').removeHandler(warnings)
    predicted = kwargs.get('predicted')
    rec = {'synth_calls': synth.calls, 'vocoder_calls': voc.calls, 'events': events, 'gave_up': warnings.count,
           'postnet_calls': synth.engine.calls if postnet else None,
           'results': [_result(r) for r in res],
           'predicted': None if predicted is None else {k: ' '.join(sorted(v)) for k, v in predicted.items()}}
    return rec if keep is None else {k: rec[k] for k in keep}


def _sv2tts(**model_kw):
    from text_to_speech_amd.tacotron2 import SV2TTSTacotron2
    pool = np.asarray([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 13]], np.float32)
    return lambda synth: SV2TTSTacotron2(synth, lang='en', embeddings=pool, embedding_dim=4, **model_kw)


SAME = 'the same as from the list'


def _or_same(record, of_the_list):
    """The record of a run from a pre-filled queue, or SAME where it equals that of the run from the list."""
    return SAME if record == of_the_list else record


REPEAT = [A, {'text': B}, C, F, A]                                               # (the repeat 4 inputs behind: see INPUTS)
CALLS = ('synth_calls', 'vocoder_calls')


def predict_scenarios():
    out = {}
    # every mode, with and without per-sentence streams, from a list and from a queue
    # (full records for one mode per scheduler with streams on; the calls, and with streams on the events, of the others)
    for name, mode in MODES.items():
        for streams in (False, True):
            full = streams and name in ('sequential', 'overlap', 'backlog3')
            keep = None if full else CALLS + ('events',) if streams else CALLS
            kw = dict(mode, max_text_length=9, seed=5, sentence_streams=streams, keep=keep)
            key = f'modes/{name}/streams={int(streams)}'
            out[key] = run(INPUTS, **kw)
            out[key + '/queue'] = _or_same(run(INPUTS, as_queue=True, **kw), out[key])
    out['modes/overlap/no_vocoder'] = run(INPUTS[:3], no_vocoder=True, overlap=True)        # falls back to the sequential loop
    out['split/sentences'] = run([D, A], max_text_length=-2)
    out['split/sentences/backlog'] = run([D, A], max_text_length=-2, batch_backlog=2)
    for name, mode in (('sequential', {}), ('overlap', {'overlap': True}), ('backlog3', {'batch_backlog': 3}),
                       ('backlog8_packed', {'batch_backlog': 8, 'pack_vocoder': True})):
        for streams in (False, True):
            kw = dict(mode, method='stream', max_text_length=9, sentence_streams=streams,
                      keep=CALLS + ('events', 'results') if streams else CALLS)
            key = f'stream/{name}/streams={int(streams)}'
            out[key] = run(INPUTS, **kw)
            out[key + '/queue'] = _or_same(run(INPUTS, as_queue=True, **kw), out[key])
    # decoder behaviour
    texts = [A, B, C]
    dec = dict(keep=CALLS + ('postnet_calls', 'results', 'gave_up'))
    n_b = _n_tok(B)
    fail_once = lambda n, attempt, row: n if (n == n_b and attempt == 0) else 10 ** 6
    never_passes = lambda n, attempt, row: n if n == n_b else 10 ** 6
    for name, mode in (('sequential', {}), ('overlap', {'overlap': True}), ('backlog3', {'batch_backlog': 3})):
        out[f'decode/pass/{name}'] = run(texts, **dec, **mode)
        out[f'decode/cut/{name}'] = run(texts, frames='never', postnet=True, **dec, **mode)
        for streams in (False, True):
            tag = f'{name}/streams={int(streams)}'
            retry = dec if not streams else dict(keep=CALLS + ('gave_up',))     # (the results are those without streams)
            out[f'decode/fail_once/{tag}'] = run(texts, frames=fail_once, sentence_streams=streams, **retry, **mode)
            out[f'decode/never_passes/{tag}'] = run(texts, frames=never_passes, max_trial=2, sentence_streams=streams,
                                                   **retry, **mode)
        if name == 'backlog3':
            out[f'decode/cut_no_postnet/{name}'] = run(texts, frames='never', **dec, **mode)
        out[f'decode/max_length_int/{name}'] = run(texts, max_length=40, **dec, **mode)
        out[f'decode/vocoder_config/{name}'] = run([A, E], vocoder_config={'sigma': 0.5}, silence_time=0.25,
                                                   deterministic=True, **dec, **mode)
        if name == 'overlap':
            continue
        out[f'decode/max_length_none/{name}'] = run([A, B], max_length=None, frames=lambda n, attempt, row: 4 * n, **dec,
                                                    **mode)
        out[f'decode/no_vocoder/{name}'] = run(texts, no_vocoder=True, **dec, **mode)
    # cache
    for name, mode in (('sequential', {}), ('overlap', {'overlap': True}), ('backlog3', {'batch_backlog': 3})):
        held = lambda: {B: {'text': B, 'audio': 'kept.wav'}}
        out[f'cache/prefilled/{name}'] = run(REPEAT, own_predicted=held(), **mode)
        out[f'cache/prefilled/{name}/streams=1'] = run(REPEAT, own_predicted=held(), sentence_streams=True, keep=CALLS, **mode)
        out[f'cache/overwrite/{name}'] = run(REPEAT[:3], own_predicted=held(), overwrite=True, **mode)
        out[f'cache/built/{name}'] = run(REPEAT, keep=('events',), **mode)              # predict builds the map: joins
        out[f'cache/no_callbacks/{name}'] = run([A, B, A], recorders=False, **mode)     # nothing fills the map: A is redone
        for ro in (False, True):
            for rr in (False, True) if name != 'overlap' else ():
                out[f'returns/{name}/output={ro}/results={rr}'] = run(REPEAT, own_predicted=held(), return_output=ro,
                                                                      return_results=rr, keep=('events', 'results', 'predicted'),
                                                                      **mode)
    # speaker embeddings: per sentence on the sequential path, once per call on the others
    vector = np.asarray([0.5, 0.25, 2, 8], np.float32)
    # (the embedding never reaches the vocoder or the results: the synthesizer calls say it all)
    spk = dict(model=_sv2tts(), max_text_length=9, keep=('synth_calls',))
    selectors = {'omitted': {}, 'none': {'embeddings': None}, 'row0': {'embeddings': 0}, 'row2': {'embeddings': 2},
                 'mean': {'embeddings': 'mean'}, 'random': {'embeddings': 'random'}, 'dict': {'embeddings': {'mode': 1}},
                 'vector': {'embeddings': vector}}
    for name, mode in (('sequential', {}), ('overlap', {'overlap': True}), ('backlog3', {'batch_backlog': 3})):
        for sel, kw in selectors.items():
            out[f'sv2tts/{name}/{sel}'] = run([A, B, D, C], **spk, **mode, **kw)
        out[f'sv2tts/{name}/none_label'] = run([A, B], **{**spk, 'model': _sv2tts(use_label_embedding=True)}, embeddings=None,
                                               **mode)
        out[f'sv2tts/{name}/cached_random'] = run([A, B, D, C], embeddings='random', **spk, **mode,
                                                  own_predicted={B: {'text': B, 'audio': 'kept.wav'}})
    out['sv2tts/stream/random'] = run([A, B, C], method='stream', embeddings='random', **spk)
    return out


def refusals():
    """The messages of the refused calls."""
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    model, voc = Tacotron2(FakeSynth()), WaveGlow(FakeVocoder())
    out = {}
    for name, kw in (('pack_without_backlog', {'pack_vocoder': True}), ('pack_backlog1', {'pack_vocoder': True, 'batch_backlog': 1}),
                     ('backlog0', {'batch_backlog': 0}), ('backlog_overlap', {'batch_backlog': 2, 'overlap': True})):
        try:
            model.predict([A, B], vocoder=voc, save=False, **kw)
            out[name] = None
        except ValueError as exc:
            out[name] = str(exc)
    try:
        m = _sv2tts()(FakeSynth())
        m.embeddings = None
        m.infer(A)
    except ValueError as exc:
        out['no_embeddings'] = str(exc)
    return out


# ---- HipRuntime over a fake engine ------------------------------------------------------------------------------------------
class _Handle:
    def __init__(self, log):
        self.log = log

    def close(self):
        self.log.append(['close'])


class PlainEngine:
    """An engine without the split entry points."""

    def __init__(self):
        self.log = []

    def tacotron2_infer(self, tokens, **kw):
        self.log.append(['tacotron2_infer', _plain(np.asarray(tokens)), _plain(kw)])
        return 'out'

    def tacotron2_forward(self, tokens, mel_input, mel_lengths, **kw):
        self.log.append(['tacotron2_forward', type(tokens).__name__, _plain(np.asarray(mel_input)), _plain(mel_lengths), _plain(kw)])
        return 'out'

    def waveglow_infer(self, mel, **kw):
        self.log.append(['waveglow_infer', _plain(np.asarray(mel)), _plain(kw)])
        return np.zeros((mel.shape[0], mel.shape[1] * 256), np.float32)


class SplitEngine(PlainEngine):
    """An engine with `tacotron2_encode` / `tacotron2_decode`; a decode with max_len == 13 raises."""

    def tacotron2_encode(self, tokens, speaker=None, into=None):
        self.log.append(['tacotron2_encode', _plain(np.asarray(tokens)), _plain(speaker), into is not None])
        return into if into is not None else _Handle(self.log)

    def tacotron2_decode(self, encoded, **kw):
        self.log.append(['tacotron2_decode', type(encoded).__name__, _plain(kw)])
        if kw['max_len'] == 13:
            raise RuntimeError('decode failed')
        return 'out'


def runtime_scenarios():
    from text_to_speech_amd.runtime import HipRuntime
    out = {}
    tok = np.zeros((2, 6), np.int32)
    tok[0, :6], tok[1, :4] = 7, 9
    other = tok + (tok != 0)
    spk = np.asarray([[1, 2], [3, 4]], np.float32)
    mel_in = np.zeros((2, 5, 80), np.float32)
    mel = np.ones((2, 3, 80), np.float32)
    masks = np.full((2, 8, 2, 256), 2, np.float32)
    z = np.ones((2, 96, 8), np.float32)
    taco_calls = [
        ('none', (tok,), {}), ('float', (tok,), {'max_length': 2.5}), ('int', (tok,), {'max_length': 8}),
        ('zero', (tok,), {'max_length': 0}), ('one_row', (tok[0],), {'max_length': 3.}),
        ('speaker', ((tok, spk),), {'max_length': 8}), ('tuple_of_one', ((tok,),), {'max_length': 8}),
        ('seed', (tok,), {'max_length': 8, 'seed': 5}), ('streams', (tok,), {'max_length': 8, 'streams': [(4, 1, 2), 9]}),
        ('streams_seed', (tok,), {'max_length': 8, 'streams': [(4, 1, 2), (9, 0, 0)], 'seed': 5}),
        ('deterministic', (tok,), {'max_length': 8, 'deterministic': True}),
        ('masks', (tok,), {'max_length': 8, 'prenet_masks': masks}),
        ('window', (tok,), {'max_length': 8, 'attn_mask_win_len': 12, 'attn_mask_offset': 0.5, 'early_stopping': 0,
                            'precision': 'f16', 'unknown': 1}),
        ('again', (tok,), {'max_length': 8}), ('other', (other,), {'max_length': 8}),
        ('raises', (tok,), {'max_length': 13}), ('after_raise', (tok,), {'max_length': 8}),
        ('streams_deterministic', (tok,), {'max_length': 8, 'streams': [1, 2], 'deterministic': True}),
        ('streams_masks', (tok,), {'max_length': 8, 'streams': [1, 2], 'prenet_masks': masks}),
        ('streams_short', (tok,), {'max_length': 8, 'streams': [1]}),
    ]
    forward_calls = [
        ('default', (tok, mel_in, [5, 3]), {}), ('again', (tok, mel_in, [5, 3]), {}),
        ('one_utterance', (tok[0], mel_in[0]), {}), ('speaker', ((tok, spk), mel_in, [5, 3]), {}),
        ('seed', (tok, mel_in, [5, 3]), {'seed': 5}), ('deterministic', (tok, mel_in, [5, 3]), {'deterministic': True}),
        ('masks', (tok, mel_in, [5, 3]), {'prenet_masks': masks[:, :5], 'precision': 'f16'}),
        ('after', (other, mel_in, [5, 3]), {}),
    ]
    wg_calls = [
        ('default', (mel,), {}), ('again', (mel,), {'sigma': 0.5}), ('one_utterance', (mel[0],), {}),
        ('seed', (mel,), {'seed': 5}), ('deterministic', (mel,), {'deterministic': True}), ('z', (mel,), {'z': z}),
        ('lengths', (mel,), {'lengths': [3, 2]}), ('packed', (mel,), {'lengths': [3, 2], 'packed': True}),
        ('streams', (mel,), {'streams': [(4, 1), 9], 'lengths': [3, 2], 'packed': True}),
        ('streams_seed', (mel,), {'streams': [(4, 1), (9, 0)], 'seed': 5, 'precision': 'f16', 'unknown': 1}),
        ('after', (mel,), {}),
        ('packed_without_lengths', (mel,), {'packed': True}),
        ('streams_deterministic', (mel,), {'streams': [1, 2], 'deterministic': True}),
        ('streams_z', (mel,), {'streams': [1, 2], 'z': z}), ('streams_wide', (mel,), {'streams': [(0, 0, 0), 1]}),
    ]
    for ename, engine in (('plain', PlainEngine), ('split', SplitEngine)):
        for method, calls in (('tacotron2_infer', taco_calls), ('tacotron2_forward', forward_calls), ('waveglow_infer', wg_calls),
                              ('__call__', [('tokens', (tok,), {'max_length': 8}), ('mel', (mel,), {})])):
            if ename == 'split' and method in ('waveglow_infer', '__call__'):
                continue                                                       # (the vocoder path does not look at the engine)
            eng = engine()
            rt = HipRuntime('none', engine=eng, seed=77, model=None)
            steps = []
            for name, args, kw in calls:
                eng.log.clear()
                try:
                    getattr(rt, method)(*args, **kw)
                    raised = None
                except (ValueError, RuntimeError) as exc:
                    raised = f'{type(exc).__name__}: {exc}'
                # RUNTIME_STEP
                steps.append([name, list(eng.log), raised, rt._offset, rt.encoder_reuses, rt._encoded is not None])
            out[f'{ename}/{method}'] = steps
    return out


# ---- TTSPipeline over a fake engine -----------------------------------------------------------------------------------------
def pipeline_scenarios():
    """`synthesize_tokens` with the tensors kept on the host (`on_the_host`): the frame budget, the
    keys and offsets the engine gets, and the pipeline's running offset after every call."""
    import torch
    from text_to_speech_amd.pipeline import TTSPipeline

    class Out:
        pass

    class Engine:
        device = 0
        last_steps = 0

        def __init__(self):
            self.log = []

        def random_prenet_masks(self, B, max_len, seed, offset):
            self.log.append(['random_prenet_masks', B, max_len, seed, offset])
            return torch.zeros((B, max_len, 2, 256))

        def tacotron2_infer(self, tok, **kw):
            self.log.append(['tacotron2_infer', _plain(tok), _plain(kw)])
            n_tok = (tok != 0).sum(dim=1)
            out = Out()
            out.lengths = torch.minimum(n_tok * 2, torch.tensor(kw['max_len']))
            out.mel = torch.zeros((tok.shape[0], kw['max_len'], 80))
            self.last_steps = int(out.lengths.max())
            return out

        def waveglow_infer(self, mel, **kw):
            self.log.append(['waveglow_infer', _plain(mel), _plain(kw)])
            return torch.ones((mel.shape[0], mel.shape[1] * 256))

    tok = np.zeros((2, 6), np.int32)
    tok[0, :6], tok[1, :4] = 7, 9
    calls = [('float', {'max_length': 2.5}), ('int', {'max_length': 9}), ('zero', {'max_length': 0}), ('default', {}),
             ('deterministic', {'max_length': 9, 'deterministic': True}), ('ragged', {'max_length': 9, 'ragged': True}),
             ('row_ids', {'max_length': 9, 'row_ids': [11, 2], 'ragged': True}),
             ('masks_and_z', {'max_length': 9, 'prenet_masks': np.zeros((2, 9, 2, 256), np.float32),
                              'z': np.zeros((2, 9 * 32, 8), np.float32)}),
             ('on_device', {'max_length': 9, 'on_device': True, 'round_frames_to': 1}), ('after', {'max_length': 9}),
             ('trim_dict', {'trim_silence': {'method': 'rms'}}), ('trim_on_device', {'trim_silence': True, 'on_device': True}),
             ('row_ids_deterministic', {'row_ids': [1, 2], 'deterministic': True})]
    def on_the_host(pipe, **kw):
        """`synthesize_tokens` asks for torch.device('cuda', n) by that name (it imports torch when called, so there is no
        name of its own to patch): the name gives the host device for the length of this one call, in this thread."""
        real = torch.device
        torch.device = lambda *a, **k: real('cpu')
        try:
            return pipe.synthesize_tokens(tok, **kw)
        finally:
            torch.device = real

    out = {}
    for rank in (0, 3):
        eng = Engine()
        pipe = TTSPipeline(eng, seed=9, rank=rank)
        steps = []
        for name, kw in calls if rank == 0 else [c for c in calls if c[0] in ('float', 'row_ids', 'after')]:
            eng.log.clear()
            try:
                audio, lengths, n_steps = on_the_host(pipe, **kw)
                got = {'audio': [_plain(a) for a in audio], 'lengths': _plain(lengths), 'steps': n_steps}
            except ValueError as exc:
                got = f'ValueError: {exc}'
            steps.append({'call': name, 'engine': list(eng.log), 'returned': got, 'offset': pipe._offset})
        out[f'rank{rank}'] = steps
    return out


def frame_cap_values():
    """The frame budget of a token count under float, int and absent `max_length`, as the three call sites compute it through
    their public entry: read back from the `HipRuntime` scenarios' `max_len` -- here only the float32 product's corner cases."""
    from text_to_speech_amd.runtime import HipRuntime
    eng = PlainEngine()
    rt = HipRuntime('none', engine=eng, seed=1)
    out = []
    for n_tok in (1, 3, 7, 33, 100, 255):
        for max_length in (0.1, 0.3, 1.1, 3., 4.7, 10.):
            rt.tacotron2_infer(np.ones((1, n_tok), np.int32), max_length=max_length, deterministic=True)
            out.append([n_tok, max_length, eng.log[-1][2]['max_len']])
    return out


def trace():
    return {'predict': predict_scenarios(), 'refusals': refusals(), 'runtime': runtime_scenarios(),
            'pipeline': pipeline_scenarios(), 'frame_cap': frame_cap_values()}


def check_paths(t):
    """Every scenario takes the path it names."""
    p = t['predict']
    n_b = _n_tok(B)
    for key, rec in p.items():
        if rec == SAME:
            continue
        rows = lambda r: [sum(1 for v in row if v) for c in r['synth_calls'] for row in c[0]]
        if key.startswith('decode/fail_once/'):
            assert rows(rec).count(n_b) == 2, key                              # the failing row was decoded twice, the others once
            assert sorted(rows(rec)) == sorted(rows(p['decode/pass/' + key.split('/')[2]]) + [n_b]), key
        if key.startswith('decode/never_passes/'):
            assert rows(rec).count(n_b) == 2, key                              # max_trial=2
            assert rec['gave_up'] == 1, key                                    # ... and the warning came once, for that row
        elif key.startswith('decode/') and 'max_length_int' not in key:
            assert rec['gave_up'] == 0, key
        if key.startswith('decode/cut/backlog'):
            assert rec['postnet_calls'], key
        if key.startswith('decode/cut/sequential') or key.startswith('decode/cut/overlap'):
            assert rec['postnet_calls'] == [], key                             # a lone row is never cut
        if key.startswith('cache/prefilled/'):
            assert n_b not in rows(rec), key                                   # the cached text reached no synthesizer call
        if key.startswith('cache/prefilled/'):
            assert rows(rec).count(_n_tok(A)) == 1, key                        # the repeat was served from the cache
        if key.startswith('cache/overwrite/'):
            assert n_b in rows(rec), key
        if key.startswith('modes/backlog'):
            assert max(len(c[0]) for c in rec['synth_calls']) > 1, key
            assert any(c[1] is not None for c in rec['vocoder_calls']), key
        if key.startswith('modes/backlog8_packed'):
            assert any(c[2].get('packed') for c in rec['vocoder_calls']), key
        if key.startswith('modes/') and 'results' in rec and 'no_vocoder' not in key:
            assert any(len(r[2]) == 3 for r in rec['results']), key            # the text in 3 parts
            assert any(r[3] == 0.15 for r in rec['results']), key              # the silence result
    spk = lambda key: [c[3] for c in p[key]['synth_calls']]
    first = lambda s: s[0] if isinstance(s[0], list) else s
    assert len({tuple(first(s)) for s in spk('sv2tts/sequential/random')}) > 1     # per sentence
    for name in ('overlap', 'backlog3'):
        assert len({tuple(first(s)) for s in spk(f'sv2tts/{name}/random')}) == 1   # once per call
    assert all(v is not None for v in t['refusals'].values())
    split = {s[0]: s for s in t['runtime']['split/tacotron2_infer']}
    assert split['raises'][2] and not split['raises'][5]                       # the failed decode dropped the encoded batch
    assert any(e[0] == 'tacotron2_encode' for e in split['after_raise'][1])    # ... and the next call encoded again
    assert split['again'][4] > split['none'][4]


def dump(t, f):
    """The trace as JSON with one scenario (or runtime method, or pipeline rank) per line."""
    import json
    one = lambda v: json.dumps(v, separators=(',', ':'), sort_keys=True)
    sections = []
    for name, section in t.items():
        if isinstance(section, dict):
            body = ',\n'.join(f'{json.dumps(k)}:{one(v)}' for k, v in section.items())
            sections.append(f'{json.dumps(name)}:{{\n{body}\n}}')
        else:
            sections.append(f'{json.dumps(name)}:{one(section)}')
    f.write('{\n' + ',\n'.join(sections) + '\n}\n')
