"""CPU: what the packed WaveGlow call stands on -- the gap length (numpy oracle), the packing plan, the argument errors that
come before any GPU call, and `predict(batch_backlog=k, pack_vocoder=True)` on fake models."""
import numpy as np
import pytest

from conftest import rms
from waveglow_packed_ref import header_gap_frames, infer_packed, packing_plan

WAVE_RMS_TOL = 1e-4                                   # the project's fp32 waveform tolerance


def test_four_gap_frames_isolate_the_segments_and_three_do_not(wg_weights, wg_cfg):
    """Segments of 6, 1 and 5 frames in one row, junk on the gap frames, against the oracle's run of each segment alone.
    One WN layer reaches 2^7 positions = 4 frames and the masked residual stream stops anything from travelling further, so
    TTS_HIP_WG_GAP_FRAMES = 4 gives the solo audio up to BLAS blocking (measured 2.6e-7 .. 2.7e-7 RMS on signals of RMS
    1.03 .. 1.06; bound 1e-6: a factor 4 for another CPU's blocking, four orders of magnitude below the first failure) and
    one frame less does not (measured 1.2e-2, 5.5e-2, 1.8e-2; bound: worse than 100 x the 1e-4 waveform tolerance)."""
    from oracle import waveglow_ref
    gap = header_gap_frames()
    assert gap == 4
    lens = (6, 1, 5)
    rng = np.random.default_rng(7)
    mels = [rng.uniform(-11.5, 1.2, (n, 80)).astype(np.float32) for n in lens]
    zs = [rng.standard_normal((n * 32, 8)).astype(np.float32) for n in lens]
    solo = [waveglow_ref.infer(m[None], wg_weights, wg_cfg, z=z[None])[0] for m, z in zip(mels, zs)]
    errs = {}
    for g in (gap, gap - 1):
        plan = packing_plan(lens, max(lens), g)
        F = plan['F']
        assert F == sum(lens) + g * (len(lens) - 1)
        mel = np.full((1, F, 80), 55.0, np.float32)                      # gap contents must not matter
        z = np.full((1, F * 32, 8), 9.0, np.float32)
        mel[0, plan['gaps'][:1]] = np.nan
        for s, m, zz in zip(plan['starts'], mels, zs):
            mel[0, s:s + len(m)] = m
            z[0, s * 32:(s + len(m)) * 32] = zz
        out = infer_packed(mel, z, plan['flags'], wg_weights, wg_cfg)
        assert np.isfinite(out).all()
        assert not out[np.repeat(np.asarray(plan['flags']) == 0, 256)].any()
        errs[g] = [rms(out[s * 256:(s + n) * 256] - ref) for s, n, ref in zip(plan['starts'], lens, solo)]
        print(f'gap {g}: F = {F}, rms of each segment against its solo oracle run', ['%.2e' % e for e in errs[g]],
              'signal rms', ['%.3f' % rms(s) for s in solo])
    assert max(errs[gap]) <= 1e-6
    assert min(errs[gap - 1]) > 100 * WAVE_RMS_TOL


def test_packing_plan():
    gap = header_gap_frames()
    # zeros take no space and no gap, wherever they stand
    p = packing_plan((0, 3, 0, 0, 2, 0), 5, gap)
    assert p['F'] == 3 + gap + 2 and p['starts'] == [0, 0, 0, 0, 3 + gap, 0]
    assert p['gaps'] == list(range(3, 3 + gap))
    assert p['flags'] == [1 + 5 + 0, 1 + 5 + 1, 1 + 5 + 2] + [0] * gap + [1 + 20 + 0, 1 + 20 + 1]
    # a single row: the row itself; one frame; nothing at all
    p = packing_plan((7,), 9, gap)
    assert p == {'starts': [0], 'F': 7, 'flags': list(range(1, 8)), 'gaps': []}
    assert packing_plan((1,), 1, gap) == {'starts': [0], 'F': 1, 'flags': [1], 'gaps': []}
    assert packing_plan((0, 0), 4, gap) == {'starts': [0, 0], 'F': 0, 'flags': [], 'gaps': []}
    # all rows full: B * T frames and B - 1 gaps; the flags name every frame of the batch once, in order
    B, T = 3, 4
    p = packing_plan((T,) * B, T, gap)
    assert p['F'] == B * T + gap * (B - 1) and p['starts'] == [b * (T + gap) for b in range(B)]
    assert [f for f in p['flags'] if f] == list(range(1, B * T + 1))
    assert all(p['flags'][g] == 0 for g in p['gaps']) and len(p['gaps']) == gap * (B - 1)
    # the full-size shape of DESIGN.md section 4.2
    p = packing_plan((800, 523, 77, 1, 640, 799, 300, 0), 800, gap)
    assert p['F'] == 3140 + 6 * gap == 3164


class _NoGpu:
    """Stands in for a HipEngine: any call is a failure (argument errors must come first)."""
    def __getattr__(self, name):
        raise AssertionError(f'engine.{name} called')


def test_argument_errors_come_before_any_gpu_call():
    from text_to_speech_amd.engine import HipEngine
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2, stream, tts
    from text_to_speech_amd.waveglow import WaveGlow
    eng = HipEngine.__new__(HipEngine)                                   # no handle, no library
    mel = np.zeros((2, 4, 80), np.float32)
    with pytest.raises(ValueError, match='packed=True needs lengths'):
        eng.waveglow_infer(mel, packed=True)
    rt = HipRuntime.__new__(HipRuntime)
    rt.engine = _NoGpu()
    with pytest.raises(ValueError, match='packed=True needs lengths'):
        rt.waveglow_infer(mel, packed=True)
    with pytest.raises(ValueError, match='packed=True needs lengths'):
        WaveGlow(rt.waveglow_infer)(mel, packed=True)
    model, voc = Tacotron2(_NoGpu()), WaveGlow(_NoGpu())
    for kw in ({}, {'batch_backlog': 1}, {'batch_backlog': None}):
        with pytest.raises(ValueError, match='pack_vocoder'):
            model.predict(['a.', 'b.'], vocoder=voc, save=False, pack_vocoder=True, **kw)
        with pytest.raises(ValueError, match='pack_vocoder'):
            tts(['a.', 'b.'], model=model, vocoder=voc, save=False, pack_vocoder=True, **kw)
    with pytest.raises(ValueError, match='pack_vocoder'):
        model.predict(['a.', 'b.'], vocoder=voc, save=False, pack_vocoder=True, overlap=True)


def test_c_abi_declares_the_packed_calls():
    from text_to_speech_amd import _lib
    assert _lib.SIGNATURES['tts_hip_waveglow_infer_packed'] == _lib.SIGNATURES['tts_hip_waveglow_infer_ragged']
    assert _lib.SIGNATURES['tts_hip_waveglow_infer_packed_async'] == _lib.SIGNATURES['tts_hip_waveglow_infer_ragged_async']
    lib = _lib.load_library()
    assert lib.tts_hip_abi_version() == 13
    for name in ('tts_hip_waveglow_infer_packed', 'tts_hip_waveglow_infer_packed_async'):
        assert hasattr(lib, name)
    assert lib.tts_hip_waveglow_infer_packed(None, None, 1, 1, None, None, 1.0, None, 0, 0) == -1       # TTS_HIP_EINVAL
    assert lib.tts_hip_waveglow_infer_packed_async(None, None, 1, 1, None, None, 1.0, None, 0, None) == -1


def test_predict_pack_vocoder_on_fake_models():
    """`predict(batch_backlog=4, pack_vocoder=True)`: one vocoder call per group with `lengths` and `packed=True`; results
    and callbacks in input order, identical to the run without `pack_vocoder` (whose calls carry no `packed`)."""
    from test_stream_backlog import BatchSynth, RaggedVocoder, _texts
    from text_to_speech_amd.tacotron2 import Tacotron2, stream
    from text_to_speech_amd.waveglow import WaveGlow

    class Recording(RaggedVocoder):
        def __init__(self):
            super().__init__()
            self.kwargs = []

        def __call__(self, mel, lengths=None, **kwargs):
            self.kwargs.append(dict(kwargs, lengths=lengths))
            return super().__call__(mel, lengths=lengths, **{k: v for k, v in kwargs.items() if k != 'packed'})

    def run(texts, **kw):
        synth, fake = BatchSynth(), Recording()
        rec = []
        res = Tacotron2(synth).predict(texts, vocoder=WaveGlow(fake), save=False, max_length=3., callbacks=[
            lambda text, audio=None, **_: rec.append((text, np.asarray(audio).copy()))], **kw)
        return res, rec, synth, fake

    texts = _texts(10)
    res, rec, synth, fake = run(texts, batch_backlog=4, pack_vocoder=True)
    plain_res, plain_rec, plain_synth, plain_fake = run(texts, batch_backlog=4)
    assert [t for t, _ in rec] == [t for t, _ in plain_rec] == texts
    assert [r['text'] for r in res] == [r['text'] for r in plain_res] == texts
    for (_, a), (_, b), r, s in zip(rec, plain_rec, res, plain_res):
        assert np.array_equal(a, b) and np.array_equal(r['audio'], s['audio'])
        assert len(r['mel']) == len(s['mel']) == 1 and np.array_equal(r['mel'][0], s['mel'][0])
    assert [c[0] for c in fake.calls] == [c[0] for c in plain_fake.calls] == [4, 4, 2]                 # one call per group
    assert [len(c[0]) for c in synth.calls] == [4, 4, 2]
    assert all(k.get('packed') is True and k['lengths'] is not None for k in fake.kwargs)
    assert all('packed' not in k and k['lengths'] is not None for k in plain_fake.kwargs)
    assert [c[2] for c in fake.calls] == [c[2] for c in plain_fake.calls]
    # stream() hands the argument on (its warm-up sentences run alone, without it)
    synth, fake = BatchSynth(), Recording()
    got = []
    stream(iter(texts[:4]), model=Tacotron2(synth), vocoder=WaveGlow(fake), save=False, max_length=3., batch_backlog=4,
           pack_vocoder=True, callbacks=[lambda text, **_: got.append(text)])
    assert got[-4:] == texts[:4]
    assert [k.get('packed') for k in fake.kwargs] == [None, None, True]
