"""GPU: cepstral envelope matching (csrc/stft_inv.hip: tts_hip_formant_match) against the float64 restatement of
tests/formant_ref.py, stage by stage (`HipEngine.formant_match_probe`) on every case of tests/formant_cases.py, on ragged batches
with a warp per row, on the host, device and stream routes, through `effects.pitch_shift(preserve_formants=True)`,
`effects.formant_shift` and the sentence pipeline's `preserve_formants` / `formant_steps`, and on the synthetic vowel of
tests/test_formant.py; bounds from tests/formant_cases.py."""
import ctypes

import numpy as np
import pytest

import formant_cases as C
import formant_ref as Fm
from test_formant import F0_TOL, F2_HZ, G, vowel_check, vowel_report

pytestmark = pytest.mark.gpu

PROBED = ('logmag', 'envelope', 'gain', 'operand', 'frames')


def _plan(eng, g):
    from text_to_speech_amd.stft import STFT
    return STFT(filter_length=g.fl, hop_length=g.hop, win_length=g.wl, engine=eng)._plan()


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize('name', C.NAMES)
def test_stage_by_stage(gpu_engine, name):
    """Every probe stage against float64 applied to the run's own previous stage (the log-magnitudes against `mel_fn_probe`'s
    spectra of the two signals), within the bounds of the case's plan; zeros in the frames behind a row's own.  No case is left
    out of any comparison."""
    case = C.BY_NAME[name]
    g, (x, s) = case.geom, C.inputs_of(name)
    plan = _plan(gpu_engine, g)
    B, N, F = case.B, case.N, g.frames(case.N)
    kw = dict(warp=list(case.warps), lifter=case.Q, max_gain_db=case.max_gain_db, lengths=list(case.lengths))
    kept = {what: gpu_engine.formant_match_probe(plan, x, s, what, **kw) for what in PROBED}
    kept['audio'] = gpu_engine.formant_match(plan, x, s, **kw)
    kept['spectrum'] = np.stack([gpu_engine.mel_fn_probe(plan, a, 'spectrum', lengths=list(case.lengths)) for a in (x if s is None else s, x)])
    assert kept['logmag'].shape == kept['envelope'].shape == (2, B, F, g.cut) and kept['gain'].shape == (B, F, g.cut)
    assert kept['operand'].shape == (B, F, 2 * g.cut) and kept['frames'].shape == (B, F, g.fl) and kept['audio'].shape == (B, N)
    assert all(np.isfinite(a).all() for a in kept.values())
    errs = C.stage_errors(name, kept.__getitem__)
    print(name, ' '.join(f'{st} {e:.3e}' for st, e in errs.items()))
    for st, bound in C.BOUNDS[case.group].items():
        assert errs[st] <= bound, (st, errs[st], bound)
    if case.audio == 'zeros':
        assert not kept['operand'].any() and not kept['frames'].any() and not kept['audio'].any()
    if s is None:                                               # one transform: both halves are the audio's
        assert _bits(kept['logmag'][0], kept['logmag'][1]) and _bits(kept['envelope'][0], kept['envelope'][1])


@pytest.mark.parametrize('group', sorted(C.GEOMS))
def test_source_null_is_source_equal_to_audio(gpu_engine, group):
    """The same bits at every stage; with warp = 1 the gain is exactly 1 and the operand is the spectrum bit for bit."""
    g = C.GEOMS[group]
    plan = _plan(gpu_engine, g)
    N = C.max_len(g)
    lengths = [N, g.wl - 3, N - g.hop - 1]
    x = np.stack([C.TC.signal(kind, N, g, seed=b) for b, kind in enumerate(('noisy', 'gaps', 'full'))])
    for b, L in enumerate(lengths):
        x[b, L:] = 0
    for warp in ([0.8, 2.0, 1.37], 1.0):
        kw = dict(warp=warp, lengths=lengths)
        for what in PROBED:
            assert _bits(gpu_engine.formant_match_probe(plan, x, None, what, **kw), gpu_engine.formant_match_probe(plan, x, x, what, **kw)), what
        assert _bits(gpu_engine.formant_match(plan, x, None, **kw), gpu_engine.formant_match(plan, x, x.copy(), **kw))
    spec = gpu_engine.mel_fn_probe(plan, x, 'spectrum', lengths=lengths)
    gain = gpu_engine.formant_match_probe(plan, x, None, 'gain', lengths=lengths)
    op = gpu_engine.formant_match_probe(plan, x, None, 'operand', lengths=lengths)
    for b, L in enumerate(lengths):
        Fb = g.frames(L)
        assert (gain[b, :Fb] == 1).all() and (gain[b, Fb:] == 0).all()
        assert _bits(op[b, :Fb], spec[b, :Fb]) and (op[b, Fb:] == 0).all()
    # ... and the call is then the plan's inverse of that spectrum: what stft_inverse gives for the row's frames
    back = gpu_engine.stft_inverse(plan, spec[..., :g.cut], spec[..., g.cut:], frames=[g.frames(L) for L in lengths], polar=False)
    got = gpu_engine.formant_match(plan, x, lengths=lengths)
    for b, L in enumerate(lengths):
        keep = min(L, g.samples(g.frames(L)))
        assert _bits(got[b, :keep], back[b, :keep]) and (got[b, keep:] == 0).all()


@pytest.mark.parametrize('group', sorted(C.GEOMS))
def test_ragged_rows_with_a_warp_each(gpu_engine, group):
    """Six rows, a warp each (0.5, 1 and 2 among them), NaN behind every length in both signals: finite, every row bit-equal to
    the row called alone (test_stage_by_stage holds such rows to the restatement), zero beyond its length; a repeat gives the
    same bits; host = device = stream."""
    import torch
    g = C.GEOMS[group]
    plan = _plan(gpu_engine, g)
    N = C.max_len(g)
    lengths = [N, g.hop, N - g.hop // 2 - 1, 2 * g.fl, N // 2, g.fl + 1]
    warps = [0.5, 1.0, 2.0, 1.37, 0.8, 1.0]
    x = np.stack([C.TC.signal('noisy', N, g, seed=b) for b in range(6)])
    s = np.stack([C.TC.signal('tone' if b % 2 else 'full', N, g, seed=10 + b) for b in range(6)])
    for b, L in enumerate(lengths):
        x[b, L:] = np.nan
        s[b, L:] = np.nan
    kw = dict(warp=warps, lengths=lengths, lifter=min(9, g.fl // 2 - 1), max_gain_db=12.0)
    got = gpu_engine.formant_match(plan, x, s, **kw)
    assert got.shape == (6, N) and np.isfinite(got).all()
    assert _bits(gpu_engine.formant_match(plan, x, s, **kw), got)
    for what in PROBED:
        stage = gpu_engine.formant_match_probe(plan, x, s, what, **kw)
        assert np.isfinite(stage).all(), what
    for b, (L, w) in enumerate(zip(lengths, warps)):
        alone = gpu_engine.formant_match(plan, x[b, :L], s[b, :L], **dict(kw, warp=w, lengths=None))
        keep = min(L, g.samples(g.frames(L)))
        assert alone.shape == (1, L) and _bits(got[b, :L], alone[0]) and (got[b, keep:] == 0).all(), (b, L, w)
        assert np.abs(alone[0, :keep]).max() > 0
    xd, sd = torch.as_tensor(x).cuda(), torch.as_tensor(s).cuda()
    on_device = gpu_engine.formant_match(plan, xd, sd, **kw)
    assert on_device.is_cuda and _bits(on_device.cpu().numpy(), got)
    stream = torch.cuda.Stream()
    queued = gpu_engine.formant_match(plan, xd, sd, stream=stream, **kw)
    stream.synchronize()
    assert _bits(queued.cpu().numpy(), got)
    mixed = gpu_engine.formant_match(plan, xd, s, **kw)         # a host source next to a device audio is moved there
    assert mixed.is_cuda and _bits(mixed.cpu().numpy(), got)
    assert torch.equal(torch.nan_to_num(xd), torch.nan_to_num(torch.as_tensor(x).cuda()))


def _tones(n=12000):
    from test_time_stretch import two_tones
    return np.stack([two_tones(220.3).astype(np.float32)[:n], two_tones(1000.0).astype(np.float32)[:n]])


def test_pitch_shift_with_preserved_formants_is_its_three_parts(gpu_engine):
    """... and without them the result of the two parts it was before, bit for bit."""
    import torch
    from text_to_speech_amd import effects
    eng = gpu_engine
    x, lengths = _tones(), [12000, 9000]
    plan = effects.default_plan(eng)
    for n_steps, formant_steps in ((-3, 0.0), (7, 0.0), (4, -2.0)):
        r, p, q = effects.pitch_ratio(n_steps)
        stretched, n = eng.time_stretch(plan, x, r, lengths=lengths)
        shifted = effects.fix_length(eng.resample(stretched, p, q, lengths=n), 12000).copy()
        shifted[1, 9000:] = 0
        plain = effects.pitch_shift(x, n_steps, engine=eng, lengths=lengths)
        assert _bits(plain, shifted) and _bits(effects.pitch_shift(x, n_steps, engine=eng, lengths=lengths, preserve_formants=False), shifted)
        want = eng.formant_match(plan, shifted, x, warp=2.0 ** (formant_steps / 12), lengths=lengths)
        got = effects.pitch_shift(x, n_steps, engine=eng, lengths=lengths, preserve_formants=True, formant_steps=formant_steps)
        assert got.shape == x.shape and _bits(got, want) and not _bits(got, plain) and (got[1, 9000:] == 0).all()
        if formant_steps:                                       # formant_steps implies the matching
            assert _bits(effects.pitch_shift(x, n_steps, engine=eng, lengths=lengths, formant_steps=formant_steps), want)
        on_device = effects.pitch_shift(torch.as_tensor(x).cuda(), n_steps, engine=eng, lengths=lengths, preserve_formants=True,
                                        formant_steps=formant_steps)
        assert on_device.is_cuda and _bits(on_device.cpu().numpy(), want)
    row = effects.pitch_shift(x[0], 4, engine=eng, preserve_formants=True)
    assert row.shape == (12000,) and _bits(row, effects.pitch_shift(x[:1], 4, engine=eng, preserve_formants=True)[0])


def test_formant_shift(gpu_engine):
    import torch
    from text_to_speech_amd import effects
    from text_to_speech_amd.runtime import HipRuntime
    eng = gpu_engine
    x, lengths = _tones(), [12000, 9000]
    plan = effects.default_plan(eng)
    want = eng.formant_match(plan, x, None, warp=2.0 ** (3 / 12), lengths=lengths)
    got = effects.formant_shift(x, 3, engine=eng, lengths=lengths)
    assert got.shape == x.shape and _bits(got, want) and (got[1, 9000:] == 0).all()
    assert effects.formant_shift(x, 0, engine=eng) is x
    assert _bits(effects.pitch_shift(x, 0, engine=eng, lengths=lengths, formant_steps=3), want)
    on_device = effects.formant_shift(torch.as_tensor(x).cuda(), 3, engine=eng, lengths=lengths)
    assert on_device.is_cuda and _bits(on_device.cpu().numpy(), want)
    assert _bits(effects.formant_shift(x[0], -4, engine=eng, lifter=20, max_gain_db=12.0),
                 eng.formant_match(plan, x[0], warp=2.0 ** (-4 / 12), lifter=20, max_gain_db=12.0)[0])
    rt = HipRuntime('w', model='waveglow', engine=eng, seed=0)
    assert _bits(rt.formant_shift(x, 3, lengths=lengths), want)
    assert _bits(rt.pitch_shift(x[0], 4, preserve_formants=True), effects.pitch_shift(x[0], 4, engine=eng, preserve_formants=True))
    assert eng.default_lifter(plan) == 33
    for bad in (dict(warp=2.5), dict(warp=[1.0, 1.0, 1.0]), dict(lifter=0), dict(lifter=512), dict(max_gain_db=0.0), dict(max_gain_db=61.0)):
        with pytest.raises(ValueError, match='formant_match: '):
            eng.formant_match(plan, x, **bad)
    with pytest.raises(ValueError, match='source must have the shape of audio'):
        eng.formant_match(plan, x, x[:, :100])


@pytest.mark.parametrize('steps', Fm.VOWEL_STEPS)
def test_the_vowel_keeps_its_formants(gpu_engine, steps):
    """The CPU suite's criteria on the device's output."""
    from text_to_speech_amd import effects
    x = Fm.vowel().astype(np.float32)
    shifted = effects.pitch_shift(x, steps, engine=gpu_engine)
    corrected = effects.pitch_shift(x, steps, engine=gpu_engine, preserve_formants=True)
    vowel_check(vowel_report(shifted, corrected, steps, 'GPU '))


def test_formant_shift_alone_moves_the_peaks(gpu_engine):
    from text_to_speech_amd import effects
    x = Fm.vowel().astype(np.float32)
    up = 2 ** (3 / 12)
    z = effects.formant_shift(x, 3, engine=gpu_engine)
    k1, k2 = Fm.lowest_peak(x, G), Fm.nearest_peak(x, G, F2_HZ)
    got1, got2, f0 = Fm.lowest_peak(z, G), Fm.nearest_peak(z, G, F2_HZ * up), Fm.autocorr_f0(z)
    print(f'GPU +3 formant steps: peaks at bins {got1} / {got2} (want {k1 * up:.1f} / {k2 * up:.1f}), F0 {f0:.2f} Hz')
    assert abs(got1 - k1 * up) <= 3 and abs(got2 - k2 * up) <= 3 and abs(f0 - Fm.F0) <= F0_TOL


def test_refusals_through_the_real_symbols(gpu_engine):
    """The messages are the front end's (tests/test_formant.py), with the entry point's name in front."""
    eng, g = gpu_engine, C.GEOMS['small']
    plan = _plan(eng, g)
    lib, h = eng._lib, eng._h
    x = np.ones((2, 400), np.float32)
    out = np.full((2, 400), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    wide, bad_lengths = np.array([1.0, 2.5]), np.array([400, 0], np.int32)       # kept alive
    whisper = eng.mel_fn(dict(kind='whisper', sampling_rate=16000, n_mel_channels=80, filter_length=400, hop_length=160,
                              win_length=400, mel_fmin=0.0, mel_fmax=8000.0))
    emph = eng.mel_fn(dict(sampling_rate=22050, n_mel_channels=1, filter_length=64, hop_length=16, win_length=64, mel_fmin=0.0,
                           mel_fmax=11025.0, pre_emph=0.97))

    def call(audio=p(x), source=None, B=2, N=400, lengths=None, fn=plan.handle, warps=None, Q=9, db=24.0, res=p(out), mem=0):
        rc = lib.tts_hip_formant_match(h, audio, source, B, N, lengths, fn, warps, Q, db, res, mem)
        return rc, (lib.tts_hip_last_error(h) or b'').decode()

    table = [
        (dict(fn=ctypes.c_void_p(0x1234), audio=None), 'formant_match: not a plan of this handle'),
        (dict(audio=None), 'formant_match: bad argument'), (dict(res=None), 'formant_match: bad argument'),
        (dict(lengths=p(bad_lengths)), 'formant_match: lengths[1] = 0 outside [1, N = 400]'),
        (dict(fn=whisper.handle), 'formant_match: refused for a Whisper plan'),
        (dict(fn=emph.handle), 'formant_match: pre_emph = 0.97 > 0 cannot be inverted'),
        (dict(warps=p(wide)), 'formant_match: warps[1] = 2.5 must be finite and lie in [0.5, 2]'),
        (dict(Q=32), 'formant_match: lifter Q = 32 outside [1, filter_length / 2 - 1 = 31]'),
        (dict(db=0.0), 'formant_match: max_gain_db = 0 must be finite and lie in (0, 60]'),
        (dict(mem=2), 'formant_match: bad mem kind 2'),
    ]
    for kw, message in table:
        rc, msg = call(**kw)
        assert rc == -1 and msg == message, (kw, rc, msg)
    assert (out == 7.0).all()                                                # nothing was written
    for what, message in ((5, 'formant_match_probe: no stage 5 (0 .. 4)'), (-1, 'formant_match_probe: no stage -1 (0 .. 4)')):
        rc = lib.tts_hip_formant_match_probe(h, p(x), None, 2, 400, None, plan.handle, None, 9, 24.0, what, p(out), 0)
        assert rc == -1 and (lib.tts_hip_last_error(h) or b'').decode() == message
    rc = lib.tts_hip_formant_match_async(h, None, None, 2, 400, None, plan.handle, None, 9, 24.0, p(out), None)
    assert rc == -1 and (lib.tts_hip_last_error(h) or b'').decode() == 'formant_match_async: bad argument'
    # a good call on the same handle still succeeds: the row comes back where the window rebuilds it
    rc, msg = call()
    assert rc == 0, msg
    assert np.isfinite(out).all() and np.abs(out[:, 64:320] - 1.0).max() <= 1e-4


def test_the_sentence_pipeline_takes_preserve_formants_and_formant_steps(gpu_engine, monkeypatch):
    """tts(..., pitch_steps=, preserve_formants=True) and tts(..., formant_steps=) are `effects` applied to the plain result;
    with the defaults nothing new is called."""
    from text_to_speech_amd import effects
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2, tts
    from text_to_speech_amd.waveglow import WaveGlow
    model = Tacotron2(HipRuntime('t', model='tacotron2', engine=gpu_engine, seed=0))
    voc = WaveGlow(HipRuntime('w', model='waveglow', engine=gpu_engine, seed=0))
    kw = dict(model=model, vocoder=voc, max_length=6., max_text_length=-2, save=False, seed=5)
    text = 'Hello there. General test!'
    plain = tts(text, **kw)
    calls = []
    for name in ('time_stretch', 'resample', 'formant_match'):
        real = getattr(type(gpu_engine), name)
        monkeypatch.setattr(type(gpu_engine), name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name), _real(self, *a, **k))[1])
    same = tts(text, preserve_formants=False, formant_steps=0.0, **kw)
    assert calls == [] and _bits(same['audio'], plain['audio'])
    assert _bits(tts(text, preserve_formants=True, **kw)['audio'], plain['audio']) and calls == []
    kept = tts(text, pitch_steps=4, preserve_formants=True, **kw)
    assert calls == ['time_stretch', 'resample', 'formant_match']
    want = effects.pitch_shift(plain['audio'], 4.0, engine=gpu_engine, preserve_formants=True)
    assert _bits(kept['audio'], want) and kept['time'] == plain['time'] and len(want) == len(plain['audio'])
    assert not _bits(want, effects.pitch_shift(plain['audio'], 4.0, engine=gpu_engine))
    del calls[:]
    sized = tts(text, formant_steps=-2, **kw)
    assert calls == ['formant_match'] and _bits(sized['audio'], effects.formant_shift(plain['audio'], -2.0, engine=gpu_engine))
    assert all(_bits(a, b) for a, b in zip(plain['mel'], kept['mel']))
