"""GPU: time stretching (csrc/stft_inv.hip: tts_hip_time_stretch) against the float64 restatement of tests/time_stretch_ref.py,
stage by stage (`HipEngine.time_stretch_probe`) on every case of tests/time_stretch_cases.py, on ragged batches with a rate per
row, on the host, device and stream routes, end to end (amplitude and frequency at every rate), and through
`effects.pitch_shift` and the sentence pipeline's `speed` / `pitch_steps`; bounds from tests/time_stretch_cases.py."""
import ctypes

import numpy as np
import pytest

import stft_inv_ref as R
import time_stretch_cases as C
import time_stretch_ref as V
from test_time_stretch import CHECK_RATES, EDGE, FREQS, HZ_TOL, RMS_TOL, RMS_WANT, SR, two_tones

pytestmark = pytest.mark.gpu

PROBED = ('spectrum', 'magnitude', 'owner', 'operand', 'frames')


def _plan(eng, g):
    from text_to_speech_amd.stft import STFT
    return STFT(filter_length=g.fl, hop_length=g.hop, win_length=g.wl, engine=eng)._plan()


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize('name', C.NAMES)
def test_stage_by_stage(gpu_engine, name):
    """Every probe stage against float64 applied to the run's own previous stage: the owners equal, the others within the
    bounds of the case's plan.  No case is left out of any comparison."""
    case = C.BY_NAME[name]
    g, x = case.geom, C.audio_of(name)
    plan = _plan(gpu_engine, g)
    F, T, S = g.frames(case.n), V.out_frames(g.frames(case.n), case.rate), V.out_samples(case.n, case.rate)
    kept = {what: gpu_engine.time_stretch_probe(plan, x, case.rate, what) for what in PROBED}
    audio, out_lengths = gpu_engine.time_stretch(plan, x, case.rate)
    assert audio.shape == (S,) and out_lengths.tolist() == [S] and out_lengths.dtype == np.int32
    assert kept['spectrum'].shape == (1, F, 2 * g.cut) and kept['magnitude'].shape == kept['owner'].shape == (1, T, g.cut)
    assert kept['operand'].shape == (1, T, 2 * g.cut) and kept['frames'].shape == (1, T, g.fl)
    assert _bits(kept['spectrum'], gpu_engine.mel_fn_probe(plan, x, 'spectrum'))
    row = {what: a[0] for what, a in kept.items()}
    row['audio'] = audio
    errs = C.stage_errors(name, row.__getitem__)
    print(name, ' '.join(f'{s} {e:.3e}' for s, e in errs.items()))
    assert errs['owner'] == 0
    for s, bound in C.BOUNDS[case.group].items():
        assert errs[s] <= bound, (s, errs[s], bound)
    keep = min(S, g.samples(T))
    assert np.isfinite(audio).all() and (audio[keep:] == 0).all()
    if case.signal == 'zeros' or T == 1:
        assert (audio == 0).all()
    if case.signal == 'zeros':
        assert (row['magnitude'] == 0).all() and (row['owner'] == -1).all() and (row['operand'] == 0).all() and (row['frames'] == 0).all()
    if case.signal == 'gaps':                                   # the branch without peaks ran, between frames that have peaks
        silent = (row['owner'] < 0).all(axis=1)
        assert silent.any() and not silent.all() and (row['operand'][silent] == 0).all()


@pytest.mark.parametrize('group', ['small', 'gapped', 'default'])
def test_ragged_rows_with_a_rate_each(gpu_engine, group):
    """Six rows, a rate each (0.25, 1 and 4 among them), NaN behind every length: finite, every row bit-equal to the row called
    alone (test_stage_by_stage holds single rows to the restatement), zero beyond what it holds; a repeat gives the same
    bits."""
    g = C.GEOMS[group]
    plan = _plan(gpu_engine, g)
    N = 9 * g.fl // 2 + 7
    lengths = [N, g.hop, N - g.hop // 2 - 1, 2 * g.fl, N // 2, g.fl + 1]
    rates = [0.25, 1.0, 4.0, 1.37, 0.8, 2.0]
    x = np.stack([C.signal('noisy', N, g, seed=b) for b in range(6)])
    for b, L in enumerate(lengths):
        x[b, L:] = np.nan
    got, out_lengths = gpu_engine.time_stretch(plan, x, rates, lengths=lengths)
    S = [V.out_samples(L, r) for L, r in zip(lengths, rates)]
    assert got.shape == (6, max(S)) and out_lengths.tolist() == S and np.isfinite(got).all()
    again, _ = gpu_engine.time_stretch(plan, x, rates, lengths=lengths)
    assert _bits(again, got)
    for b, (L, r) in enumerate(zip(lengths, rates)):
        alone, n_alone = gpu_engine.time_stretch(plan, x[b, :L], r)
        assert alone.shape == (S[b],) and n_alone.tolist() == [S[b]]
        assert _bits(got[b, :S[b]], alone) and (got[b, S[b]:] == 0).all(), (b, L, r)
        keep = min(S[b], g.samples(V.out_frames(g.frames(L), r)))
        assert (alone[keep:] == 0).all() and np.abs(alone[:keep]).max() > 0


def test_host_device_and_stream_give_the_same_bits(gpu_engine):
    import torch
    g = C.GEOMS['default']
    plan = _plan(gpu_engine, g)
    x = np.stack([C.signal('noisy', 6000, g, seed=b) for b in range(3)])
    lengths, rates = [6000, 2500, 700], [0.8, 1.25, 0.5]
    first, n_first = gpu_engine.time_stretch(plan, x, rates, lengths=lengths)
    assert _bits(gpu_engine.time_stretch(plan, x, rates, lengths=lengths)[0], first)
    xd = torch.as_tensor(x).cuda()
    on_device, n_dev = gpu_engine.time_stretch(plan, xd, rates, lengths=lengths)
    assert on_device.is_cuda and _bits(on_device.cpu().numpy(), first) and n_dev.tolist() == n_first.tolist()
    stream = torch.cuda.Stream()
    queued, _ = gpu_engine.time_stretch(plan, xd, rates, lengths=lengths, stream=stream)
    stream.synchronize()
    assert _bits(queued.cpu().numpy(), first)
    assert torch.equal(xd, torch.as_tensor(x).cuda())
    # a scalar rate is every row's; one row without the batch axis comes back without it
    same, _ = gpu_engine.time_stretch(plan, x, 0.8)
    assert _bits(same, gpu_engine.time_stretch(plan, x, [0.8] * 3)[0])
    assert _bits(gpu_engine.time_stretch(plan, x[0], 0.8)[0], same[0])


def test_rate_one_is_the_denoiser_at_strength_zero(gpu_engine):
    """Both are the plan's transform and inverse with the spectrum's own phases in between.  The bound: every bin of a frame
    off by the operand bound (2.5e-6 of the frame's peak, A N / 4 for a tone of amplitude A under the Hann window) with
    independent signs moves a sample of the time frame by sqrt(513) x 2.5e-6 x A N / 4 x 2 / (N x 4) = 7e-6 A; four frames
    overlap, divided by a summed squared window of 1.5 and scaled by 4: at most 10.7 times that, 7.6e-5, rounded up."""
    g = C.GEOMS['default']
    plan = _plan(gpu_engine, g)
    x = C.signal('noisy', 20 * 256 + 77, g, seed=3)[None]
    got, _ = gpu_engine.time_stretch(plan, x, 1.0)
    want = gpu_engine.denoise(plan, x, np.zeros(g.cut, np.float32), 0.0)
    err = R.row_error(got, want)
    print(f'rate 1 against denoise(strength=0): {err:.3e}')
    assert got.shape == want.shape and err <= 1e-4


@pytest.mark.parametrize('f', FREQS)
def test_amplitude_and_frequency_survive_every_rate(gpu_engine, f):
    """The CPU suite's properties on the GPU's output: all seven rates of one tone as the rows of one call."""
    from text_to_speech_amd import effects
    x = np.tile(two_tones(f).astype(np.float32), (len(CHECK_RATES), 1))
    got, out_lengths = effects.time_stretch(x, list(CHECK_RATES), engine=gpu_engine)
    for b, r in enumerate(CHECK_RATES):
        assert out_lengths[b] == int(np.rint(SR / r))
        inner = got[b, EDGE:out_lengths[b] - EDGE]
        rms, hz = V.rms(inner), V.dominant_hz(inner)
        print(f'f {f} rate {r}: rms {rms:.4f} ({abs(rms / RMS_WANT - 1):.2%}), peak {hz:.3f} Hz')
        assert abs(rms / RMS_WANT - 1) <= RMS_TOL and abs(hz - f) <= HZ_TOL


def test_pitch_shift_is_its_two_parts(gpu_engine):
    import torch
    from text_to_speech_amd import effects
    eng = gpu_engine
    x = np.stack([two_tones(220.3).astype(np.float32)[:12000], two_tones(1000.0).astype(np.float32)[:12000]])
    lengths = [12000, 9000]
    for n_steps in (-3, 7):
        r, p, q = effects.pitch_ratio(n_steps)
        stretched, n = eng.time_stretch(effects.default_plan(eng), x, r, lengths=lengths)
        want = effects.fix_length(eng.resample(stretched, p, q, lengths=n), 12000).copy()
        want[1, 9000:] = 0
        got = effects.pitch_shift(x, n_steps, engine=eng, lengths=lengths)
        assert got.shape == x.shape and _bits(got, want)
        on_device = effects.pitch_shift(torch.as_tensor(x).cuda(), n_steps, engine=eng, lengths=lengths)
        assert on_device.is_cuda and _bits(on_device.cpu().numpy(), want)
        hz = V.dominant_hz(got[0, EDGE:-EDGE])
        assert abs(hz - 220.3 * 2 ** (n_steps / 12)) <= HZ_TOL, (n_steps, hz)


def test_refusals_through_the_real_symbols(gpu_engine):
    """The messages are the front end's (tests/test_time_stretch.py), with the entry point's name in front."""
    eng, g = gpu_engine, C.GEOMS['small']
    plan = _plan(eng, g)
    lib, h = eng._lib, eng._h
    x = np.ones((2, 400), np.float32)
    out = np.full((2, 400), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ones, fast, bad_lengths = np.array([1.0, 1.0]), np.array([1.0, 4.5]), np.array([400, 0], np.int32)       # kept alive
    whisper = eng.mel_fn(dict(kind='whisper', sampling_rate=16000, n_mel_channels=80, filter_length=400, hop_length=160,
                              win_length=400, mel_fmin=0.0, mel_fmax=8000.0))
    emph = eng.mel_fn(dict(sampling_rate=22050, n_mel_channels=1, filter_length=64, hop_length=16, win_length=64, mel_fmin=0.0,
                           mel_fmax=11025.0, pre_emph=0.97))

    def call(audio=p(x), B=2, N=400, lengths=None, rates=p(ones), fn=plan.handle, res=p(out), M=400, mem=0):
        rc = lib.tts_hip_time_stretch(h, audio, B, N, lengths, rates, fn, res, M, mem)
        return rc, (lib.tts_hip_last_error(h) or b'').decode()

    table = [
        (dict(fn=ctypes.c_void_p(0x1234), audio=None), 'time_stretch: not a plan of this handle'),
        (dict(audio=None), 'time_stretch: bad argument'), (dict(rates=None), 'time_stretch: bad argument'),
        (dict(lengths=p(bad_lengths)), 'time_stretch: lengths[1] = 0 outside [1, N = 400]'),
        (dict(fn=whisper.handle), 'time_stretch: refused for a Whisper plan'),
        (dict(fn=emph.handle), 'time_stretch: pre_emph = 0.97 > 0 cannot be inverted'),
        (dict(rates=p(fast)), 'time_stretch: rates[1] = 4.5 must be finite and lie in [0.25, 4]'),
        (dict(M=399), 'time_stretch: M = 399, but max_b llrint(lengths[b] / rates[b]) = 400'),
        (dict(mem=2), 'time_stretch: bad mem kind 2'),
    ]
    for kw, message in table:
        rc, msg = call(**kw)
        assert rc == -1 and msg == message, (kw, rc, msg)
    assert (out == 7.0).all()                                                # nothing was written
    for what, message in ((5, 'time_stretch_probe: no stage 5 (0 .. 4)'), (-1, 'time_stretch_probe: no stage -1 (0 .. 4)')):
        rc = lib.tts_hip_time_stretch_probe(h, p(x), 2, 400, None, p(ones), plan.handle, what, p(out), 400, 0)
        assert rc == -1 and (lib.tts_hip_last_error(h) or b'').decode() == message
    rc = lib.tts_hip_time_stretch_async(h, p(x), 2, 400, None, None, plan.handle, p(out), 400, None)
    assert rc == -1 and (lib.tts_hip_last_error(h) or b'').decode() == 'time_stretch_async: bad argument'
    assert lib.tts_hip_time_stretch_samples(plan.handle, 401, 2.0) == 200 and lib.tts_hip_time_stretch_frames(plan.handle, 401, 2.0) == 13
    assert lib.tts_hip_time_stretch_samples(whisper.handle, 4000, 1.0) == -1 and lib.tts_hip_time_stretch_frames(plan.handle, 401, 5.0) == -1
    for bad in (5.0, float('nan'), [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match='rate must'):
            eng.time_stretch(plan, x, bad)
    # a good call on the same handle still succeeds: rate 1 gives the row back where the window rebuilds it
    rc, msg = call()
    assert rc == 0, msg
    assert np.isfinite(out).all() and np.abs(out[:, 64:320] - 1.0).max() <= 1e-4


def test_the_sentence_pipeline_takes_speed_and_pitch_steps(gpu_engine, monkeypatch):
    """tts(..., speed=, pitch_steps=) is `effects` applied to the plain result; with the defaults nothing new is called."""
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
    for name in ('time_stretch', 'resample'):
        real = getattr(type(gpu_engine), name)
        monkeypatch.setattr(type(gpu_engine), name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name), _real(self, *a, **k))[1])
    same = tts(text, speed=1.0, pitch_steps=0.0, **kw)
    assert calls == [] and _bits(same['audio'], plain['audio']) and same['time'] == plain['time']
    fast = tts(text, speed=1.25, pitch_steps=-2, **kw)
    assert calls == ['time_stretch', 'time_stretch', 'resample']
    want, _ = effects.time_stretch(plain['audio'], 1.25, engine=gpu_engine)
    want = effects.pitch_shift(want, -2.0, engine=gpu_engine)
    assert _bits(fast['audio'], want) and fast['time'] == len(want) / 22050 and len(want) == V.out_samples(len(plain['audio']), 1.25)
    assert all(_bits(a, b) for a, b in zip(plain['mel'], fast['mel']))
    rt = HipRuntime('w', model='waveglow', engine=gpu_engine, seed=0)
    assert _bits(rt.time_stretch(plain['audio'], 1.25)[0], effects.time_stretch(plain['audio'], 1.25, engine=gpu_engine)[0])
