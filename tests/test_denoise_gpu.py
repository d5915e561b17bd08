"""GPU: the WaveGlow denoiser (csrc/stft_inv.hip: tts_hip_denoise) against the float64 restatement of tests/denoise_ref.py, stage
by stage (`HipEngine.denoise_probe`), on ragged batches, in place, through `Denoiser`, `HipRuntime.waveglow_infer(...,
denoiser_strength=)` and the sentence pipeline; bounds from tests/denoise_cases.py."""
import ctypes

import numpy as np
import pytest

import denoise_cases as C
import denoise_ref as D
import stft_inv_cases as SC
import stft_inv_ref as R

pytestmark = pytest.mark.gpu


def _plan(eng, g):
    from text_to_speech_amd.stft import STFT
    return STFT(filter_length=g.fl, hop_length=g.hop, win_length=g.wl, engine=eng)._plan()


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize('name', C.NAMES)
def test_stage_by_stage(gpu_engine, name):
    """The spectrum bit-equal to the mel plan's own; the operand against the float64 gate of the run's spectrum; the time frames
    and the audio against float64 on the run's operand."""
    case = C.BY_NAME[name]
    g, x, bias = case.geom, C.audio_of(case), C.bias_of(case.geom)
    plan = _plan(gpu_engine, g)
    kept = {what: gpu_engine.denoise_probe(plan, x, bias, case.strength, what) for what in ('spectrum', 'operand', 'frames')}
    kept['audio'] = gpu_engine.denoise(plan, x, bias, case.strength)
    assert kept['audio'].shape == x.shape and kept['frames'].shape == (1, case.F, g.fl)
    assert _bits(kept['spectrum'], gpu_engine.mel_fn_probe(plan, x, 'spectrum'))
    errs = C.stage_errors(name, kept.__getitem__)
    print(name, ' '.join(f'{s} {e:.3e}' for s, e in errs.items()))
    for s, e in errs.items():
        assert e <= C.BOUNDS[s], (s, e)
    if case.signal == 'silence':
        assert (kept['operand'] == 0).all() and (kept['audio'] == 0).all()
    if case.signal == 'tone' and case.strength == 1.0:
        share = D.clamped_share(kept['spectrum'], bias, case.s, g)
        assert C.CLAMPED[0] <= share <= C.CLAMPED[1], share


@pytest.mark.parametrize('g,F', [(R.GEOMS[0], 8), (R.GEOMS[1], 9), (R.GEOMS[2], 12), (R.GEOMS[3], 65)])
def test_ragged_rows_equal_single_rows(gpu_engine, g, F):
    """Rows of {1, 2, F / 2, F - 1, F} hops of samples and one length that is no multiple of the hop, NaN behind each row's
    length: finite, every row bit-equal to the row alone, zero beyond what the row keeps."""
    plan = _plan(gpu_engine, g)
    N = F * g.hop
    lengths = [g.hop, 2 * g.hop, (F // 2) * g.hop, (F - 1) * g.hop, N, N - g.hop // 2 - 1]
    rng = np.random.default_rng(F)
    x = rng.uniform(-0.8, 0.8, (len(lengths), N)).astype(np.float32)
    for b, L in enumerate(lengths):
        x[b, L:] = np.nan
    bias = C.bias_of(g)
    got = gpu_engine.denoise(plan, x, bias, 0.5, lengths=lengths)
    assert got.shape == x.shape and np.isfinite(got).all()
    for b, L in enumerate(lengths):
        keep = D.kept_samples(L, g)
        alone = gpu_engine.denoise(plan, x[b:b + 1, :L], bias, 0.5)
        assert alone.shape == (1, L) and (alone[0, keep:] == 0).all()
        assert _bits(got[b, :keep], alone[0, :keep]) and (got[b, keep:] == 0).all() and np.abs(got[b, :keep]).max() > 0, (b, L)


@pytest.mark.parametrize('name', C.EXTRA_NAMES)
def test_stage_by_stage_on_the_extra_geometries(gpu_engine, name):
    """test_stage_by_stage on the second table (gapped, sparse, long) under its own bounds; a sample no window covers is
    exactly 0 in the audio."""
    case = C.case_of(name)
    g, x, bias = case.geom, C.audio_of(case), C.bias_of(case.geom)
    bounds = C.EXTRA_BOUNDS[name.split('_')[0]]
    plan = _plan(gpu_engine, g)
    kept = {what: gpu_engine.denoise_probe(plan, x, bias, case.strength, what) for what in ('spectrum', 'operand', 'frames')}
    kept['audio'] = gpu_engine.denoise(plan, x, bias, case.strength)
    assert kept['audio'].shape == x.shape and kept['frames'].shape == (1, case.F, g.fl)
    assert _bits(kept['spectrum'], gpu_engine.mel_fn_probe(plan, x, 'spectrum'))
    errs = C.stage_errors(name, kept.__getitem__)
    print(name, ' '.join(f'{s} {e:.3e}' for s, e in errs.items()))
    for s, e in errs.items():
        assert e <= bounds[s], (s, e)
    bare = SC.uncovered(g, case.F)
    assert np.isfinite(kept['audio']).all() and (kept['audio'][0, bare] == 0).all() and np.abs(kept['audio'][0, ~bare]).max() > 0


def test_ragged_rows_equal_single_rows_on_the_gapped_plan(gpu_engine):
    """test_ragged_rows_equal_single_rows on (16, 4, 4).  Its lengths of one and two hops are refused there (max(L,
    win_length) must pass filter_length // 2 = 8), so the two shortest rows are 9 and 12 samples; 33 is no hop multiple.
    Beside the bits of the row alone: the samples no window covers are exactly 0, the others follow the float64 restatement."""
    g, F = SC.EXTRA_GEOMS['gapped'][0], 9
    plan = _plan(gpu_engine, g)
    N = F * g.hop
    lengths = [g.half + 1, 3 * g.hop, (F // 2) * g.hop, (F - 1) * g.hop, N, N - g.hop // 2 - 1]
    rng = np.random.default_rng(F)
    x = rng.uniform(-0.8, 0.8, (len(lengths), N)).astype(np.float32)
    for b, L in enumerate(lengths):
        x[b, L:] = np.nan
    bias = C.bias_of(g)
    got = gpu_engine.denoise(plan, x, bias, 0.5, lengths=lengths)
    assert got.shape == x.shape and np.isfinite(got).all()
    want = D.denoise(np.nan_to_num(x), bias, float(np.float32(0.5)), g, lengths)
    for b, L in enumerate(lengths):
        keep = D.kept_samples(L, g)
        alone = gpu_engine.denoise(plan, x[b:b + 1, :L], bias, 0.5)
        assert alone.shape == (1, L) and (alone[0, keep:] == 0).all()
        assert _bits(got[b, :keep], alone[0, :keep]) and (got[b, keep:] == 0).all() and np.abs(got[b, :keep]).max() > 0, (b, L)
        bare = SC.uncovered(g, g.frames(L))[:keep]
        assert bare.any() and (got[b, :keep][bare] == 0).all(), (b, L)
        err = R.row_error(got[b:b + 1, :keep], want[b:b + 1, :keep])
        print('gapped ragged', b, L, f'{err:.3e}')
        assert err <= SC.BOUNDS['inverse'], (b, L, err)


def test_repeat_in_place_and_device_input_give_the_same_bits(gpu_engine):
    import torch
    g = R.GEOMS[3]
    plan = _plan(gpu_engine, g)
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.8, 0.8, (3, 20 * 256)).astype(np.float32)
    lengths = [20 * 256, 7 * 256 + 100, 600]
    bias = C.bias_of(g)
    first = gpu_engine.denoise(plan, x, bias, 0.3, lengths=lengths)
    assert _bits(gpu_engine.denoise(plan, x, bias, 0.3, lengths=lengths), first)
    xd, bd = torch.as_tensor(x).cuda(), torch.as_tensor(bias.copy()).cuda()
    on_device = gpu_engine.denoise(plan, xd, bd, 0.3, lengths=lengths)
    assert on_device.is_cuda and _bits(on_device.cpu().numpy(), first)
    stream = torch.cuda.Stream()
    queued = gpu_engine.denoise(plan, xd, bd, 0.3, lengths=lengths, stream=stream)
    stream.synchronize()
    assert _bits(queued.cpu().numpy(), first)
    work = xd.clone()
    same = gpu_engine.denoise(plan, work, bd, 0.3, lengths=lengths, out=work)
    assert same.data_ptr() == work.data_ptr() and _bits(work.cpu().numpy(), first)
    assert torch.equal(xd, torch.as_tensor(x).cuda())                       # the out-of-place calls left their input alone


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
def test_denoiser_bias(gpu_engine, precision):
    from text_to_speech_amd.denoiser import Denoiser
    den = Denoiser(gpu_engine, precision=precision)
    hum = gpu_engine.waveglow_infer(np.zeros((1, 88, 80), np.float32), z=np.zeros((1, 88 * 32, 8), np.float32), sigma=0.0,
                                    precision=precision)
    magnitude, _ = gpu_engine.stft_transform(den._plan(), hum)
    bias = den.bias
    assert bias.is_cuda and tuple(bias.shape) == (513,) and den.bias is bias
    bias = bias.cpu().numpy()
    assert _bits(bias, magnitude[0, 0]) and np.isfinite(bias).all() and bias.max() > 0 and bias.min() >= 0
    given = Denoiser(gpu_engine, bias=np.arange(513))
    assert np.array_equal(given.bias.cpu().numpy(), np.arange(513, dtype=np.float32))


@pytest.mark.parametrize('mode', ['plain', 'ragged', 'packed'])
def test_vocoder_path(gpu_engine, mode):
    """`denoiser_strength` through the runtime: None is today's call; 0.5 is the denoiser applied to the audio of the plain call,
    bit for bit, and within the inverse's bound of the float64 restatement on that audio."""
    import torch
    from text_to_speech_amd.denoiser import Denoiser
    from text_to_speech_amd.runtime import HipRuntime
    rt = HipRuntime('w', model='waveglow', engine=gpu_engine, seed=3)
    rng = np.random.default_rng(12)
    mel = rng.uniform(-11.5, 1.2, (2, 12, 80)).astype(np.float32)
    lengths = np.array([12, 5], np.int32)
    kw = {'plain': {}, 'ragged': {'lengths': lengths}, 'packed': {'lengths': lengths, 'packed': True}}[mode]
    base = rt.waveglow_infer(mel, seed=7, **kw)
    offset = rt._offset
    assert _bits(rt.waveglow_infer(mel, seed=7, denoiser_strength=None, **kw), base)
    got = rt.waveglow_infer(mel, seed=7, denoiser_strength=0.5, **kw)
    assert isinstance(got, np.ndarray) and got.shape == base.shape == (2, 12 * 256) and rt._offset == offset
    samples = lengths.astype(np.int64) * 256 if kw else None
    den = Denoiser(gpu_engine)
    assert _bits(got, den(base, 0.5, samples))
    assert rt.denoiser() is rt.denoiser('f32') and _bits(rt.denoiser().bias.cpu().numpy(), den.bias.cpu().numpy())
    want = D.denoise(base, den.bias.cpu().numpy(), 0.5, R.GEOMS[3], samples)
    for b in range(2):
        err = R.row_error(got[b:b + 1], want[b:b + 1])
        print(mode, b, f'{err:.3e}')
        assert err <= SC.BOUNDS['inverse'], (b, err)
    if kw:
        assert (got[1, 5 * 256:] == 0).all()
    # a CUDA mel in, a CUDA tensor out, the same bits
    on_device = rt.waveglow_infer(torch.as_tensor(mel).cuda(), seed=7, denoiser_strength=0.5, **kw)
    assert on_device.is_cuda and _bits(on_device.cpu().numpy(), got)
    # the stitched and the exact paths end in the same denoiser
    assert _bits(rt.denoise(base, 0.5, lengths=samples), got)
    # a call that draws its noise from the running offset advances it by the vocoder's blocks alone
    from text_to_speech_amd.runtime import noise_blocks
    offset = rt._offset
    assert np.isfinite(rt.waveglow_infer(mel, denoiser_strength=0.5, **kw)).all() and rt._offset == offset + noise_blocks(2, 12)


def test_a_row_shorter_than_the_window_keeps_its_samples(gpu_engine):
    from text_to_speech_amd.denoiser import Denoiser
    from text_to_speech_amd.runtime import HipRuntime
    rt = HipRuntime('w', model='waveglow', engine=gpu_engine, seed=3)
    mel = np.random.default_rng(2).uniform(-11.5, 1.2, (1, 2, 80)).astype(np.float32)
    base = rt.waveglow_infer(mel, deterministic=True)
    got = rt.waveglow_infer(mel, deterministic=True, denoiser_strength=0.5)
    assert got.shape == base.shape == (1, 512) and np.isfinite(got).all() and np.abs(got).max() > 0
    assert _bits(got, Denoiser(gpu_engine)(base, 0.5)) and not _bits(got, base)


def test_refusals_through_the_real_symbols(gpu_engine):
    """The messages are the front end's (tests/test_denoise.py), with the entry point's name in front."""
    eng, g = gpu_engine, R.GEOMS[0]
    plan = _plan(eng, g)
    lib, h = eng._lib, eng._h
    x = np.ones((2, 40), np.float32)
    bias = np.zeros(g.cut, np.float32)
    out = np.full((2, 40), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fr = lambda *v: p(np.asarray(v, np.int32))
    short = eng.mel_fn(dict(sampling_rate=22050, n_mel_channels=1, filter_length=16, hop_length=4, win_length=4, mel_fmin=0.0,
                            mel_fmax=11025.0))
    whisper = eng.mel_fn(dict(kind='whisper', sampling_rate=16000, n_mel_channels=80, filter_length=400, hop_length=160,
                              win_length=400, mel_fmin=0.0, mel_fmax=8000.0))

    def call(audio=p(x), B=2, N=40, lengths=None, fn=plan.handle, b=p(bias), strength=0.5, res=p(out), mem=0):
        rc = lib.tts_hip_denoise(h, audio, B, N, lengths, fn, b, strength, res, mem)
        return rc, (lib.tts_hip_last_error(h) or b'').decode()

    table = [
        (dict(audio=None), 'denoise: bad argument'), (dict(res=None), 'denoise: bad argument'), (dict(fn=None), 'denoise: bad argument'),
        (dict(B=0), 'denoise: bad argument'), (dict(N=0), 'denoise: bad argument'),
        (dict(lengths=fr(40, 0)), 'denoise: lengths[1] = 0 outside [1, N = 40]'),
        (dict(lengths=fr(41, 40)), 'denoise: lengths[0] = 41 outside [1, N = 40]'),
        (dict(fn=short.handle, lengths=fr(40, 3)),
         'denoise: row 1: max(L = 3, win_length = 4) samples are not more than filter_length // 2 = 8'),
        (dict(fn=whisper.handle), 'denoise: refused for a Whisper plan'), (dict(b=None), 'denoise: bias is NULL'),
        (dict(strength=-0.1), 'denoise: strength = -0.1 must be finite and >= 0'),
        (dict(strength=float('nan')), 'denoise: strength = nan must be finite and >= 0'),
        (dict(B=65536), 'denoise: B = 65536 x N = 40 too large for 31-bit offsets (B <= 65535)'),
        (dict(mem=2), 'denoise: bad mem kind 2'), (dict(fn=ctypes.c_void_p(0x1234)), 'denoise: not a plan of this handle'),
    ]
    for kw, message in table:
        rc, msg = call(**kw)
        assert rc == -1 and msg == message, (kw, rc, msg)
    assert (out == 7.0).all()                                                # nothing was written
    for what, message in ((3, 'denoise_probe: no stage 3 (0 .. 2)'), (-1, 'denoise_probe: no stage -1 (0 .. 2)')):
        rc = lib.tts_hip_denoise_probe(h, p(x), 2, 40, None, plan.handle, p(bias), 0.5, what, p(out), 0)
        assert rc == -1 and (lib.tts_hip_last_error(h) or b'').decode() == message
    rc = lib.tts_hip_denoise_async(h, p(x), 2, 40, None, plan.handle, None, 0.5, p(out), None)
    assert rc == -1 and (lib.tts_hip_last_error(h) or b'').decode() == 'denoise_async: bias is NULL'
    with pytest.raises(ValueError, match='bias must be'):
        eng.denoise(plan, x, np.zeros(g.cut + 1, np.float32))
    # a good call on the same handle still succeeds: a zero bias is the inverse of the transform
    rc, msg = call()
    assert rc == 0, msg
    assert np.isfinite(out).all() and np.abs(out - 1.0).max() <= 1e-4


def test_the_sentence_pipeline_takes_the_keyword(gpu_engine):
    """tts(..., vocoder_config={'denoiser_strength': s}): every part's waveform is the denoised waveform of the plain run."""
    from text_to_speech_amd.denoiser import Denoiser
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2, tts
    from text_to_speech_amd.waveglow import WaveGlow
    model = Tacotron2(HipRuntime('t', model='tacotron2', engine=gpu_engine, seed=0))
    voc = WaveGlow(HipRuntime('w', model='waveglow', engine=gpu_engine, seed=0))
    kw = dict(model=model, vocoder=voc, max_length=6., max_text_length=-2, save=False, seed=5)
    plain = tts('Hello there. General test!', **kw)
    clean = tts('Hello there. General test!', vocoder_config={'denoiser_strength': 0.01}, **kw)
    frames = [m.shape[0] for m in plain['mel']]
    assert frames == [m.shape[0] for m in clean['mel']] and all(_bits(a, b) for a, b in zip(plain['mel'], clean['mel']))
    assert clean['audio'].shape == plain['audio'].shape == (sum(frames) * 256,) and np.isfinite(clean['audio']).all()
    den, at, parts = Denoiser(gpu_engine), 0, []
    for f in frames:
        parts.append(den(plain['audio'][at:at + f * 256], 0.01)[0])
        at += f * 256
    assert _bits(clean['audio'], np.concatenate(parts)) and not _bits(clean['audio'], plain['audio'])
