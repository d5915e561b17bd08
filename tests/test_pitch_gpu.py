"""GPU: tts_hip_pitch stage by stage (through tts_hip_pitch_probe), each stage against float64 applied to the run's own stage
before it, so that no bound has to cover a comparison that float32 and float64 decide differently:

  difference    within (W + 4) 2^-24 d of float64 on the same float32 samples
  normalised    within (tau + 4) 2^-24 d' of float64 on the run's own d
  pick          flag and tau* exactly those of the documented rule on the run's own d'
  period, f0    within 2 roundings of the double formula on the run's own d'(tau* - 1 .. tau* + 1)
  aperiodicity  bit-equal to the probe's d'(tau*)
  zeros at and behind a row's frames

On the frames tests/pitch_ref.py finds STABLE, flag and tau* are also those of the all-float64 restatement, and on the STABLE
voiced frames of the two sines f0 is within F0_END_TO_END = 6.3e-6 relative of the restatement's (tests/test_pitch.py derives that
bound: ten times the 6.3e-7 of a float32 numpy copy, a tenth and less of the planted mistakes; the device was seen at 7.1e-7).  Then:
rows alone bit-equal to rows of the ragged batch with NaN behind every length, host = device = stream, tts_hip_f0_error
against float64 on the diagonal, on a path from mel_dtw, on a path cut short by -1 and on one with a pair out of range, and
`WaveGlow.resynthesis_f0` / `Tacotron2.evaluate_synthesis(vocoder=)` bit-equal to their parts.
"""
import numpy as np
import pytest

import pitch_cases as pc
import pitch_ref as pr
from test_pitch import F0_END_TO_END

pytestmark = pytest.mark.gpu

CASES = pc.cases()


def check_row(name, x, n, kind, cfg, d, dp, picked, out, F):
    """Every stage check of one row: d, dp [F, lags], picked [2, F], out [3, F] of the row."""
    W, tau_min, tau_max, rate = cfg['win'], cfg['tau_min'], cfg['tau_max'], cfg['rate']
    Fb = pr.frame_count(n, cfg['hop'])
    assert d.shape == dp.shape == (F, tau_max + 1) and picked.shape == (2, F) and out.shape == (3, F), name
    for m in (d[Fb:], dp[Fb:], picked[:, Fb:], out[:, Fb:]):
        assert np.all(m == 0), name
    d, dp, picked, out = d[:Fb], dp[:Fb], picked[:, :Fb], out[:, :Fb]
    assert all(np.isfinite(m).all() for m in (d, dp, picked, out)), name
    ref = pr.track(x, n, **cfg)
    err, bound = np.abs(d - ref['d']), pr.bound_d(ref['d'], W)
    print(f'{name} d: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}')
    assert np.all(err <= bound), name
    assert np.all(d[:, 0] == 0), name
    want = pr.cmnd(d)
    err, bound = np.abs(dp - want), pr.bound_cmnd(want)
    print(f"{name} d': largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert np.all(err <= bound) and np.all(dp[:, 0] == 1), name
    voiced, taus = pr.pick(dp, tau_min, tau_max, cfg['threshold'])
    assert np.array_equal(picked[0], voiced.astype(np.float32)) and np.array_equal(picked[1], taus.astype(np.float32)), name
    f0, period, ap = pr.planes(dp, voiced, taus, rate, tau_max)
    assert np.all(np.abs(out[0] - f0) <= pr.bound_rounded(f0, 2)) and np.all(out[0][~voiced] == 0), name
    assert np.all(np.abs(out[1] - period) <= pr.bound_rounded(period, 2)), name
    assert np.array_equal(out[2], dp[np.arange(Fb), taus]), name
    ok = pr.stable(ref['d'], ref['dp'], tau_min, tau_max, cfg['threshold'])
    assert np.array_equal(voiced[ok], ref['voiced'][ok]) and np.array_equal(taus[ok], ref['tau'][ok]), name
    if kind in ('sine_int', 'sine_frac'):
        sel = ok & ref['voiced']
        rel = np.abs(out[0][sel] - ref['f0'][sel]) / ref['f0'][sel]
        if sel.any():
            print(f'{name} {kind} f0 end to end: largest relative error {rel.max():.3g} on {sel.sum()} frames')
            assert np.all(rel <= F0_END_TO_END), (name, float(rel.max()))
    return int(ok.sum()), Fb


@pytest.fixture(scope='module')
def runs(gpu_engine):
    """every case run once: name -> (d, dp, pick, out)"""
    got = {}
    for name, c in CASES.items():
        got[name] = tuple(gpu_engine.pitch_probe(c['audio'], c['lengths'], what=w, **c['kw']) for w in ('difference', 'cmnd', 'pick')) + (
            gpu_engine.pitch(c['audio'], c['lengths'], **c['kw']),)
    return got


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_stage_against_float64_of_the_stage_before(runs, name):
    c = CASES[name]
    d, dp, picked, out = runs[name]
    B, N = c['audio'].shape
    F = pr.frame_count(N, c['cfg']['hop'])
    assert out.dtype == np.float32 and out.shape == (3, B, F)
    assert np.isnan(c['audio']).any() or np.all(c['lengths'] == N)
    for b, kind in enumerate(c['kinds']):
        check_row(f'{name}[{b}]', c['audio'][b], int(c['lengths'][b]), kind, c['cfg'], d[b], dp[b], picked[:, b], out[:, b], F)


def test_closed_forms_on_the_device(runs):
    c = CASES['default']
    k = c['kinds'].index
    d, dp, picked, out = (m[..., 2:21] if m.ndim == 3 and m.shape[0] in (2, 3) and m.shape[1] == len(c['kinds']) else m[:, 2:21] for m in runs['default'])      # the frames inside the rows
    # the square wave of period 100: d(P) = d(2P) = d(3P) = 0 exactly, the first of them is taken
    sq = k('square')
    assert np.all(d[sq][:, [100, 200, 300]] == 0) and np.all(picked[0, sq] == 1) and np.all(picked[1, sq] == 100)
    assert np.all(out[2, sq] == 0) and np.all(np.abs(out[1, sq] - 100) < 0.01)      # d' is not symmetric about P: delta is small, not 0
    for flat in (k('zeros'), k('dc')):                               # S = 0: d' = 1 everywhere, unvoiced, the smallest lag of the tie
        assert np.all(d[flat] == 0) and np.all(dp[flat] == 1) and np.all(picked[0, flat] == 0) and np.all(picked[1, flat] == 45)
        assert np.all(out[0, flat] == 0) and np.all(out[1, flat] == 45) and np.all(out[2, flat] == 1)


def test_a_value_on_the_threshold_is_not_below_it(runs):
    """threshold = 1 on silence and DC: d' = 1 by rule is not < 1, so the frames are unvoiced at tau_min (`<=` would call them
    voiced); check_row holds the same frames to the rule on the run's own d'."""
    c = CASES['on_threshold']
    assert c['kw']['threshold'] == 1.0 and c['kinds'] == ('zeros', 'dc')
    d, dp, picked, out = runs['on_threshold']
    for b, frames in ((0, slice(None)), (1, slice(2, 3))):             # every frame of the silent row, the one inside the DC row
        assert np.all(dp[b, frames] == 1) and np.all(picked[0, b, frames] == 0) and np.all(picked[1, b, frames] == 2)
        assert np.all(out[0, b, frames] == 0) and np.all(out[1, b, frames] == 2) and np.all(out[2, b, frames] == 1)


def test_a_row_alone_gives_the_bits_it_gives_in_the_batch(gpu_engine, runs):
    for name in ('ragged', 'small'):
        c = CASES[name]
        d, dp, picked, out = runs[name]
        for b, n in enumerate(c['lengths']):
            row = c['audio'][b, :n]
            F1 = pr.frame_count(n, c['cfg']['hop'])
            one = gpu_engine.pitch(row, **c['kw'])
            assert one.shape == (3, 1, F1) and np.array_equal(one[:, 0], out[:, b, :F1]), (name, b)
            one = gpu_engine.pitch_probe(row, what='cmnd', **c['kw'])
            assert np.array_equal(one[0], dp[b, :F1]), (name, b)


def test_host_device_and_stream_calls_agree_to_the_bit(gpu_engine, runs):
    import torch
    c = CASES['ragged']
    out = runs['ragged'][3]
    dev = torch.as_tensor(np.nan_to_num(c['audio'], nan=7.0)).cuda()          # other garbage behind the lengths
    o_dev = gpu_engine.pitch(dev, c['lengths'], **c['kw'])
    assert o_dev.is_cuda and np.array_equal(o_dev.cpu().numpy(), out)
    stream = torch.cuda.Stream()
    o_str = gpu_engine.pitch(dev, c['lengths'], stream=stream, **c['kw'])
    stream.synchronize()
    assert np.array_equal(o_str.cpu().numpy(), out)
    p_dev = gpu_engine.pitch_probe(dev, c['lengths'], what='pick', **c['kw'])
    assert p_dev.is_cuda and np.array_equal(p_dev.cpu().numpy(), runs['ragged'][2])
    # the comparison too: tracks and path on the device, on a stream
    f0 = out[0]
    want = gpu_engine.f0_error(f0[:4], f0[1:5])
    got = gpu_engine.f0_error(o_dev[0, :4], o_dev[0, 1:5])
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    got = gpu_engine.f0_error(o_dev[0, :4], f0[1:5], stream=stream)
    stream.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def _tracks(rng, B, Fa, Fb):
    """two ragged batches of F0 tracks with unvoiced stretches, NaN and garbage behind the lengths"""
    def one(F):
        f = 120.0 * 2 ** rng.uniform(-0.6, 0.9, (B, F))
        f[rng.random((B, F)) < 0.3] = 0.0
        f[rng.random((B, F)) < 0.03] = np.nan
        f[rng.random((B, F)) < 0.03] = -50.0
        return f.astype(np.float32)
    return one(Fa), one(Fb)


def check_f0_error(name, got, a, b, la, lb, paths):
    assert got.dtype == np.float32 and got.shape == (6, len(la)), name
    for r in range(len(la)):
        want = pr.f0_error(a[r], b[r], int(la[r]), int(lb[r]), None if paths is None else paths[r])
        assert np.array_equal(got[[0, 1, 4, 5], r], want[[0, 1, 4, 5]]), (name, r, got[:, r], want)
        assert np.all(np.abs(got[[2, 3], r] - want[[2, 3]]) <= pr.bound_rounded(want[[2, 3]], 4)), (name, r, got[:, r], want)


def test_f0_error_against_float64(gpu_engine):
    rng = np.random.default_rng(5)
    B, Fa, Fb = 5, 300, 341                                          # more than one round of the 256 threads
    a, b = _tracks(rng, B, Fa, Fb)
    la, lb = np.array([300, 1, 257, 256, 77], np.int32), np.array([341, 9, 255, 256, 300], np.int32)
    for r in range(B):
        a[r, la[r]:], b[r, lb[r]:] = np.nan, 1e9
    a[1, 0], b[1, :9] = 0.0, 0.0                                     # a row without a voiced pair: rmse and mean 0
    check_f0_error('diagonal', gpu_engine.f0_error(a, b, la, lb), a, b, la, lb, None)
    full = gpu_engine.f0_error(a, b)                                 # no lengths: every frame, the garbage is unvoiced or counted as it is
    assert full[0].tolist() == [300] * B
    # a path from mel_dtw, on mels of these lengths
    import mel_dtw_cases as mc
    ma = np.stack([mc.log_mel(np.random.default_rng(r), Fa) for r in range(B)])
    mb = np.stack([mc.log_mel(np.random.default_rng(9 + r), Fb) for r in range(B)])
    _, path = gpu_engine.mel_dtw(ma, mb, la, lb, return_path=True)
    assert path.shape == (B, Fa + Fb - 1, 2)
    got = gpu_engine.f0_error(a, b, la, lb, path)
    check_f0_error('dtw path', got, a, b, la, lb, path)
    assert np.array_equal(got[0], [(path[r, :, 0] >= 0).sum() for r in range(B)])
    import torch
    _, p_dev = gpu_engine.mel_dtw(torch.as_tensor(ma).cuda(), mb, la, lb, return_path=True)
    on_dev = gpu_engine.f0_error(a, b, la, lb, p_dev)                # the path stays where mel_dtw wrote it
    assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), got)
    cut = path.copy()
    cut[0, 100:], cut[2, 0], cut[3, 300] = -1, -1, (-1, 5)           # cut short, empty, one index negative
    out_of_range = path.copy()
    out_of_range[0, 290], out_of_range[4, 50], out_of_range[3, 10] = (300, 5), (5, 300), (3, 256)      # i = la, j = lb, j = lb
    for name, p in (('cut short', cut), ('out of range', out_of_range)):
        got = gpu_engine.f0_error(a, b, la, lb, p)
        check_f0_error(name, got, a, b, la, lb, p)
    assert gpu_engine.f0_error(a, b, la, lb, cut)[0].tolist()[:3] == [100, 9, 0]
    assert np.array_equal(gpu_engine.f0_error(a, b, la, lb, cut)[:, 2], [0] * 6)
    # a row alone, and the metrics wrapper
    alone = gpu_engine.f0_error(a[4, :77], b[4, :300], path=path[4, :376])
    assert np.array_equal(alone[:, 0], gpu_engine.f0_error(a, b, la, lb, path)[:, 4])
    from text_to_speech_amd import metrics
    res = metrics.f0_error(gpu_engine, a, b, la, lb, path)
    assert list(res)[:6] == list(metrics.F0_STATS) and np.array_equal(res['vuv_error'], res['vuv_errors'] / res['pairs'])


def test_gross_cents_is_a_strict_threshold(gpu_engine):
    a = np.array([[100.0, 100.0, 100.0, 0.0]], np.float32)
    b = np.array([[120.0, 200.0, 100.0, 100.0]], np.float32)
    got = gpu_engine.f0_error(a, b)[:, 0]
    want = pr.f0_error(a[0], b[0], 4, 4)
    assert got.tolist()[:2] == [4, 3] and got[4] == 1 and got[5] == want[5] == 1        # 1200 cents is gross, 315.6 (float32 of 1.2) is not above itself
    assert gpu_engine.f0_error(a, b, gross_cents=1200.0)[5, 0] == 0 and gpu_engine.f0_error(a, b, gross_cents=300.0)[5, 0] == 2


def test_the_library_refuses_by_name(gpu_engine):
    from text_to_speech_amd import HipLibraryError
    with pytest.raises(HipLibraryError, match=r'pitch_probe: out too large'):
        gpu_engine._call('pitch_probe', [(np.zeros((1, 8), np.float32), (1, 8), 'float32')], lambda new: (new((1,)),),
                         lambda ins, outs, where: (ins[0], 1 << 20, 1 << 4, None, 22050, 1, 1024, 45, 367, 0.1, 0, outs[0], *where), twin=False)
    with pytest.raises(HipLibraryError, match=r'f0_error: P = 0 must be at least 1'):
        gpu_engine._call('f0_error', [(np.zeros((1, 8), np.float32), (1, 8), 'float32')], lambda new: (new((6, 1)),),
                         lambda ins, outs, where: (ins[0], ins[0], 1, 8, 8, None, None, ins[0], 0, 300.0, outs[0], *where), twin=False)


def test_resynthesis_f0_is_its_parts_bit_for_bit(gpu_engine):
    import torch
    import mel_dtw_cases as mc
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.waveglow import WaveGlow
    rt = HipRuntime('synthetic', engine=gpu_engine, seed=7)
    mel = mc.log_mel(np.random.default_rng(12), 40)
    wave = pc.signal('vibrato', 40 * 256 - 300, 100)                 # zero-padded to the mel's 40 * 256 samples
    res = WaveGlow(rt).resynthesis_f0([(wave, mel)], seed=5)
    assert res['names'] == WaveGlow.RESYNTHESIS_NAMES and res['per_item'].shape == (6, 1)
    audio = rt.waveglow_infer(torch.as_tensor(mel).cuda()[None], seed=5)
    padded = np.zeros((1, 40 * 256), np.float32)
    padded[0, :len(wave)] = wave
    f_rec, f_voc = gpu_engine.pitch(padded)[0], gpu_engine.pitch(audio[:, :40 * 256])[0]
    assert audio.is_cuda and f_voc.is_cuda and tuple(f_voc.shape) == (1, 41) and (f_rec[0, 2:-3] > 0).all()
    s = gpu_engine.f0_error(f_rec, f_voc).cpu().numpy()[:, 0]
    want = np.array([s[2], s[3], s[4] / s[0], s[5] / max(s[1], 1), s[1], s[0]], np.float32)
    assert np.array_equal(res['per_item'][:, 0], want) and s[0] == 41 and np.isfinite(want).all()
    assert res['mean'] == {n: float(v) for n, v in zip(res['names'], want)}


def test_evaluate_synthesis_with_a_vocoder_is_its_parts_bit_for_bit(gpu_engine):
    from text_to_speech_amd.audio import load_audio, load_mel
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    rt = HipRuntime('synthetic', engine=gpu_engine, seed=7)
    model, wg = Tacotron2(rt, lang='en'), WaveGlow(rt)

    class Seeded:                                                    # the same noise in the method and in its parts
        def infer(self, mel, **kw):
            return wg.infer(mel, seed=5, **kw)

    texts = ['Hello there.', 'A somewhat longer sentence, this one.']
    waves = [pc.signal('vibrato', 23 * 256 - 7, 100), pc.signal('sine_frac', 41 * 256 - 200, 140)]
    res = model.evaluate_synthesis(list(zip(texts, waves)), batch_size=2, max_length=3., vocoder=Seeded(), pitch=dict(threshold=0.15))
    assert res['names'] == Tacotron2.SYNTHESIS_NAMES + Tacotron2.SYNTHESIS_F0_NAMES
    per = res['per_item']
    assert per.shape == (10, 2) and per.dtype == np.float32 and np.isfinite(per).all()
    toks = [np.asarray(model.encode_text(model.clean_text(t), cleaned=True), np.int32) for t in texts]
    loaded = [np.asarray(load_audio(w, 22050, engine=gpu_engine), np.float32) for w in waves]      # once; the mel is of these samples
    mels = [np.asarray(load_mel(w, engine=gpu_engine, normalize=False), np.float32) for w in loaded]
    assert [len(m) for m in mels] == [23, 41]
    tok = np.zeros((2, max(len(t) for t in toks)), np.int32)
    target = np.zeros((2, 41, 80), np.float32)
    recorded = np.zeros((2, max(len(w) for w in loaded)), np.float32)
    for r in range(2):
        tok[r, :len(toks[r])], target[r, :len(mels[r])], recorded[r, :len(loaded[r])] = toks[r], mels[r], loaded[r]
    out = rt.tacotron2_infer(tok, max_length=3., deterministic=True, on_device=True)
    frames = out.lengths.cpu().numpy().astype(np.int32)
    wanted, samples = np.array([23, 41], np.int32), np.array([len(w) for w in loaded], np.int32)
    assert frames.min() >= 1
    stats, path = gpu_engine.mel_dtw(out.mel, target, frames, wanted, return_path=True)
    audio = rt.waveglow_infer(out.mel, lengths=frames, seed=5)[:, :out.mel.shape[1] * 256]
    f_syn = gpu_engine.pitch(audio, frames * 256, threshold=0.15)[0]
    f_rec = gpu_engine.pitch(recorded, samples, threshold=0.15)[0]
    s = gpu_engine.f0_error(f_syn, f_rec, frames, wanted, path).cpu().numpy()
    stats = stats.cpu().numpy()
    assert path.is_cuda and f_syn.is_cuda and np.array_equal(per[0], stats[2]) and np.array_equal(per[1], stats[1])
    assert np.array_equal(per[6], s[2]) and np.array_equal(per[9], s[1]) and np.array_equal(s[0], stats[1])      # every pair of the path
    assert np.array_equal(per[7], s[4] / s[0]) and np.array_equal(per[8], s[5] / np.maximum(s[1], 1))
    assert (gpu_engine.pitch(recorded, samples, threshold=0.15)[0][:, 3:20] > 0).all()                          # the recordings are voiced
    # the default call: the six names of before, and on the mels used above the values
    plain = model.evaluate_synthesis(list(zip(texts, mels)), batch_size=2, max_length=3.)
    assert plain['names'] == Tacotron2.SYNTHESIS_NAMES and np.array_equal(plain['per_item'], per[:6])
