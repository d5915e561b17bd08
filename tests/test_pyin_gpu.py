"""GPU: tts_hip_pyin stage by stage (through tts_hip_pyin_probe), each stage against float64 applied to the run's own stage before
it (pyin_ref.check_run, the bounds tests/test_pyin.py holds a float32 numpy copy to), so that no bound has to cover a comparison
float32 and float64 decide differently:

  p             within 5 2^-24 of the prior's total of float64 on the run's own d' (from tts_hip_pitch_probe)
  obs, cand     from the run's own p: a bin of K troughs within K - 1 roundings; cand within a place of float32(period)
  v             within n_bins roundings of the sum of the run's own obs
  delta         one step from the run's own delta_{t-1}, obs and v within bound_delta
  back          the float64 argmax wherever the best two predecessors lie more than twice that bound apart, elsewhere a
                predecessor within twice the bound of the best
  path          the exact backtrack of the run's own back from the first maximum of its last delta
  planes        within 2 roundings of the double formulas on the run's own path, cand and v
  end to end    the float64 score of the run's path within bound_score of the float64 optimum of the same model; f0 of the sine
                rows within F0_END_TO_END of the all-float64 restatement where both decode the same voiced state
  zeros at and behind a row's frames

Then: rows alone bit-equal to rows of the ragged batch with NaN behind every length, host = device = stream, repeats, the YIN
call's stages bit-equal to what the commit before this call gave on the same inputs (tests/golden/pitch_yin_bits.json: sha256 of
every stage's bytes), f0_error on pYIN tracks along a DTW path, and `resynthesis_f0` / `evaluate_synthesis` with f0_method='pyin'
bit-equal to their parts.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import pitch_cases as pc
import pitch_ref as pr
import pyin_cases as yc
import pyin_ref as yr
from test_pitch import F0_END_TO_END

pytestmark = pytest.mark.gpu

CASES = yc.cases()
STAGES = ('trough', 'obs', 'delta', 'back', 'path')


def _yin_kw(kw):
    return {k: kw[k] for k in ('rate', 'hop', 'win', 'fmin', 'fmax')}


@pytest.fixture(scope='module')
def runs(gpu_engine):
    """every case run once: name -> dict(dp, trough, obs, delta, back, path, out)"""
    got = {}
    for name, c in CASES.items():
        r = {w: gpu_engine.pyin_probe(c['audio'], c['lengths'], what=w, **c['kw']) for w in STAGES}
        r['dp'] = gpu_engine.pitch_probe(c['audio'], c['lengths'], what='cmnd', **_yin_kw(c['kw']))
        r['out'] = gpu_engine.pyin(c['audio'], c['lengths'], **c['kw'])
        got[name] = r
    return got


def _row(r, b, Fb=None):
    """the row's run as pyin_ref.check_run takes it, its first Fb frames"""
    s = slice(None, Fb)
    return dict(p=r['trough'][b, s], obs=r['obs'][0, b, s], cand=r['obs'][1, b, s], delta=r['delta'][b, s], back=r['back'][b, s],
                path=r['path'][b, s], planes=r['out'][:, b, s])


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_stage_against_float64_of_the_stage_before(runs, name):
    c, r = CASES[name], runs[name]
    cfg, nb = c['cfg'], c['cfg']['n_bins']
    B, N = c['audio'].shape
    F = pr.frame_count(N, c['grid']['hop'])
    assert r['out'].dtype == np.float32 and r['out'].shape == (3, B, F) and r['trough'].shape == (B, F, cfg['tau_max'] + 1)
    assert r['obs'].shape == (2, B, F, nb) and r['delta'].shape == r['back'].shape == (B, F, 2 * nb) and r['path'].shape == (B, F)
    assert np.isnan(c['audio']).any() or np.all(c['lengths'] == N)
    worst = {}
    for b, kind in enumerate(c['kinds']):
        Fb = pr.frame_count(int(c['lengths'][b]), c['grid']['hop'])
        for m in (r['trough'][b, Fb:], r['obs'][:, b, Fb:], r['delta'][b, Fb:], r['back'][b, Fb:], r['path'][b, Fb:], r['out'][:, b, Fb:]):
            assert np.all(m == 0), (name, b)
        run = _row(r, b, Fb)
        assert all(np.isfinite(m).all() for m in run.values()), (name, b)
        dp = r['dp'][b, :Fb]
        pos = yr.positions(dp, cfg)
        assert not len(pos) or np.abs(pos - np.floor(pos) - 0.5).min() > 1e-9, (name, b)         # no candidate on a bin's edge
        for stage, ratio in yr.check_run(run, dp, cfg, f'{name}[{b}]').items():
            worst[stage] = max(worst.get(stage, 0.0), ratio)
        if kind in ('zeros', 'dc'):                                    # d' flat at 1: no trough, nothing voiced
            inside = slice(2, Fb - 2) if kind == 'dc' and Fb > 4 else slice(0, Fb if kind == 'zeros' else 0)
            assert np.all(run['planes'][2][inside] == 0) and np.all(run['planes'][0][inside] == 0) and np.all(run['path'][inside] >= nb), (name, b)
        if kind in ('sine_int', 'sine_frac') and Fb > 4:
            ref = yr.track(c['audio'][b], int(c['lengths'][b]), hop=c['grid']['hop'], win=c['grid']['win'], **cfg)
            same = (ref['path'] == run['path']) & (ref['path'] < nb) & (ref['cand'][np.arange(Fb), ref['path'] % nb] > 0)
            rel = np.abs(run['planes'][0][same] - ref['f0'][same]) / ref['f0'][same]
            if same.any():
                print(f'{name}[{b}] {kind} f0 end to end: largest relative error {rel.max():.3g} on {same.sum()} frames')
                assert np.all(rel <= F0_END_TO_END), (name, b, float(rel.max()))
    print(f'{name}: largest error / bound per stage', {k: round(v, 3) for k, v in worst.items()})


def test_values_exactly_on_a_threshold(runs):
    """d' = 1/2 and 3/4 bit for bit at troughs, thresholds at 1/4 steps: the threshold a d' sits on is not above it (check_run
    holds p to the rule; `<=` would move 0.3 and 0.2 of mass, tests/test_pyin.py)"""
    r, cfg = runs['on_threshold'], CASES['on_threshold']['cfg']
    on = 0
    for b in range(2):
        for t in range(1, 4):
            q = r['dp'][b, t]
            flag = yr.troughs(q, cfg['tau_min'], cfg['tau_max'])
            hit = flag & np.isin(q, (0.25, 0.5, 0.75))
            on += int(hit.sum())
            wrong = yr.trough_probs(q, flag, cfg['prior_table'], cfg['no_trough_prob'], 'threshold_le')
            if hit.any():
                assert np.abs(r['trough'][b, t] - wrong).max() > 0.05
    assert on >= 3


def test_a_row_alone_gives_the_bits_it_gives_in_the_batch_and_repeats(gpu_engine, runs):
    for name in ('default', 'lags_2_3_step1', 'bins_65'):
        c, r = CASES[name], runs[name]
        again = gpu_engine.pyin(c['audio'], c['lengths'], **c['kw'])
        assert np.array_equal(again, r['out']), name
        for b, n in enumerate(c['lengths']):
            row = c['audio'][b, :n]
            F1 = pr.frame_count(n, c['grid']['hop'])
            one = gpu_engine.pyin(row, **c['kw'])
            assert one.shape == (3, 1, F1) and np.array_equal(one[:, 0], r['out'][:, b, :F1]), (name, b)
            for w in ('obs', 'delta', 'back'):
                one = gpu_engine.pyin_probe(row, what=w, **c['kw'])
                want = r[w][:, b, :F1] if w == 'obs' else r[w][b, :F1]
                assert np.array_equal(one[:, 0] if w == 'obs' else one[0], want), (name, b, w)


def test_host_device_and_stream_calls_agree_to_the_bit(gpu_engine, runs):
    import torch
    c, r = CASES['default'], runs['default']
    dev = torch.as_tensor(np.nan_to_num(c['audio'], nan=7.0)).cuda()          # other garbage behind the lengths
    o_dev = gpu_engine.pyin(dev, c['lengths'], **c['kw'])
    assert o_dev.is_cuda and np.array_equal(o_dev.cpu().numpy(), r['out'])
    stream = torch.cuda.Stream()
    o_str = gpu_engine.pyin(dev, c['lengths'], stream=stream, **c['kw'])
    stream.synchronize()
    assert np.array_equal(o_str.cpu().numpy(), r['out'])
    for w in ('trough', 'path'):
        p_dev = gpu_engine.pyin_probe(dev, c['lengths'], what=w, **c['kw'])
        assert p_dev.is_cuda and np.array_equal(p_dev.cpu().numpy(), r[w])


def test_yin_gives_the_bits_it_gave_before(gpu_engine):
    """tts_hip_pitch shares its frame stages with the new kernel: every stage of it, on the inputs of tests/pitch_cases.py,
    hashes to what the library gave before the stages were shared (the values tests/test_pitch_gpu.py holds to float64)."""
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'pitch_yin_bits.json')) as f:
        want = json.load(f)
    cases = pc.cases()
    assert sorted(want) == sorted(cases)
    for name, c in cases.items():
        for w in ('difference', 'cmnd', 'pick'):
            got = np.ascontiguousarray(gpu_engine.pitch_probe(c['audio'], c['lengths'], what=w, **c['kw']))
            assert hashlib.sha256(got.tobytes()).hexdigest() == want[name][w], (name, w)
        got = np.ascontiguousarray(gpu_engine.pitch(c['audio'], c['lengths'], **c['kw']))
        assert hashlib.sha256(got.tobytes()).hexdigest() == want[name]['pitch'], name


def test_f0_error_on_pyin_tracks_along_a_dtw_path(gpu_engine):
    import mel_dtw_cases as mc
    from test_pitch_gpu import check_f0_error
    B, n = 3, 30 * 256
    a = np.stack([pc.signal(k, n, 110, seed=r) for r, k in enumerate(('vibrato', 'tone_noise', 'missing_fundamental'))])
    b = np.stack([pc.signal(k, n + 1024, 118, seed=5 + r) for r, k in enumerate(('vibrato', 'noise', 'sine_frac'))])
    la, lb = np.array([n, n - 700, 20 * 256], np.int32), np.array([n + 1024, n, n + 1000], np.int32)
    fa, fb = gpu_engine.pyin(a, la)[0], gpu_engine.pyin(b, lb)[0]
    Fa, Fb = fa.shape[1], fb.shape[1]
    ta, tb = (1 + la // 256).astype(np.int32), (1 + lb // 256).astype(np.int32)
    assert (fa[0, 3:-3] > 0).all() and (fb[1] == 0).all()            # the tone is voiced throughout, the noise nowhere
    ma = np.stack([mc.log_mel(np.random.default_rng(r), Fa) for r in range(B)])
    mb = np.stack([mc.log_mel(np.random.default_rng(9 + r), Fb) for r in range(B)])
    _, path = gpu_engine.mel_dtw(ma, mb, ta, tb, return_path=True)
    got = gpu_engine.f0_error(fa, fb, ta, tb, path)
    check_f0_error('pyin tracks, dtw path', got, fa, fb, ta, tb, path)
    assert got[1, 0] > 20 and got[1, 1] == 0 and got[4, 1] > 20     # voiced pairs of the two tones; tone against noise: voicing errors only


def test_the_library_refuses_by_name(gpu_engine):
    from text_to_speech_amd import HipLibraryError
    x = np.zeros((1, 8), np.float32)
    table = np.full(4, 0.25, np.float32)
    args = lambda **kw: (lambda ins, outs, where: (ins[0], 1, 8, None, 22050, 4, 8, 1, 3, table, 4, 0.01, kw.get('fmin', 60.0), 10,
                                                   kw.get('n_bins', 4), kw.get('max_step', 2), 0.01, *kw.get('what', ()), outs[0], *where))
    with pytest.raises(HipLibraryError, match=r'pyin: n_bins = 0 is outside \[1, 1024\]'):
        gpu_engine._call('pyin', [(x, (1, 8), 'float32')], lambda new: (new((3, 1, 3)),), args(n_bins=0), twin=False)
    with pytest.raises(HipLibraryError, match=r'pyin: max_step = 5 is outside \[1, n_bins = 4\]'):
        gpu_engine._call('pyin', [(x, (1, 8), 'float32')], lambda new: (new((3, 1, 3)),), args(max_step=5), twin=False)
    with pytest.raises(HipLibraryError, match=r'pyin_probe: what = 5 is no stage'):
        gpu_engine._call('pyin_probe', [(x, (1, 8), 'float32')], lambda new: (new((3, 1, 3)),), args(what=(5,)), twin=False)
    with pytest.raises(ValueError, match='max_step'):
        gpu_engine.pyin(x, hop=4, win=8, n_bins=4, max_step=5)


def test_resynthesis_f0_with_pyin_is_its_parts_bit_for_bit(gpu_engine):
    import torch
    import mel_dtw_cases as mc
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.waveglow import WaveGlow
    rt = HipRuntime('synthetic', engine=gpu_engine, seed=7)
    mel = mc.log_mel(np.random.default_rng(12), 40)
    wave = pc.signal('vibrato', 40 * 256 - 300, 100)
    res = WaveGlow(rt).resynthesis_f0([(wave, mel)], f0_method='pyin', f0_config=dict(switch_prob=0.02), seed=5)
    assert res['names'] == WaveGlow.RESYNTHESIS_NAMES and res['per_item'].shape == (6, 1)
    audio = rt.waveglow_infer(torch.as_tensor(mel).cuda()[None], seed=5)
    padded = np.zeros((1, 40 * 256), np.float32)
    padded[0, :len(wave)] = wave
    f_rec, f_voc = gpu_engine.pyin(padded, switch_prob=0.02)[0], gpu_engine.pyin(audio[:, :40 * 256], switch_prob=0.02)[0]
    assert f_voc.is_cuda and tuple(f_voc.shape) == (1, 41) and (f_rec[0, 2:-3] > 0).all()
    s = gpu_engine.f0_error(f_rec, f_voc).cpu().numpy()[:, 0]
    want = np.array([s[2], s[3], s[4] / s[0], s[5] / max(s[1], 1), s[1], s[0]], np.float32)
    assert np.array_equal(res['per_item'][:, 0], want) and s[0] == 41 and np.isfinite(want).all()
    yin = WaveGlow(rt).resynthesis_f0([(wave, mel)], seed=5)         # the default is the threshold tracker, as before
    s = gpu_engine.f0_error(gpu_engine.pitch(padded)[0], gpu_engine.pitch(audio[:, :40 * 256])[0]).cpu().numpy()[:, 0]
    assert np.array_equal(yin['per_item'][:, 0], np.array([s[2], s[3], s[4] / s[0], s[5] / max(s[1], 1), s[1], s[0]], np.float32))


def test_evaluate_synthesis_with_pyin_is_its_parts_bit_for_bit(gpu_engine):
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
    items = list(zip(texts, waves))
    res = model.evaluate_synthesis(items, batch_size=2, max_length=3., vocoder=Seeded(), f0_method='pyin', f0_config=dict(no_trough_prob=0.02))
    assert res['names'] == Tacotron2.SYNTHESIS_NAMES + Tacotron2.SYNTHESIS_F0_NAMES
    per = res['per_item']
    assert per.shape == (10, 2) and per.dtype == np.float32 and np.isfinite(per).all()
    toks = [np.asarray(model.encode_text(model.clean_text(t), cleaned=True), np.int32) for t in texts]
    loaded = [np.asarray(load_audio(w, 22050, engine=gpu_engine), np.float32) for w in waves]
    mels = [np.asarray(load_mel(w, engine=gpu_engine, normalize=False), np.float32) for w in loaded]
    tok = np.zeros((2, max(len(t) for t in toks)), np.int32)
    target = np.zeros((2, 41, 80), np.float32)
    recorded = np.zeros((2, max(len(w) for w in loaded)), np.float32)
    for r in range(2):
        tok[r, :len(toks[r])], target[r, :len(mels[r])], recorded[r, :len(loaded[r])] = toks[r], mels[r], loaded[r]
    out = rt.tacotron2_infer(tok, max_length=3., deterministic=True, on_device=True)
    frames = out.lengths.cpu().numpy().astype(np.int32)
    wanted, samples = np.array([23, 41], np.int32), np.array([len(w) for w in loaded], np.int32)
    assert frames.min() >= 1
    _, path = gpu_engine.mel_dtw(out.mel, target, frames, wanted, return_path=True)
    audio = rt.waveglow_infer(out.mel, lengths=frames, seed=5)[:, :out.mel.shape[1] * 256]
    f_syn = gpu_engine.pyin(audio, frames * 256, no_trough_prob=0.02)[0]
    f_rec = gpu_engine.pyin(recorded, samples, no_trough_prob=0.02)[0]
    s = gpu_engine.f0_error(f_syn, f_rec, frames, np.minimum(wanted, 1 + samples // 256).astype(np.int32), path).cpu().numpy()
    want = np.stack([s[2], s[4] / np.maximum(s[0], 1), s[5] / np.maximum(s[1], 1), s[1]]).astype(np.float32)
    assert np.array_equal(per[6:], want), (per[6:], want)
    yin = model.evaluate_synthesis(items, batch_size=2, max_length=3., vocoder=Seeded())
    assert np.array_equal(yin['per_item'][:6], per[:6]) and not np.array_equal(yin['per_item'][6:], per[6:])
