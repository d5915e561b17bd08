"""CPU: the definitions behind the WaveGlow denoiser (csrc/stft_inv.hip: tts_hip_denoise) -- the float64 restatement
(tests/denoise_ref.py) on its own, the bounds the GPU tests use (each above the float32 numpy copy's own distance from float64
and a factor ten below every planted mistake on the case it shows best in), the host-only front end (csrc/audio_call.h:
denoise_check) through csrc/host_check.cpp's `denoise` kind, built with -fsanitize=address,undefined as a stand-alone
program, and the host logic that decides where the denoiser runs, on recording stand-ins for the runtime."""
import numpy as np
import pytest

import denoise_cases as C
import denoise_ref as D
import stft_inv_ref as R
from test_audio_call import _accepted, _refused, carved, ceil_div, checker      # noqa: F401  (checker: the fixture)

_LOUD = tuple(n for n in C.NAMES if C.BY_NAME[n].signal != 'silence')


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('base', sorted({c.base for c in C.CASES if c.geom.fl != 1024 or c.F == 65}))
def test_identities(base):
    case = C.BY_NAME[base + '_s1']
    g, x, bias = case.geom, C.audio_of(case), C.bias_of(case.geom)
    spec = R.transform(x, g)
    # strength 0 is the inverse of the transform (|X| X / |X| is X up to float64 rounding)
    assert R.row_error(D.denoise(x, bias, 0.0, g), D.cut_rows(R.inverse(spec, g), [case.n], g, case.n)) <= 1e-12
    # a bias above every magnitude closes the gate
    m = D.magnitude(spec, g)
    assert (D.denoise(x, np.full(g.cut, m.max() + 1.0), 1.0, g) == 0).all()
    for s in C.STRENGTHS:
        op = D.gate(spec, bias, s, g)
        gm = D.magnitude(op, g)
        assert (gm <= m * (1 + 1e-12)).all()
        is_open = gm > 1e-9 * max(m.max(), 1.0)
        cross = op[..., :g.cut] * spec[..., g.cut:] - op[..., g.cut:] * spec[..., :g.cut]      # sin of the angle between them
        dot = op[..., :g.cut] * spec[..., :g.cut] + op[..., g.cut:] * spec[..., g.cut:]
        assert (np.abs(cross[is_open]) <= 1e-12 * (gm * m)[is_open]).all() and (dot[is_open] > 0).all()
        want = np.maximum(m - s * bias.astype(np.float64), 0)
        assert np.abs(gm - want).max() <= 1e-12 * max(m.max(), 1.0)
    if case.signal == 'silence':
        assert (D.denoise(x, bias, 1.0, g) == 0).all() and (D.denoise(x, bias, 1.0, g, dtype=np.float32) == 0).all()


def test_both_branches_of_the_gate_run_on_the_tone_cases():
    for name in C.NAMES:
        case = C.BY_NAME[name]
        if case.signal == 'tone' and case.strength == 1.0:
            share = D.clamped_share(R.transform(C.audio_of(case), case.geom), C.bias_of(case.geom), case.s, case.geom)
            print(name, f'clamped {share:.0%}')
            assert C.CLAMPED[0] <= share <= C.CLAMPED[1], (name, share)


def test_rows_are_cut_to_their_lengths():
    """Lengths that are no multiple of the hop, and a row shorter than win_length: the row keeps min(length, samples of its
    frames) samples of the inverse of its own zero-padded samples."""
    for g in R.GEOMS[:3]:
        n = g.samples(9)
        rng = np.random.default_rng(n)
        x = rng.standard_normal((4, n))
        lengths = [n, n - g.hop // 2 - 1, g.wl - 3, g.half + 1]
        got = D.denoise(x, C.bias_of(g), 0.5, g, lengths)
        for b, L in enumerate(lengths):
            keep = D.kept_samples(L, g)
            assert keep <= L and (got[b, keep:] == 0).all() and np.abs(got[b, :keep]).max() > 0
            alone = D.denoise(x[b:b + 1, :L], C.bias_of(g), 0.5, g)
            assert np.array_equal(got[b, :keep], alone[0, :keep])
    assert D.kept_samples(13, R.GEOMS[0]) == 13                          # padded to win_length = 16 by the plan, cut back
    g = R.GEOMS[3]
    assert [D.kept_samples(f * 256, g) for f in (1, 2, 5, 12)] == [256, 512, 1280, 3072]   # a vocoder row gets its samples back


# ---- bounds ------------------------------------------------------------------------------------------------------------
def test_bounds_lie_above_float32():
    worst = {}
    for name in C.NAMES:
        runner = C.numpy_runner(name)
        for s, e in C.stage_errors(name, runner).items():
            worst[s] = max(worst.get(s, 0.0), e)
        if C.BY_NAME[name].signal == 'silence':
            assert (runner('operand') == 0).all() and (runner('audio') == 0).all()
    print('float32 numpy distances', {s: f'{e:.3e}' for s, e in worst.items()})
    assert C.BOUNDS['operand'] / 12 <= worst['operand'] <= C.BOUNDS['operand'] / 8      # ten times it, rounded up to two digits
    for s, e in worst.items():
        assert e <= C.BOUNDS[s] / 5, (s, e, C.BOUNDS[s])


@pytest.mark.parametrize('plant', D.GATE_MISTAKES)
def test_operand_bound_lies_below_planted_mistakes(plant):
    """A mistake in the gate (float64 run with the mistake, judged like a GPU run) moves the operand of the case it shows best
    in by at least ten times the bound."""
    effects = [(C.stage_errors(name, C.numpy_runner(name, np.float64, plant))['operand'], name) for name in _LOUD]
    best = max(effects)
    print(plant, 'best-showing case', best, 'weakest', min(effects))
    assert best[0] >= 10 * C.BOUNDS['operand'], best
    assert best[0] >= 6e-2


def test_audio_bound_lies_below_a_missing_cut():
    """`no_cut` shows where a row is shorter than what its frames overlap-add to: a row the plan zero-pads to win_length."""
    effects = []
    for g in R.GEOMS:
        n = g.samples(9)
        x = R.signal('tone', n, g, seed=9)[None]
        lengths = [g.wl // 2 + 1]
        assert D.kept_samples(lengths[0], g) == lengths[0] < g.samples(g.frames(lengths[0]))
        good = D.denoise(x, C.bias_of(g), 1.0, g, lengths)
        bad = D.denoise(x, C.bias_of(g), 1.0, g, lengths, plant='no_cut')
        effects.append((R.row_error(bad, good), g))
    print('no_cut best-showing case', max(effects, key=lambda t: t[0]))
    assert max(e for e, _ in effects) >= 10 * C.BOUNDS['audio']


# ---- the second table: gapped, sparse, long --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.EXTRA_NAMES)
def test_extra_bounds_lie_above_float32(name):
    gname = name.split('_')[0]
    bounds = C.EXTRA_BOUNDS[gname]
    errs = C.stage_errors(name, C.numpy_runner(name))
    print(name, 'float32 numpy distances', {s: f'{e:.3e}' for s, e in errs.items()}, 'bounds', bounds)
    assert bounds['operand'] / 12 <= errs['operand'] <= bounds['operand'] / 8           # ten times it, rounded up to two digits
    for s, e in errs.items():
        assert e <= bounds[s] / 5, (s, e, bounds[s])
    # a sample no window covers comes back 0, whatever the gate did
    case = C.case_of(name)
    bare = C.SC.uncovered(case.geom, case.F)
    assert bare.any() == (gname != 'long') and (D.denoise(C.audio_of(case), C.bias_of(case.geom), case.s, case.geom)[0][bare] == 0).all()


@pytest.mark.parametrize('plant', D.GATE_MISTAKES)
@pytest.mark.parametrize('name', C.EXTRA_NAMES)
def test_extra_operand_bound_lies_below_planted_mistakes(name, plant):
    """Every gate mistake moves the operand of every extra case by at least ten times its bound -- but the missing clamp on
    gapped, where no bin of the tone lies under half the bias and nothing clamps."""
    case = C.case_of(name)
    share = D.clamped_share(R.transform(C.audio_of(case), case.geom), C.bias_of(case.geom), case.s, case.geom)
    effect = C.stage_errors(name, C.numpy_runner(name, np.float64, plant))['operand']
    print(name, plant, f'effect {effect:.3e} clamped {share:.0%}')
    if plant == 'no_clamp' and share == 0:
        assert name.startswith('gapped') and effect == 0
    else:
        assert effect >= 10 * C.EXTRA_BOUNDS[name.split('_')[0]]['operand'] and effect >= 4e-3


# ---- the front end, as a stand-alone program under ASan / UBSan ----------------------------------------------------------
def _plan(g=R.GEOMS[0], **more):
    return dict(filter_length=g.fl, hop_length=g.hop, win_length=g.wl, n_mel_channels=1, mel_fmax=11025, **more)


def geometry(g, B, N, lengths):
    """What denoise_check derives: the transform's workspace (MelGeom), the inverse's on the same frame slots (GlGeom of the
    inverse alone), frames and kept samples per row."""
    cut, fl = g.cut, g.fl
    K4, Kpad, NB, MAGK = ceil_div(fl, 4) * 4, ceil_div(fl, 32) * 32, ceil_div(2 * cut, 32) * 32, ceil_div(cut, 32) * 32
    Fr = g.frames(N)
    PW = max(N, g.wl) + 2 * g.half
    NP = ceil_div(PW + K4 - fl, 4) * 4
    rows = B * Fr
    fwd = [8 * B, 4 * B, B * NP * 4 + 256, rows * Kpad * 4 if g.hop % 4 else 0, rows * NB * 4, rows * MAGK * 4, 0]
    inv = [4 * B, 0, rows * NB * 4, 0, 0, rows * fl * 4]
    lengths = list(lengths) or [N] * B
    return [[Fr, PW, NP, carved(*fwd[:2]), carved(*fwd[:4]), carved(*fwd)],
            [Fr, carved(*inv[:2]), carved(*inv[:5]), carved(*inv)],
            [g.frames(L) for L in lengths], [D.kept_samples(L, g) for L in lengths]]


@pytest.mark.parametrize('g', R.GEOMS)
def test_geometry(checker, g):
    rng = np.random.default_rng(g.fl)
    for _ in range(6):
        N = int(rng.integers(g.half + 1, 12 * g.fl))
        B = int(rng.integers(1, 6))
        lengths = [int(v) for v in rng.integers(1, N + 1, B)]
        lengths[0] = N
        if B > 1:
            lengths[1] = max(1, min(N, g.wl - 1))                        # shorter than win_length: zero-padded by the plan
        if B > 2:
            lengths[2] = max(1, N - g.hop // 2 - 1)                      # no multiple of the hop
        assert _accepted(checker, 'denoise', lengths, N=N, **_plan(g)) == geometry(g, B, N, lengths), (N, lengths)
        assert _accepted(checker, 'denoise', B=B, N=N, what=2, **_plan(g)) == geometry(g, B, N, ())


@pytest.mark.parametrize('gname', ['long', 'sparse'])
def test_geometry_on_the_extra_plans(checker, gname):
    """hop > filter_length and filter_length = 2048 through the same stand-alone sweep (gapped refuses the sweep's row of
    win_length - 1 samples: REFUSALS has that message)."""
    test_geometry(checker, C.SC.EXTRA_GEOMS[gname][0])


OK = dict(B=2, N=40, strength=0.5, **_plan())
REFUSALS = [
    # (lengths, settings, substrings of the message), in the documented order
    ((), dict(OK, null='audio'), ['bad argument']),
    ((), dict(OK, null='out'), ['bad argument']),
    ((), dict(OK, null='fn'), ['bad argument']),
    ((), dict(OK, B=0), ['bad argument']),
    ((), dict(OK, N=0), ['bad argument']),
    ((40, 0), OK, ['lengths[1] = 0 outside [1, N = 40]']),
    ((41, 40), OK, ['lengths[0] = 41 outside [1, N = 40]']),
    ((40, 3), dict(OK, **_plan(R.Geom(16, 4, 4))), ['row 1: max(L = 3, win_length = 4) samples are not more than filter_length // 2 = 8']),
    ((), dict(OK, mel_kind=1), ['refused for a Whisper plan']),
    ((), dict(OK, null='bias'), ['bias is NULL']),
    ((), dict(OK, strength=-0.1), ['strength = -0.1 must be finite and >= 0']),
    ((), dict(OK, strength='nan'), ['strength = nan must be finite']),
    ((), dict(OK, strength='inf'), ['strength = inf must be finite']),
    ((), dict(OK, B=65536), ['too large for 31-bit offsets (B <= 65535)']),
    ((), dict(OK, B=3, N=180000000), ['B = 3 x N = 180000000 too large']),
    ((), dict(OK, B=40, N=4000000), ['too large']),                   # the workspaces pass 2^31 before the audio does
    ((), dict(OK, mem=2), ['bad mem kind 2']),
    ((), dict(OK, what=3), ['no stage 3 (0 .. 2)']),
]


@pytest.mark.parametrize('lengths,settings,needles', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals(checker, lengths, settings, needles):
    _refused(checker, 'denoise', needles, lengths, **settings)


def test_first_match_wins(checker):
    short = _plan(R.Geom(16, 4, 4))
    every = dict(OK, **short, mel_kind=1, null='bias', strength=-1, mem=2, what=3)
    assert 'bad argument' in _refused(checker, 'denoise', [], (), **dict(every, B=0))
    assert 'lengths[0] = 41' in _refused(checker, 'denoise', [], (41, 3), **every)
    assert 'row 1' in _refused(checker, 'denoise', [], (40, 3), **every)
    assert 'Whisper' in _refused(checker, 'denoise', [], (40, 9), **every)
    assert 'bias is NULL' in _refused(checker, 'denoise', [], (40, 9), **dict(every, mel_kind=0))
    assert 'strength' in _refused(checker, 'denoise', [], (40, 9), **dict(every, mel_kind=0, null=''))
    assert 'too large' in _refused(checker, 'denoise', [], (), **dict(every, mel_kind=0, null='', strength=0, B=65536))
    assert 'mem kind' in _refused(checker, 'denoise', [], (40, 9), **dict(every, mel_kind=0, null='', strength=0))
    assert 'no stage 3' in _refused(checker, 'denoise', [], (40, 9), **dict(every, mel_kind=0, null='', strength=0, mem=0))
    assert _accepted(checker, 'denoise', (40, 9), **dict(every, mel_kind=0, null='', strength=0, mem=0, what=-1))


# ---- where the denoiser runs: host logic on recording stand-ins ----------------------------------------------------------
class _Engine:
    """An engine stand-in that records the vocoder calls it gets."""
    device = 0

    def __init__(self):
        self.calls = []

    def waveglow_infer(self, mel, **kw):
        self.calls.append(('waveglow_infer', tuple(mel.shape), kw))
        return np.zeros((mel.shape[0], mel.shape[1] * 256), np.float32)


class _Runtime:
    """A runtime stand-in behind `WaveGlow`: records every vocoder call and every whole-waveform denoise."""

    def __init__(self):
        self.calls, self.denoised = [], []

    def __call__(self, mel, **kw):
        self.calls.append((tuple(mel.shape), kw))
        return np.ones((mel.shape[0], mel.shape[1] * 256), np.float32)

    def denoise(self, audio, strength=0.1, lengths=None, precision=None):
        self.denoised.append((tuple(audio.shape), strength, precision))
        return 2 * np.atleast_2d(audio)


def test_no_strength_adds_no_call():
    from text_to_speech_amd.runtime import HipRuntime
    for off in (None, 0, 0.0):
        eng = _Engine()
        rt = HipRuntime('x', model='waveglow', engine=eng, seed=1)
        before = rt._offset
        out = rt.waveglow_infer(np.zeros((2, 3, 80), np.float32), denoiser_strength=off, deterministic=True)
        assert out.shape == (2, 768) and len(eng.calls) == 1 and '_denoisers' not in eng.__dict__
        assert eng.calls[0][2] == {'sigma': 1.0, 'precision': 'f32', 'z': None} and rt._offset == before
    with pytest.raises(ValueError, match='denoiser_strength'):
        HipRuntime('x', model='waveglow', engine=_Engine()).waveglow_infer(np.zeros((1, 3, 80), np.float32), denoiser_strength=-1)
    with pytest.raises(ValueError, match='denoiser_strength'):
        HipRuntime('x', model='waveglow', engine=_Engine()).waveglow_infer(np.zeros((1, 3, 80), np.float32),
                                                                          denoiser_strength=float('nan'))


def test_one_denoiser_per_precision_and_handle():
    from text_to_speech_amd.runtime import HipRuntime
    eng = _Engine()
    a, b = HipRuntime('x', engine=eng), HipRuntime('y', engine=eng, vocoder_precision='f16x3')
    assert a.denoiser() is a.denoiser('f32') is b.denoiser('f32') and b.denoiser() is a.denoiser('f16x3')
    assert a.denoiser().precision == 'f32' and b.denoiser().precision == 'f16x3' and a.denoiser() is not b.denoiser()
    assert sorted(eng._denoisers) == ['f16x3', 'f32'] and eng.calls == []           # building one runs nothing
    d = a.denoiser()
    assert (d.stft.filter_length, d.stft.hop_length, d.stft.win_length) == (1024, 256, 1024)


def test_windowed_and_exact_paths_denoise_once():
    from text_to_speech_amd.waveglow import WaveGlow
    mel = np.zeros((1, 700, 80), np.float32)
    # a direct call passes the keyword on
    rt = _Runtime()
    WaveGlow(rt).infer(mel, denoiser_strength=0.3, sigma=0.5)
    assert rt.calls == [((1, 700, 80), {'denoiser_strength': 0.3, 'sigma': 0.5})] and rt.denoised == []
    # stitched windows: no window sees it, the whole waveform is denoised once
    for batch in (False, True):
        rt = _Runtime()
        out = WaveGlow(rt).infer(mel, win_len=256, denoiser_strength=0.3, precision='f16x3', batch=batch)
        plain = WaveGlow(_Runtime()).infer(mel, win_len=256, precision='f16x3', batch=batch)
        assert len(rt.calls) == (1 if batch else 4) and all('denoiser_strength' not in kw for _, kw in rt.calls)
        assert rt.denoised == [((700 * 256,), 0.3, 'f16x3')]
        assert out.shape == plain.shape == (700 * 256,) and np.array_equal(out, 2 * plain)
    # a mel that fits one window, and a batch, are direct calls
    rt = _Runtime()
    WaveGlow(rt).infer(mel[:, :200], win_len=256, denoiser_strength=0.3)
    WaveGlow(rt).infer(np.zeros((2, 700, 80), np.float32), win_len=256, denoiser_strength=0.3)
    assert [kw.get('denoiser_strength') for _, kw in rt.calls] == [0.3, 0.3] and rt.denoised == []
    rt = _Runtime()
    WaveGlow(rt).infer(mel[:, :200], win_len=256)
    assert rt.calls == [((1, 200, 80), {})]                                 # without the keyword the call is today's
    # infer_exact: tiles without it, one denoise of the whole
    rt = _Runtime()
    out = WaveGlow(rt).infer_exact(mel, tile_frames=300, denoiser_strength=0.2)
    assert len(rt.calls) == 3 and all('denoiser_strength' not in kw for _, kw in rt.calls)
    assert rt.denoised == [((1, 700 * 256), 0.2, None)] and out.shape == (1, 700 * 256) and (out == 2).all()
    rt = _Runtime()
    assert (WaveGlow(rt).infer_exact(mel, tile_frames=300) == 1).all() and rt.denoised == []
    with pytest.raises(ValueError, match='whole waveform'):
        WaveGlow(rt).infer_exact(mel, tile_frames=300, tiles=[0], denoiser_strength=0.2)
    with pytest.raises(ValueError, match='denoise'):
        WaveGlow(lambda m, **kw: np.ones((1, m.shape[1] * 256), np.float32)).infer(mel, win_len=256, denoiser_strength=0.3)


def test_the_pipeline_forwards_the_keyword():
    from text_to_speech_amd.tacotron2 import Tacotron2, _stage_kwargs
    from text_to_speech_amd.waveglow import WaveGlow
    rt = _Runtime()
    voc = WaveGlow(rt)
    _, vocode, finish = _stage_kwargs(dict(vocoder=voc, vocoder_config={'denoiser_strength': 0.01}, reduce_noise=True))
    assert 'vocoder_config' not in finish
    part = {'mel': [np.zeros((5, 80), np.float32), np.zeros((0, 80), np.float32), np.zeros((7, 80), np.float32)]}
    audios, _ = Tacotron2._vocode_parts(None, part, utterance=3, **vocode)
    assert [a.shape for a in audios] == [(5 * 256,), (7 * 256,)]
    assert [kw['denoiser_strength'] for _, kw in rt.calls] == [0.01, 0.01] and rt.calls[0][1]['streams'] == [(3, 0)]
    rt.calls.clear()
    grouped, _ = Tacotron2._vocode_group(None, [part, part], [3, 4], packed=True, **vocode)
    assert len(rt.calls) == 1 and rt.calls[0][1]['denoiser_strength'] == 0.01 and rt.calls[0][1]['packed'] is True
    assert list(rt.calls[0][1]['lengths']) == [5, 7, 5, 7] and [len(a) for a in grouped] == [2, 2]
