"""CPU: the definitions behind csrc/stft_inv.hip -- the closed-form inverse basis against scipy's pinv, the float64
restatement (tests/stft_inv_ref.py) on its own, the host-only front end (csrc/audio_call.h: stft_inv_check, the Cholesky mel
inversion) through csrc/host_check.cpp's `stft_inv` kind, built with -fsanitize=address,undefined as a stand-alone program,
the Python objects, and the bounds the GPU tests use: each lies above the float32 numpy copy's own distance from float64
and a factor ten below the weakest planted mistake."""
import os
import subprocess

import numpy as np
import pytest

import stft_inv_cases as C
import stft_inv_ref as R
from test_audio_call import LIM, _accepted, _refused, carved, ceil_div, checker      # noqa: F401  (checker: the fixture)


# ---- the basis and the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('fl,hop,wl', [(15, 5, 12), (16, 4, 16), (64, 10, 48), (1024, 256, 1024), (33, 7, 20)])
def test_closed_form_basis_equals_pinv(fl, hop, wl):
    w = R.centred_window(R.Geom(fl, wl, hop))
    a, b = R.inverse_basis_pinv(fl, hop) * w, R.inverse_basis_closed(fl, hop) * w
    assert a.shape == (2 * (fl // 2 + 1), fl)
    assert np.abs(a - b).max() <= 1e-12
    assert np.abs(a - R.inverse_basis_closed(fl, hop, ck_edge=True) * w).max() > 1e-6      # the planted c_k is not the pinv


@pytest.mark.parametrize('name', [n for n in C.NAMES if n.endswith('tone')])
def test_restatement_round_trip_and_falling_inconsistency(name):
    case = C.BY_NAME[name]
    g, x = case.geom, C.audio_of(case)
    spec = R.transform(x, g)
    assert spec.shape == (1, case.F, 2 * g.cut)
    assert R.row_error(R.inverse(spec, g)[:, :case.n], x) <= 1e-6           # float32 tables: their rounding, nothing else
    S = C.target_of(name)
    inc = [R.inconsistency(R.griffin_lim(S, g, k)[:, :case.n], S, g) for k in range(0, 13, 3)]
    assert all(b <= a * (1 + 1e-9) for a, b in zip(inc, inc[1:])), inc
    assert inc[-1] < 0.7 * inc[0]


def test_phase_check_leaves_out_few_bins():
    for name in C.NAMES:
        case = C.BY_NAME[name]
        if case.signal in ('tone', 'full'):
            m = R.polar(R.transform(C.audio_of(case), case.geom), case.geom)[0]
            assert 1.0 - (m >= C.PHASE_FLOOR * m.max(axis=-1, keepdims=True)).mean() <= C.PHASE_LEFT_OUT, name


# ---- bounds ------------------------------------------------------------------------------------------------------------
def _worst(plant=None, dtype=np.float32, names=C.NAMES):
    worst = {}
    for name in names:
        for m in C.MOMENTA:
            for init in (None, C.init_of(name)):
                errs = C.stage_errors(name, m, init, C.numpy_runner(name, m, init, dtype, plant))
                for s, e in errs.items():
                    worst[s] = max(worst.get(s, 0.0), e)
    return worst


def _inverse_distances(plant=None, dtype=np.float32, names=C.NAMES):
    """(inverse, roundtrip): the inverse of the float32 transform's planes against float64 on the same planes, and against
    the signal."""
    wi = wr = 0.0
    for name in names:
        case = C.case_of(name)
        g, x = case.geom, C.audio_of(case)
        spec = R.transform(x, g, np.float32)
        got = R.inverse(spec, g, None, dtype, plant)
        wi = max(wi, R.row_error(got, R.inverse(spec.astype(np.float64), g)))
        wr = max(wr, R.row_error(got[:, :case.n], x))
    return wi, wr


def test_bounds_lie_above_float32():
    worst = _worst()
    worst['inverse'], worst['roundtrip'] = _inverse_distances()
    print('float32 numpy distances', {s: f'{e:.3e}' for s, e in worst.items()})
    for s, e in worst.items():
        assert e <= C.BOUNDS[s] / 5, (s, e, C.BOUNDS[s])             # the bounds are ten times these, rounded


def test_target_bound():
    """The log-mel target max(0, exp(mel) . Minv): BOUNDS['target'] lies above the float32 numpy copy's distance from float64
    (the bound is ten times it) and a factor ten below the planted mistakes -- the clamp missing, the filterbank used for its
    inverse."""
    x, W, Minv = C.log_mel_case()
    g = R.GEOMS[3]
    mag = R.polar(R.transform(x, g), g)[0]
    mel = np.log(np.maximum(mag @ W.T, 1e-5)).astype(np.float32)            # what TacotronSTFT(audio) returns
    want = R.mel_target(mel, Minv)
    d = R.target_error(R.mel_target(mel, Minv.astype(np.float32), np.float32), want)
    print(f'float32 numpy target {d:.3e}')
    assert C.BOUNDS['target'] / 12 <= d <= C.BOUNDS['target'] / 8
    for plant, got in (('no_clamp', R.mel_target(mel, Minv, plant='no_clamp')), ('filterbank', R.mel_target(mel, W))):
        effect = R.target_error(got, want)
        print(plant, f'effect {effect:.3e}')
        assert effect >= 10 * C.BOUNDS['target'], plant


# which stage a planted mistake first shows in, and on which cases it can show at all
_SHOWS = {
    'no_window': 'frames', 'ck_edge': 'frames', 'imag_sign': 'frames',
    'ws_from_w': 'signal', 'no_scale': 'signal', 'trim_off_by_one': 'signal', 'reflect_off_by_one': 'signal',
    'p00_zero': 'phasor', 'momentum_from_c': 'phasor',
}
_LOUD = tuple(n for n in C.NAMES if not n.endswith('silence') and '_f63_' not in n and '_f64_' not in n)


@pytest.mark.parametrize('plant', sorted(_SHOWS))
def test_bounds_lie_below_planted_mistakes(plant):
    """The smallest effect of a mistake over the cases it can show on (float64 loop with the mistake, judged like a GPU run)
    is at least ten times the stage's bound."""
    stage = _SHOWS[plant]
    names = tuple(n for n in C.NAMES if n.endswith('silence')) if plant == 'p00_zero' else _LOUD
    if plant == 'reflect_off_by_one':               # an impulse leaves the rows' ends silent: nothing to reflect
        names = tuple(n for n in _LOUD if not n.endswith('impulse'))
    effects = []
    for name in names:
        for m in (C.MOMENTA if plant != 'momentum_from_c' else (0.99,)):
            init = C.init_of(name)
            errs = C.stage_errors(name, m, init, C.numpy_runner(name, m, init, np.float64, plant))
            effects.append((errs[stage], name, m))
    weakest = min(effects)
    print(plant, 'weakest effect', weakest)
    assert weakest[0] >= 10 * C.BOUNDS[stage], weakest


@pytest.mark.parametrize('plant', ['no_window', 'ws_from_w', 'no_scale', 'trim_off_by_one', 'ck_edge', 'imag_sign'])
def test_inverse_bound_lies_below_planted_mistakes(plant):
    effects = []
    for name in _LOUD:
        case = C.BY_NAME[name]
        g = case.geom
        spec = R.transform(C.audio_of(case), g)
        effects.append((R.row_error(R.inverse(spec, g, plant=plant), R.inverse(spec, g)), name))
    print(plant, 'weakest effect', min(effects))
    assert min(effects)[0] >= 10 * C.BOUNDS['inverse'] and min(effects)[0] >= 10 * C.BOUNDS['roundtrip']


def test_a_neighbours_frame_count_shows_in_a_ragged_overlap_add():
    for g in R.GEOMS[:3]:
        F = 9
        rng = np.random.default_rng(3)
        spec = rng.standard_normal((2, F, 2 * g.cut))
        frames = [F // 2, F]
        good, bad = R.inverse(spec, g, frames), R.inverse(spec, g, frames, plant='neighbour_frames')
        assert R.row_error(bad, good) >= 10 * C.BOUNDS['inverse']


@pytest.mark.parametrize('name', C.E2E)
def test_end_to_end_bounds(name):
    """Ten times the float32 numpy loop's distance from the float64 loop."""
    case = C.BY_NAME[name]
    S = C.target_of(name)
    d = R.row_error(R.griffin_lim(S, case.geom, C.E2E_ITERS, dtype=np.float32), R.griffin_lim(S, case.geom, C.E2E_ITERS))
    print(name, f'float32 loop {d:.3e}')
    assert C.E2E_BOUNDS[name] / 12 <= d <= C.E2E_BOUNDS[name] / 8


# ---- the second table: gapped, sparse, long ------------------------------------------------------------------------------
_EXTRA = sorted(C.EXTRA_GEOMS)


def _extra_names(gname, loud=False):
    """The cases of a geometry; loud: without the ones whose spectrum is all zero (gapped's impulse falls on a sample whose
    window is 0 in the one frame that covers it: the plan sees silence)."""
    names = tuple(n for n in C.EXTRA_NAMES if C.geom_name(n) == gname)
    return tuple(n for n in names if np.abs(C.target_of(n)).max() > 0) if loud else names


@pytest.mark.parametrize('gname', _EXTRA)
def test_extra_geometries_meet_their_preconditions(gname):
    """On the reference alone: stft_inv_check takes F, the plan gives samples(F) samples F frames, and the samples no window
    covers exist on gapped and sparse (with a summed squared window of exactly 0) and not on long."""
    g, F, signals = C.EXTRA_GEOMS[gname]
    assert g.samples(F) > g.half and g.frames(g.samples(F)) == F
    assert g.wl <= g.fl and (gname != 'sparse' or (g.hop > g.fl and g.hop % 4 == 0)) and (gname != 'long' or g.fl > 1024)
    bare = C.uncovered(g, F)
    w2 = R.tables(g)[2].astype(np.float64)
    ws = np.zeros(g.hop * (F - 1) + g.fl)
    for f in range(F):
        ws[f * g.hop:f * g.hop + g.fl] += w2
    kept = ws[g.half:g.half + g.samples(F)]
    assert np.array_equal(kept <= R.FLT_MIN, bare) and (kept[bare] == 0).all()         # the float32 table agrees, and it is 0
    print(gname, 'samples', g.samples(F), 'of them uncovered', int(bare.sum()))
    assert bare.sum() == {'gapped': g.samples(F) // 4, 'sparse': 36, 'long': 0}[gname]
    for name in _extra_names(gname):
        case = C.case_of(name)
        x = C.audio_of(case)
        back = R.inverse(R.transform(x, g), g)
        assert (back[0, :case.n][bare] == 0).all()
        assert R.row_error(back[:, :case.n][:, ~bare], x[:, ~bare]) <= 1e-5       # float32 tables, over sparse's window edge
    assert _extra_names(gname, loud=True) == tuple(n for n in _extra_names(gname) if n != 'gapped_f9_impulse')


@pytest.mark.parametrize('gname', _EXTRA)
def test_extra_bounds_lie_above_float32(gname):
    names = _extra_names(gname)
    worst = _worst(names=names)
    worst['inverse'], worst['roundtrip'] = _inverse_distances(names=names)
    bounds = C.EXTRA_BOUNDS[gname]
    print(gname, 'float32 numpy distances', {s: f'{e:.3e}' for s, e in worst.items()}, 'bounds', bounds)
    assert ('roundtrip' in bounds) == (gname == 'long') and sorted(set(worst) - {'roundtrip'}) == sorted(set(bounds) - {'roundtrip'})
    for s, b in bounds.items():
        if s == 'spectrum':                                     # the forward plan's own bound
            assert worst[s] <= b / 5
        elif b == 0:
            assert worst[s] == 0
        else:
            assert b / 12 <= worst[s] <= b / 8, (s, worst[s], b)    # ten times it, rounded up to two digits


# ck_edge changes the last bin alone: it cannot show on long's tone, whose last bin holds under 0.4 % of a frame's largest magnitude
_EXTRA_CANNOT_SHOW = {'ck_edge': ('long_f9_tone',)}


@pytest.mark.parametrize('plant', sorted(_SHOWS))
@pytest.mark.parametrize('gname', _EXTRA)
def test_extra_bounds_lie_below_planted_mistakes(gname, plant):
    """As test_bounds_lie_below_planted_mistakes.  P(0, 0) = 0 shows in the phase update where the spectrum is silent (gapped's
    impulse); on every other case it shows in the first operand, through the zeros of `init`, and is held against that bound."""
    bounds = C.EXTRA_BOUNDS[gname]
    loud = tuple(n for n in _extra_names(gname, loud=True) if n not in _EXTRA_CANNOT_SHOW.get(plant, ()))
    silent = tuple(n for n in _extra_names(gname) if n not in _extra_names(gname, loud=True))
    if plant == 'reflect_off_by_one':
        loud = tuple(n for n in loud if not n.endswith('impulse'))
    groups = [('phasor', silent), ('operand', loud)] if plant == 'p00_zero' else [(_SHOWS[plant], loud)]
    for stage, names in groups:
        effects = []
        for name in names:
            for m in (C.MOMENTA if plant != 'momentum_from_c' else (0.99,)):
                init = C.init_of(name)
                errs = C.stage_errors(name, m, init, C.numpy_runner(name, m, init, np.float64, plant))
                effects.append((errs[stage], name, m))
        if effects:
            print(gname, plant, stage, 'weakest effect', min(effects))
            assert min(effects)[0] >= 10 * bounds[stage] and min(effects)[0] > 0, min(effects)
    assert loud


@pytest.mark.parametrize('plant', ['no_window', 'ws_from_w', 'no_scale', 'trim_off_by_one', 'ck_edge', 'imag_sign'])
@pytest.mark.parametrize('gname', _EXTRA)
def test_extra_inverse_bound_lies_below_planted_mistakes(gname, plant):
    effects = []
    for name in _extra_names(gname, loud=True):
        case = C.case_of(name)
        g = case.geom
        spec = R.transform(C.audio_of(case), g)
        effects.append((R.row_error(R.inverse(spec, g, plant=plant), R.inverse(spec, g)), name))
    print(gname, plant, 'weakest effect', min(effects))
    assert min(effects)[0] >= 10 * max(C.EXTRA_BOUNDS[gname]['inverse'], C.EXTRA_BOUNDS[gname].get('roundtrip', 0.0))


@pytest.mark.parametrize('name', sorted(C.LOG_MEL_PLANS))
def test_log_mel_plans(name):
    """The plans of the ragged log-mel test: no channel is empty and the filterbank has full rank (the plan's own inverse
    exists), every row passes stft_inv_check, and BOUNDS['target'] lies ten times above the float32 numpy copy's distance
    from float64 on every row."""
    g, mel, W, Minv = C.log_mel_rows(name)
    n_mel = C.LOG_MEL_PLANS[name][3]
    assert W.shape == (n_mel, g.cut) and (W.max(axis=1) > 0).all() and np.linalg.matrix_rank(W) == n_mel
    assert g.frames(g.samples(C.LOG_MEL_F)) == C.LOG_MEL_F
    assert {'mel8': 32, 'mel32': 32, 'mel80': 96}[name] == ceil_div(n_mel, 32) * 32
    for b, Fb in enumerate(C.LOG_MEL_FRAMES):
        assert g.samples(Fb) > g.half and np.isnan(mel[b, Fb:]).all() and np.isfinite(mel[b, :Fb]).all()
        want = R.mel_target(mel[b:b + 1, :Fb], Minv)
        d = R.target_error(R.mel_target(mel[b:b + 1, :Fb], Minv.astype(np.float32), np.float32), want)
        print(name, b, f'float32 numpy target {d:.3e}')
        assert d <= C.BOUNDS['target'] / 10 and want.max() > 0
        assert R.target_error(R.mel_target(mel[b:b + 1, :Fb], W), want) >= 10 * C.BOUNDS['target']


def test_phasor_at_the_ends_of_the_float_range():
    """The restatement on the pairs the GPU test feeds `init`: unit length, the direction of the pair, (1, 0) at the origin."""
    pairs = C.phasor_pairs().astype(np.float64)
    pr, pi = R.phasor(pairs[:, 0], pairs[:, 1])
    assert np.isfinite(pr).all() and np.isfinite(pi).all() and np.abs(np.hypot(pr, pi) - 1).max() <= 1e-15
    origin = (pairs == 0).all(axis=1)
    assert origin.sum() == 2 and (pr[origin] == 1).all() and (pi[origin] == 0).all()
    ang = np.arctan2(pairs[~origin, 1], pairs[~origin, 0])
    assert np.abs(pr[~origin] - np.cos(ang)).max() <= 1e-15 and np.abs(pi[~origin] - np.sin(ang)).max() <= 1e-15


# ---- the front end, as a stand-alone program under ASan / UBSan ----------------------------------------------------------
def _plan(fl=16, hop=4, wl=16, **more):
    return dict(filter_length=fl, hop_length=hop, win_length=wl, n_mel_channels=1, mel_fmax=11025, **more)


def geometry(g, B, F, frames, kind, n_mel=1, what=-1):
    cut, fl = g.cut, g.fl
    K4, Kpad, NB, EK = ceil_div(fl, 4) * 4, ceil_div(fl, 32) * 32, ceil_div(2 * cut, 32) * 32, ceil_div(n_mel, 32) * 32
    gl, rows = kind >= 0, B * F
    PW = g.hop * (F - 1) + fl
    NP = ceil_div(PW + K4 - fl, 4) * 4
    slices = [4 * B, rows * cut * 4 if gl else 0, rows * NB * 4, rows * NB * 4 if gl else 0, rows * NB * 4 if what == 5 else 0,
              rows * fl * 4, B * NP * 4 + 256 if gl else 0, rows * Kpad * 4 if gl and g.hop % 4 else 0, rows * NB * 4 if gl else 0,
              rows * EK * 4 if kind == 1 else 0, cut * EK * 4 if kind == 1 else 0]
    offs = [carved(*slices[:i]) for i in range(len(slices))]
    return [[PW, NP, EK, F * g.hop, carved(*slices)], offs, [g.samples(f) for f in frames or [F] * B]]


@pytest.mark.parametrize('g', R.GEOMS)
def test_geometry(checker, g):
    s = _plan(g.fl, g.hop, g.wl)
    F = 20
    assert _accepted(checker, 'stft_inv', B=2, F=F, C=g.cut, input_kind=-1, **s) == geometry(g, 2, F, None, -1)
    assert _accepted(checker, 'stft_inv', [1, 2, F], F=F, C=g.cut, input_kind=-1, **s) == geometry(g, 3, F, [1, 2, F], -1)
    assert _accepted(checker, 'stft_inv', [F - 1, F], F=F, C=g.cut, n_iters=3, momentum=0.99, **s) == geometry(g, 2, F, [F - 1, F], 0)
    assert _accepted(checker, 'stft_inv', B=1, F=F, C=g.cut, n_iters=3, what=5, k=2, **s) == geometry(g, 1, F, None, 0, what=5)
    mel = dict(s, n_mel_channels=40, mel_fmax=8000)
    assert _accepted(checker, 'stft_inv', B=2, F=F, C=40, input_kind=1, **mel) == geometry(g, 2, F, None, 1, n_mel=40)


@pytest.mark.parametrize('gname', sorted(C.EXTRA_GEOMS))
def test_geometry_on_the_extra_plans(checker, gname):
    """hop > filter_length and filter_length = 2048 through the same stand-alone sweep."""
    test_geometry(checker, C.EXTRA_GEOMS[gname][0])


OK = dict(B=2, F=9, C=9, n_iters=3, momentum=0.5, **_plan())
REFUSALS = [
    # (frames, settings, substrings of the message), in the documented order
    ((), dict(OK, null='audio'), ['NULL pointer']),
    ((), dict(OK, null='out'), ['NULL pointer']),
    ((), dict(OK, null='fn'), ['NULL pointer']),
    ((), dict(OK, B=0), ['B = 0, F = 9: both must be >= 1']),
    ((), dict(OK, F=0), ['B = 2, F = 0']),
    ((9, 0), OK, ['frames[1] = 0 outside [1, F = 9]']),
    ((10, 9), OK, ['frames[0] = 10 outside [1, F = 9]']),
    ((), dict(OK, input_kind=2), ['input_kind 2']),
    ((), dict(OK, C=8), ["C = 8, but the plan's bins is 9"]),
    ((), dict(OK, C=9, input_kind=1), ["C = 9, but the plan's n_mel_channels is 1"]),
    ((), dict(OK, n_iters=-1), ['n_iters = -1 < 0']),
    ((), dict(OK, momentum=1), ['momentum = 1 outside [0, 1)']),
    ((), dict(OK, momentum=-0.5), ['momentum = -0.5 outside']),
    ((), dict(OK, momentum='nan'), ['momentum']),
    ((), dict(OK, mel_kind=1), ['Whisper']),
    ((), dict(OK, pre_emph=0.97), ['pre_emph = 0.97 > 0']),
    ((), dict(OK, input_kind=1, C=1, normalize_mode=1), ['normalize_mode 1 is not invertible']),
    ((9, 3), OK, ['row 1: 3 frames give 8 samples, not more than filter_length // 2 = 8']),
    ((), dict(OK, B=65536), ['too large']),
    ((), dict(OK, B=3, F=15000000), ['too large for 31-bit offsets']),
    ((), dict(OK, mem=2), ['bad mem kind 2']),
    ((), dict(OK, what=6, k=0), ['no stage 6 (0 .. 5)']),
    ((), dict(OK, what=1, k=4), ['k = 4 outside [0, n_iters = 3]']),
    ((), dict(OK, what=1, k=-1), ['k = -1 outside']),
    ((), dict(OK, what=4, k=3), ['ends at its signal']),
]


@pytest.mark.parametrize('frames,settings,needles', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals(checker, frames, settings, needles):
    _refused(checker, 'stft_inv', needles, frames, **settings)


def test_first_match_wins(checker):
    both = dict(OK, B=0, n_iters=-1, momentum=2, mel_kind=1)
    assert 'both must be' in _refused(checker, 'stft_inv', [], (), **both)
    assert 'n_iters' in _refused(checker, 'stft_inv', [], (), **dict(both, B=2))
    assert 'momentum' in _refused(checker, 'stft_inv', [], (), **dict(both, B=2, n_iters=0))
    assert 'Whisper' in _refused(checker, 'stft_inv', [], (), **dict(both, B=2, n_iters=0, momentum=0))
    # the inverse alone has neither a loop nor a reflect: one frame is a row, pre-emphasis does not matter
    assert _accepted(checker, 'stft_inv', [1, 1], F=9, C=9, input_kind=-1, n_iters=-1, momentum=7, **_plan(pre_emph=0.97))


def _minv(exe, **settings):
    args = [exe, '--audio-call', 'stft_inv', 'minv=1', 'B=1', 'F=40', 'input_kind=1'] + [f'{k}={v}' for k, v in settings.items()]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0].strip() == '0', lines[0]
    ok = int(lines[4])
    return ok, np.array([float(v) for v in lines[5:]])


def test_cholesky_mel_inverse(checker):
    ok, vals = _minv(checker, C=80, n_mel_channels=80)
    W = R.slaney_filterbank(22050, 1024, 80, 0.0, 8000.0)
    assert ok == 1 and vals.size == W.size
    assert np.abs(vals.reshape(W.shape) - np.linalg.pinv(W).T).max() <= 1e-9
    # the restated filterbank is the oracle's (float32) one
    from oracle import mel_stft_ref
    assert np.abs(W - mel_stft_ref.mel_filterbank(22050, 1024, 80, 0.0, 8000.0)).max() <= 1e-7
    ok, vals = _minv(checker, C=128, n_mel_channels=128, filter_length=64, win_length=64, hop_length=16)
    assert ok == 0 and vals.size == 0                                    # a channel without a bin


# ---- the objects ---------------------------------------------------------------------------------------------------------
def test_configs_have_the_references_keys_and_defaults():
    from text_to_speech_amd.stft import STFT, TacotronSTFT
    assert STFT().get_config() == {'filter_length': 800, 'hop_length': 200, 'win_length': 800, 'window': 'hann',
                                   'to_magnitude': True, 'periodic': True}
    assert list(STFT(64, 16, 48, None, False, False).get_config().values()) == [64, 16, 48, None, False, False]
    cfg = TacotronSTFT().get_config()
    assert cfg == {'class_name': 'TacotronSTFT', 'n_mel_channels': 80, 'sampling_rate': 22050, 'win_length': 1024,
                   'hop_length': 256, 'filter_length': 1024, 'mel_fmin': 0.0, 'mel_fmax': 8000.0, 'pre_emph': 0.,
                   'normalize_mode': None, 'window': 'hann', 'to_magnitude': True, 'periodic': True}
    fn = TacotronSTFT(filter_length=64, hop_length=16, win_length=48, window='hamming', periodic=False).stft_fn
    assert isinstance(fn, STFT) and fn.get_config() == {'filter_length': 64, 'hop_length': 16, 'win_length': 48,
                                                        'window': 'hamming', 'to_magnitude': True, 'periodic': False}
    assert np.array_equal(STFT(8, 2, 6, window=None).fft_window(), np.ones(6))
    with pytest.raises(RuntimeError, match='no engine'):
        STFT()(np.zeros(2000, np.float32))
    with pytest.raises(ValueError):
        STFT(filter_length=16, win_length=32)


class _Recorder:
    """An engine stub that records what GriffinLim asks of it."""

    def __init__(self):
        self.calls = []

    def mel_fn(self, config, window=None):
        self.calls.append(('mel_fn', dict(config), window))
        return 'plan'

    def random_normal_rows(self, row_stride, keys, offsets=None, counts=None, stream=None, out=None):
        self.calls.append(('random_normal_rows', row_stride, list(keys), offsets))

        class _T:
            def view(self_, *shape):
                return ('init', shape)
        return _T()

    def griffin_lim(self, plan, spec, **kw):
        self.calls.append(('griffin_lim', plan, spec.shape, kw))
        B, F = (1, spec.shape[0]) if spec.ndim == 2 else spec.shape[:2]
        return np.zeros((B, F * 256), np.float32)


def test_griffin_lim_obeys_the_vocoder_contract():
    from text_to_speech_amd.griffin_lim import GriffinLim
    from text_to_speech_amd.runtime import stream_key
    from text_to_speech_amd.stft import PHASE_STREAM
    eng = _Recorder()
    voc = GriffinLim(eng, n_iters=7, momentum=0.5)
    assert voc.compiled_infer.engine is eng and voc.rate == 22050
    mel = np.zeros((3, 11, 80), np.float32)
    out = voc(mel, lengths=[11, 4, 9], streams=[(5, 0), (5, 1), (6, 0)], packed=True, sigma=0.6, precision='f16')   # ignored keywords
    assert out.shape == (3, 11 * 256)
    name, plan, shape, kw = eng.calls[-1]
    assert (name, plan, shape) == ('griffin_lim', 'plan', (3, 11, 80))
    assert kw['frames'] == [11, 4, 9] and kw['kind'] == 'log_mel' and kw['n_iters'] == 7 and kw['momentum'] == 0.5 and kw['init'] is None
    assert eng.calls[0][1]['filter_length'] == 1024 and eng.calls[0][1]['kind'] == 'tacotron'
    assert voc.infer(mel[0]).shape == (1, 11 * 256)
    # seeded: one stream per row, keyed by what the row is
    eng.calls.clear()
    seeded = GriffinLim(eng, seed=42)

    class _Cuda(np.ndarray):
        is_cuda = True
    seeded(mel.view(_Cuda), streams=[(5, 0), (5, 1), (6, 0)])
    rnd = [c for c in eng.calls if c[0] == 'random_normal_rows'][0]
    assert rnd[1] == 11 * 513 * 2 and rnd[2] == [stream_key(42, PHASE_STREAM, u, p) for u, p in ((5, 0), (5, 1), (6, 0))]
    assert eng.calls[-1][3]['init'] == ('init', (3, 11, 513, 2))


def test_get_models_takes_griffin_lim_without_changing_the_default_key(monkeypatch):
    import inspect
    from types import SimpleNamespace
    from text_to_speech_amd import runtime, tacotron2
    from text_to_speech_amd.griffin_lim import GriffinLim
    sig = inspect.signature(tacotron2.get_models)
    assert sig.parameters['vocoder'].default is None
    with pytest.raises(ValueError, match='griffin_lim'):
        tacotron2.get_models(vocoder='hifigan')
    with pytest.raises(ValueError, match='overlap'):
        tacotron2.get_models(vocoder='griffin_lim', overlap=True)
    built = []

    def fake_runtime(kind, path, model=None, engine=None, **kw):
        built.append(model)
        return SimpleNamespace(engine=engine or _Recorder(), model=model)

    monkeypatch.setattr(runtime, 'build_runtime', fake_runtime)
    monkeypatch.setattr(tacotron2, '_models', {})
    m, v = tacotron2.get_models('p', 0, 'en', vocoder='griffin_lim')
    assert built == ['tacotron2'] and isinstance(v, GriffinLim) and v.compiled_infer.engine is m.compiled_infer.engine
    assert list(tacotron2._models) == [('p', 0, 'en', False, 0, 'griffin_lim')]
    assert tacotron2.get_models('p', 0, 'en', vocoder='griffin_lim') == (m, v) and built == ['tacotron2']
    m2, v2 = tacotron2.get_models('p', 0, 'en')                       # the default pair keeps its key and builds WaveGlow
    assert built == ['tacotron2', 'tacotron2', 'waveglow'] and ('p', 0, 'en', False, 0) in tacotron2._models and m2 is not m
    # beside a caller's model the named vocoder sits on that model's engine and nothing is built or cached
    own = tacotron2._named_vocoder(m2, 'griffin_lim')
    assert isinstance(own, GriffinLim) and own.compiled_infer.engine is m2.compiled_infer.engine and len(built) == 3
    assert tacotron2._named_vocoder(None, 'griffin_lim') == 'griffin_lim' and tacotron2._named_vocoder(m2, v2) is v2
