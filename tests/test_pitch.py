"""CPU: the pitch calls' restatement, bounds, front end and bindings (no GPU).

1. tests/pitch_ref.py against closed forms: a sine of integer period P under a window that is a multiple of P has
   d(tau) = W A^2 (1 - cos 2 pi tau / P) on interior frames; silence and DC are unvoiced with d' = 1; the +-1 square wave has
   d(P) = d(2P) = 0 exactly and takes the smaller lag.
2. The cases: at least 90 % of all case frames are STABLE (pitch_ref.stable) -- a condition on the inputs, not a tolerance.
3. The bounds of tests/test_pitch_gpu.py: a float32 numpy copy of each stage lies inside them, and every planted mistake
   (pitch_ref.MISTAKES) moves its stage by at least ten times its bound.  F0_END_TO_END, the bound of f0 against the all-float64
   restatement on STABLE voiced frames of the two sines, is a factor ten above what the float32 copy is measured at here (6.3e-7
   relative, 10.5 units of 2^-24, on the 'ragged' integer-period sine) and a factor ten below the weakest of the mistakes that
   reach f0 (delta taken on d: 2.4e-3).
4. The front end (csrc/pitch_call.h) as a stand-alone program under ASan / UBSan against a Python restatement: every refusal,
   pairs of faults in the documented order, the limits at and one above.
5. The Python calls on the recording engine of tests/test_engine_calls.py; bad arguments raise before any library call.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pitch_cases as pc
import pitch_ref as pr
from test_engine_calls import run as record_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
EINVAL = -1
F0_END_TO_END = 6.3e-6               # relative; measured 6.3e-7 for the float32 copy (see 3. above)

CASES = pc.cases()
DEFAULT = dict(rate=22050, hop=256, win=1024, tau_min=45, tau_max=367, threshold=0.1)


# ---- 1. closed forms ------------------------------------------------------------------------------------------------------------
def test_difference_of_a_sine_is_its_closed_form():
    P, W, A, n = 100, 1000, 0.5, 6000
    cfg = dict(DEFAULT, win=W, hop=250)
    x = A * np.sin(2 * np.pi * np.arange(n) / P + 0.7)
    r = pr.track(x, n, **cfg)
    s = np.arange(len(r['d'])) * 250 - W // 2
    inside = (s >= 0) & (s + W + cfg['tau_max'] <= n)
    assert inside.sum() >= 15
    want = W * A * A * (1 - np.cos(2 * np.pi * np.arange(cfg['tau_max'] + 1) / P))
    assert np.abs(r['d'][inside] - want).max() <= 1e-11 * want.max()
    assert np.all(r['voiced'][inside]) and np.all(r['tau'][inside] == P)
    assert np.abs(r['f0'][inside] - 22050 / P).max() < 0.05 and np.all(r['aperiodicity'][inside] < 1e-9)


def test_silence_dc_and_the_square_wave():
    for x in (np.zeros(3000), np.full(3000, 0.3)):
        r = pr.track(x, 3000, **DEFAULT)
        inner = slice(2, 7)                                          # frames that hang over an end of a DC row see its edge
        assert np.all(r['d'][inner] == 0) and np.all(r['dp'][inner] == 1)
        assert not r['voiced'][inner].any() and np.all(r['tau'][inner] == 45)
        assert np.all(r['f0'][inner] == 0) and np.all(r['period'][inner] == 45) and np.all(r['aperiodicity'][inner] == 1)
    r = {k: v[2:21] for k, v in pr.track(pc.signal('square', 6000, 100), 6000, **DEFAULT).items()}      # the frames inside the row
    assert np.all(r['d'][:, [100, 200, 300]] == 0) and np.all(r['voiced']) and np.all(r['tau'] == 100)
    assert np.all(r['aperiodicity'] == 0)


def test_pick_rule_on_hand_made_curves():
    q = np.ones((1, 12))
    q[0, 5:9] = [0.3, 0.09, 0.05, 0.07]                              # crosses at 6, walks to 7
    assert [v.tolist() for v in pr.pick(q, 2, 11, 0.1)] == [[True], [7]]
    assert [v.tolist() for v in pr.pick(q, 8, 11, 0.1)] == [[True], [8]]          # the walk stops where the curve rises
    q[0, 5:9] = [0.3, 0.2, 0.2, 0.4]                                 # nothing below: the argmin, the smaller lag of the tie
    assert [v.tolist() for v in pr.pick(q, 2, 11, 0.1)] == [[False], [6]]
    f0, period, ap = pr.planes(np.array([[1, 1, .5, .2, .1, .3, 1]]), [True], [4], 100, 6)
    assert period[0] == 4 + (0.2 - 0.3) / (2 * (0.2 - 0.2 + 0.3)) and f0[0] == 100 / period[0] and ap[0] == 0.1
    f0, period, _ = pr.planes(np.array([[1, .1, .5, .2, .1, .3, .05]]), [True, ], [6], 100, 6)     # a neighbour outside: no delta
    assert period[0] == 6
    f0, period, _ = pr.planes(np.array([[1, .1, .5, .2, .1, .3, .05]]), [False], [1], 100, 6)
    assert period[0] == 1 and f0[0] == 0


# ---- 2. the cases ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def refs():
    """(case, row) -> the float64 restatement and its STABLE frames"""
    out = {}
    for name, c in CASES.items():
        for b, kind in enumerate(c['kinds']):
            r = pr.track(c['audio'][b], int(c['lengths'][b]), **c['cfg'])
            r['stable'] = pr.stable(r['d'], r['dp'], c['cfg']['tau_min'], c['cfg']['tau_max'], c['cfg']['threshold'])
            out[name, b] = r
    return out


def test_cases_cover_the_shapes_and_nine_frames_in_ten_are_stable(refs):
    assert set(pc.KINDS) == set(CASES['default']['kinds'])
    assert CASES['small']['lengths'].tolist() == [1, 15, 16, 17, 63, 64, 65, 500]
    assert [(c['cfg']['win'], c['cfg']['hop'], c['cfg']['tau_min'], c['cfg']['tau_max']) for c in (CASES[n] for n in ('small', 'default', 'limits', 'odd'))] == [
        (64, 16, 2, 40), (1024, 256, 45, 367), (2048, 2048, 1, 1024), (202, 50, 3, 300)]
    assert len(refs['limits', 0]['d']) == 3 and len(CASES['ragged']['kinds']) == 5
    on = refs['on_threshold', 0]                                     # silence at threshold 1: d' = 1 is not below it
    assert CASES['on_threshold']['cfg']['threshold'] == 1.0 and np.all(on['dp'] == 1) and not on['voiced'].any() and np.all(on['tau'] == 2)
    assert pr.pick(on['dp'], 2, 40, 1.0, 'threshold_le')[0].all()
    dc = refs['on_threshold', 1]
    assert np.all(dc['dp'][2] == 1) and not dc['voiced'][2] and dc['tau'][2] == 2      # the frame inside the DC row
    for name in ('small', 'ragged'):
        c = CASES[name]
        assert all(np.isnan(c['audio'][b, n:]).all() and np.isfinite(c['audio'][b, :n]).all() for b, n in enumerate(c['lengths']))
    total = sum(len(r['stable']) for r in refs.values())
    good = sum(int(r['stable'].sum()) for r in refs.values())
    print(f'STABLE: {good} of {total} frames')
    assert good >= 0.9 * total, (good, total)
    for kind in ('sine_int', 'sine_frac', 'missing_fundamental', 'vibrato', 'tone_noise', 'square', 'full_scale'):
        assert refs['default', pc.KINDS.index(kind)]['voiced'][2:-2].all(), kind
    for kind in ('noise', 'zeros', 'dc'):
        assert not refs['default', pc.KINDS.index(kind)]['voiced'][2:-2].any(), kind
    mf = refs['default', pc.KINDS.index('missing_fundamental')]      # the period of the absent fundamental, not of a harmonic
    assert np.all(np.abs(mf['period'][2:-2] - 103.37) < 0.5)


# ---- 3. the bounds --------------------------------------------------------------------------------------------------------------
def _float32_stages(c, b):
    cfg = c['cfg']
    fr = pr.frames(c['audio'][b], int(c['lengths'][b]), cfg['hop'], cfg['win'], cfg['tau_max']).astype(np.float32)
    d = np.empty((len(fr), cfg['tau_max'] + 1), np.float32)
    for tau in range(cfg['tau_max'] + 1):
        d[:, tau] = np.cumsum((fr[:, :cfg['win']] - fr[:, tau:tau + cfg['win']]) ** 2, axis=1, dtype=np.float32)[:, -1]
    S = np.concatenate([np.zeros((len(d), 1), np.float32), np.cumsum(d[:, 1:], axis=1, dtype=np.float32)], axis=1)
    dp = np.where(S == 0, np.float32(1), d * np.arange(d.shape[1], dtype=np.float32) / np.where(S == 0, np.float32(1), S)).astype(np.float32)
    dp[:, 0] = 1
    return d, dp


@pytest.mark.parametrize('name', sorted(CASES))
def test_float32_copy_of_the_restatement_is_inside_every_gpu_bound(refs, name):
    c = CASES[name]
    for b in range(len(c['kinds'])):
        d, dp = _float32_stages(c, b)
        ref = refs[name, b]
        assert np.all(np.abs(d - ref['d']) <= pr.bound_d(ref['d'], c['cfg']['win'])), (name, b)
        want = pr.cmnd(d)
        assert np.all(np.abs(dp - want) <= pr.bound_cmnd(want)), (name, b)


def _sine_frames(refs):
    for (name, b), r in refs.items():
        if CASES[name]['kinds'][b] in ('sine_int', 'sine_frac'):
            sel = r['stable'] & r['voiced']
            if sel.any():
                yield name, b, r, sel


def test_f0_end_to_end_bound_is_ten_times_the_float32_copy(refs):
    worst = 0.0
    for name, b, r, sel in _sine_frames(refs):
        c = CASES[name]
        r32 = pr.track32(c['audio'][b], int(c['lengths'][b]), **c['cfg'])
        assert np.array_equal(r32['tau'][sel], r['tau'][sel]) and r32['voiced'][sel].all()
        worst = max(worst, float((np.abs(r32['f0'][sel] - r['f0'][sel]) / r['f0'][sel]).max()))
    print(f'float32 copy: f0 within {worst:.3g} relative ({worst / pr.EPS:.1f} EPS) of float64')
    assert 0 < worst <= F0_END_TO_END / 10 * 1.001


def _tracks(seed=3, F=200):
    rng = np.random.default_rng(seed)
    a, b = (120.0 * 2 ** rng.uniform(-0.5, 0.8, F) for _ in range(2))
    a[rng.random(F) < 0.3], b[rng.random(F) < 0.3] = 0.0, 0.0
    path = [(min(t, 149), min(t // 2 + t % 2 * (t > 100), 179)) for t in range(190)]
    return a.astype(np.float32), b.astype(np.float32), path


@pytest.mark.parametrize('mistake', pr.MISTAKES)
def test_gpu_bound_is_a_tenth_of_every_planted_mistake(refs, mistake):
    """The weakest effect of a mistake, over the frames the GPU test compares, in units of that comparison's bound (an exact
    comparison: any change at all)."""
    tones = [(n, b) for (n, b) in refs if CASES[n]['kinds'][b] not in ('zeros', 'dc', 'noise') and n in ('default', 'ragged', 'odd')]
    if mistake in ('window_start', 'read_past_length'):
        effect = 0.0
        for name, b in tones:
            c, ref = CASES[name], refs[name, b]
            n = int(c['lengths'][b])
            if mistake == 'read_past_length':
                if n == c['audio'].shape[1] or name != 'ragged':
                    continue
                x = pc.signal(c['kinds'][b], c['audio'].shape[1], 120, seed=b)           # the row as it goes on behind its length
                assert np.array_equal(x[:n], c['audio'][b, :n])
            else:
                x = c['audio'][b]
            fr = pr.frames(x, n, c['cfg']['hop'], c['cfg']['win'], c['cfg']['tau_max'], mistake)
            d = pr.difference(fr, c['cfg']['win'], c['cfg']['tau_max'])
            bound = pr.bound_d(ref['d'], c['cfg']['win'])
            effect = max(effect, float((np.abs(d - ref['d'])[bound > 0] / bound[bound > 0]).max()))
    elif mistake in ('prefix_shifted', 'no_tau_factor'):
        effect = np.inf
        for name, b in tones:
            ref = refs[name, b]
            bound = pr.bound_cmnd(ref['dp'])[:, 2:]
            moved = np.abs(pr.cmnd(ref['d'], mistake) - ref['dp'])[:, 2:]
            effect = min(effect, float((moved[bound > 0] / bound[bound > 0]).max()))
    elif mistake in ('threshold_le', 'no_walk', 'argmin_last'):
        # compared exactly: the mistake has to change a flag or a lag on some frame the GPU test compares.  There the rule runs on
        # the device's own float32 d'; the frames that show `<=` ('on_threshold': silence and the inside of a DC row, d' = 1 by
        # rule = the threshold) hold the same exact 1 in float32 and float64, the others are looked for among the STABLE frames
        changed = False
        for (name, b), ref in refs.items():
            cfg = CASES[name]['cfg']
            v, t = pr.pick(ref['dp'], cfg['tau_min'], cfg['tau_max'], cfg['threshold'], mistake)
            sel = np.all(ref['d'] == 0, axis=1) if mistake == 'threshold_le' else ref['stable']
            changed |= not (np.array_equal(v[sel], ref['voiced'][sel]) and np.array_equal(t[sel], ref['tau'][sel]))
        effect = np.inf if changed else 0.0
    elif mistake in ('delta_sign', 'delta_on_d', 'no_delta'):
        effect, on_f0 = np.inf, 0.0
        for name, b, r, sel in _sine_frames(refs):
            f0, period, _ = pr.planes(r['dp'], r['voiced'], r['tau'], CASES[name]['cfg']['rate'], CASES[name]['cfg']['tau_max'], r['d'], mistake)
            effect = min(effect, float((np.abs(f0 - r['f0'])[sel] / pr.bound_rounded(r['f0'], 2)[sel]).max()))
            on_f0 = max(on_f0, float((np.abs(f0 - r['f0'])[sel] / r['f0'][sel]).max()))
        print(f'{mistake}: f0 moves by up to {on_f0:.3g} relative')
        assert on_f0 >= 10 * F0_END_TO_END
    else:
        a, b, path = _tracks()
        good, bad = pr.f0_error(a, b, 150, 180, path), pr.f0_error(a, b, 150, 180, path, mistake=mistake)
        if mistake == 'vuv_counts_unvoiced':
            effect = np.inf if bad[4] != good[4] else 0.0             # a count: compared exactly
        else:
            effect = float(abs(bad[2] - good[2]) / pr.bound_rounded(good[2], 4))
    print(f'{mistake}: weakest effect = {effect:.3g} bounds')
    assert effect >= 10


# ---- 4. the front end -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    return os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')


GOOD = dict(B=3, N=6000, rate=22050, hop=256, win=1024, tau_min=45, tau_max=367, threshold=0.1, mem=0, probe=0, what=-1, null='', len=None)
GOOD_F0 = dict(f0=1, B=3, Fa=40, Fb=52, P=91, path=0, gross=315.64, mem=0, null='', la=None, lb=None)
TABLES = ('len', 'la', 'lb')


def _call(exe, s):
    """-> (status, message, the layout numbers or None)"""
    args = [f'{k}={v}' for k, v in s.items() if k != 'null' and k not in TABLES]
    args += [f'{k}=' + ','.join(str(v) for v in s[k]) for k in TABLES if s.get(k) is not None]
    args += [f"null={s['null']}"] if s['null'] else []
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, '--pitch'] + args, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    rc, _, msg = lines[0].partition(' ')
    return int(rc), msg, [int(v) for v in lines[1].split()] if len(lines) > 1 else None


def _out_elems(s):
    BF = s['B'] * (1 + s['N'] // s['hop'])
    return 3 * BF if not s['probe'] else 2 * BF if s['what'] == 2 else BF * (s['tau_max'] + 1)


def pitch_check(s):
    """pitch_check restated -> (status, message)"""
    for name in ('audio', 'out'):
        if name in s['null'].split(','):
            return EINVAL, f'{name} is NULL'
    for name in ('B', 'N', 'rate'):
        if s[name] < 1:
            return EINVAL, f'{name} = {s[name]} must be at least 1'
    if not 1 <= s['hop'] <= s['win']:
        return EINVAL, f"hop = {s['hop']} is outside [1, win = {s['win']}]"
    if not 2 <= s['win'] <= 2048:
        return EINVAL, f"win = {s['win']} is outside [2, 2048]"
    if s['tau_min'] < 1 or s['tau_min'] >= s['tau_max'] or s['tau_max'] > 1024:
        return EINVAL, f"lags [{s['tau_min']}, {s['tau_max']}] must satisfy 1 <= tau_min < tau_max <= 1024"
    thr = np.float32(s['threshold'])
    if not 0 < thr <= 1:
        return EINVAL, f'threshold = {float(thr):g} is outside (0, 1]'
    if s['mem'] not in (0, 1):
        return EINVAL, f"bad mem kind {s['mem']}"
    if s['probe'] and not 0 <= s['what'] <= 2:
        return EINVAL, f"what = {s['what']} is no stage (0 difference, 1 normalised difference, 2 pick)"
    for row, n in enumerate((s['len'] or [])[:s['B']]):
        if not 1 <= n <= s['N']:
            return EINVAL, f"lengths[{row}] = {n} is outside [1, N = {s['N']}]"
    if s['N'] > 1 << 24:
        return EINVAL, f"N = {s['N']}: above {1 << 24} samples"
    if s['B'] * s['N'] * 4 >= 1 << 31:
        return EINVAL, f"audio too large (B = {s['B']}, N = {s['N']}: 2^31 bytes or more); split the batch"
    if _out_elems(s) * 4 >= 1 << 31:
        return EINVAL, f'out too large ({_out_elems(s)} floats: 2^31 bytes or more); split the batch'
    return 0, ''


def _offsets(sizes):
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += (n + 255) // 256 * 256
    return offsets, at


def pitch_layout(s):
    """pitch_layout restated -> [F, threads, lens, in, out, out_elems, bytes]"""
    host = s['mem'] == 0
    offsets, at = _offsets([s['B'] * 4, s['B'] * s['N'] * 4 * host, _out_elems(s) * 4 * host])
    return [1 + s['N'] // s['hop'], (-(-(s['tau_max'] + 1) // 4) + 63) // 64 * 64, *offsets, _out_elems(s), at]


def f0_check(s):
    """f0_error_check restated -> (status, message)"""
    for name in ('f0_a', 'f0_b', 'stats'):
        if name in s['null'].split(','):
            return EINVAL, f'{name} is NULL'
    for name in ('B', 'Fa', 'Fb') + (('P',) if s['path'] else ()):
        if s[name] < 1:
            return EINVAL, f'{name} = {s[name]} must be at least 1'
    g = np.float32(s['gross'])
    if not (np.isfinite(g) and g > 0):
        return EINVAL, f'gross_cents = {float(g):g} must be finite and positive'
    if s['mem'] not in (0, 1):
        return EINVAL, f"bad mem kind {s['mem']}"
    for key, T in (('la', 'Fa'), ('lb', 'Fb')):
        for row, n in enumerate((s[key] or [])[:s['B']]):
            if not 1 <= n <= s[T]:
                return EINVAL, f'len_{key[1]}[{row}] = {n} is outside [1, {T} = {s[T]}]'
    if s['Fa'] > 8192 or s['Fb'] > 8192:
        return EINVAL, f"Fa = {s['Fa']}, Fb = {s['Fb']}: above 8192 frames"
    if s['path'] and s['P'] > s['Fa'] + s['Fb']:
        return EINVAL, f"P = {s['P']}: above Fa + Fb = {s['Fa'] + s['Fb']} pairs"
    if s['B'] * (s['Fa'] + s['Fb']) > 1 << 19:
        return EINVAL, f"B*(Fa+Fb) too large (B = {s['B']}, Fa = {s['Fa']}, Fb = {s['Fb']}: above {1 << 19} frames); split the batch"
    return 0, ''


def f0_layout(s):
    host, B = s['mem'] == 0, s['B']
    offsets, at = _offsets([2 * B * 4, B * s['Fa'] * 4 * host, B * s['Fb'] * 4 * host, B * s['P'] * 8 * (host and bool(s['path'])), 6 * B * 4 * host])
    return [*offsets, at]


def test_front_end_refuses_by_name_in_the_documented_order(checker):
    refusals = [
        (dict(null='audio'), 'audio is NULL'), (dict(null='out'), 'out is NULL'), (dict(null='out', probe=1, what=0), 'out is NULL'),
        (dict(B=0), 'B = 0 must be at least 1'), (dict(N=0), 'N = 0 must be at least 1'), (dict(rate=0), 'rate = 0 must be at least 1'),
        (dict(hop=0), 'hop = 0 is outside [1, win = 1024]'), (dict(hop=1025), 'hop = 1025 is outside [1, win = 1024]'),
        (dict(win=2049, hop=2049), 'win = 2049 is outside [2, 2048]'), (dict(win=1, hop=1), 'win = 1 is outside [2, 2048]'),
        (dict(tau_min=0), 'lags [0, 367] must satisfy 1 <= tau_min < tau_max <= 1024'),
        (dict(tau_min=367), 'lags [367, 367] must satisfy 1 <= tau_min < tau_max <= 1024'),
        (dict(tau_max=1025), 'lags [45, 1025] must satisfy 1 <= tau_min < tau_max <= 1024'),
        (dict(threshold=0), 'threshold = 0 is outside (0, 1]'), (dict(threshold=1.5), 'threshold = 1.5 is outside (0, 1]'),
        (dict(threshold='nan'), 'threshold = nan is outside (0, 1]'), (dict(threshold=-0.1), 'threshold = -0.1 is outside (0, 1]'),
        (dict(mem=2), 'bad mem kind 2'), (dict(probe=1, what=3), 'what = 3 is no stage (0 difference, 1 normalised difference, 2 pick)'),
        (dict(probe=1, what=-1), 'what = -1 is no stage (0 difference, 1 normalised difference, 2 pick)'),
        (dict(len=[1, 0, 1]), 'lengths[1] = 0 is outside [1, N = 6000]'), (dict(len=[6001, 0, 1]), 'lengths[0] = 6001 is outside [1, N = 6000]'),
        (dict(B=1, N=(1 << 24) + 1), 'N = 16777217: above 16777216 samples'),
        (dict(B=32, N=1 << 24), 'audio too large (B = 32, N = 16777216: 2^31 bytes or more); split the batch'),
        (dict(B=16, N=1 << 24, hop=1, win=2, tau_min=1, tau_max=2), f'out too large ({3 * 16 * ((1 << 24) + 1)} floats: 2^31 bytes or more); split the batch'),
        (dict(B=200, N=1000000, hop=1, win=4, tau_min=1, tau_max=3, probe=1, what=0),
         f'out too large ({200 * 1000001 * 4} floats: 2^31 bytes or more); split the batch'),
        # pairs of faults: first match wins, in the documented order
        (dict(null='audio,out', B=0), 'audio is NULL'), (dict(null='out', B=0), 'out is NULL'), (dict(B=0, N=0), 'B = 0 must be at least 1'),
        (dict(N=0, rate=0), 'N = 0 must be at least 1'), (dict(rate=0, hop=0), 'rate = 0 must be at least 1'),
        (dict(hop=3000, win=2500), 'hop = 3000 is outside [1, win = 2500]'), (dict(win=2500, tau_max=2000), 'win = 2500 is outside [2, 2048]'),
        (dict(tau_min=0, threshold=2), 'lags [0, 367] must satisfy 1 <= tau_min < tau_max <= 1024'),
        (dict(threshold=2, mem=7), 'threshold = 2 is outside (0, 1]'), (dict(mem=7, probe=1, what=9), 'bad mem kind 7'),
        (dict(probe=1, what=9, len=[0, 0, 0]), 'what = 9 is no stage (0 difference, 1 normalised difference, 2 pick)'),
        (dict(B=1, N=(1 << 24) + 1, len=[(1 << 24) + 2]), 'lengths[0] = 16777218 is outside [1, N = 16777217]'),
        (dict(B=64, N=(1 << 24) + 1), 'N = 16777217: above 16777216 samples'),
    ]
    seen = set()
    for wrong, msg in refusals:
        s = dict(GOOD, **wrong)
        assert _call(checker, s) == (EINVAL, 'who: ' + msg, None), wrong
        want = pitch_check(dict(s, threshold=float(s['threshold'])))
        assert want == (EINVAL, msg), (wrong, want)
        seen.add(re.sub(r'-?\d+', '#', msg))
    assert len(seen) >= 14, sorted(seen)
    f0_refusals = [
        (dict(null='f0_a'), 'f0_a is NULL'), (dict(null='f0_b'), 'f0_b is NULL'), (dict(null='stats'), 'stats is NULL'),
        (dict(B=0), 'B = 0 must be at least 1'), (dict(Fa=0), 'Fa = 0 must be at least 1'), (dict(Fb=-1), 'Fb = -1 must be at least 1'),
        (dict(path=1, P=0), 'P = 0 must be at least 1'), (dict(gross=0), 'gross_cents = 0 must be finite and positive'),
        (dict(gross='inf'), 'gross_cents = inf must be finite and positive'), (dict(gross='nan'), 'gross_cents = nan must be finite and positive'),
        (dict(gross=-3), 'gross_cents = -3 must be finite and positive'), (dict(mem=5), 'bad mem kind 5'),
        (dict(la=[1, 41, 1]), 'len_a[1] = 41 is outside [1, Fa = 40]'), (dict(lb=[0, 1, 1]), 'len_b[0] = 0 is outside [1, Fb = 52]'),
        (dict(B=1, Fa=8193), 'Fa = 8193, Fb = 52: above 8192 frames'), (dict(path=1, P=93), 'P = 93: above Fa + Fb = 92 pairs'),
        (dict(B=65, Fa=8192, Fb=1), 'B*(Fa+Fb) too large (B = 65, Fa = 8192, Fb = 1: above 524288 frames); split the batch'),
        (dict(null='stats,f0_b', B=0), 'f0_b is NULL'), (dict(B=0, Fa=0), 'B = 0 must be at least 1'), (dict(Fb=0, path=1, P=0), 'Fb = 0 must be at least 1'),
        (dict(path=1, P=0, gross=0), 'P = 0 must be at least 1'), (dict(gross=0, mem=5), 'gross_cents = 0 must be finite and positive'),
        (dict(mem=5, la=[0, 0, 0]), 'bad mem kind 5'), (dict(la=[1, 1, 99], lb=[0, 1, 1]), 'len_a[2] = 99 is outside [1, Fa = 40]'),
        (dict(B=1, Fa=8193, la=[8194]), 'len_a[0] = 8194 is outside [1, Fa = 8193]'),
        (dict(B=70, Fa=8193, Fb=1, path=1, P=9000), 'Fa = 8193, Fb = 1: above 8192 frames'),
        (dict(B=70, Fa=8192, Fb=1, path=1, P=8194), 'P = 8194: above Fa + Fb = 8193 pairs'),
    ]
    for wrong, msg in f0_refusals:
        s = dict(GOOD_F0, **wrong)
        assert _call(checker, s) == (EINVAL, 'who: ' + msg, None), wrong
        assert f0_check(dict(s, gross=float(s['gross']))) == (EINVAL, msg), wrong
    assert _call(checker, dict(GOOD_F0, P=0)) == (0, '', f0_layout(dict(GOOD_F0, P=0)))          # no path: P is not looked at


def test_front_end_accepts_and_sizes_at_the_limits(checker):
    for wrong in [dict(), dict(mem=1), dict(B=1, N=1, hop=1, win=2, tau_min=1, tau_max=2), dict(win=2048, hop=2048, tau_min=1, tau_max=1024),
                  dict(threshold=1), dict(threshold=1e-30), dict(B=1, N=1 << 24, mem=1), dict(B=31, N=1 << 24, mem=1), dict(len=[1, 6000, 77]),
                  dict(B=8, N=204800, mem=1), dict(B=8, N=204800, probe=1, what=1, mem=1), dict(hop=1024), dict(rate=1),
                  dict(B=1, N=1458000, probe=1, what=0, mem=1),
                  *(dict(probe=1, what=w, mem=m) for w in range(3) for m in (0, 1))]:
        s = dict(GOOD, **wrong)
        assert _call(checker, s) == (0, '', pitch_layout(s)), wrong
        assert pitch_check(s) == (0, '')
    top = (1 << 29) // 368                                           # B * F of a probe at the default lags, at and one above
    assert pitch_check(dict(GOOD, B=1, hop=1, N=top - 1, probe=1, what=1)) == (0, '') != pitch_check(dict(GOOD, B=1, hop=1, N=top, probe=1, what=1))
    for n in (top - 1, top):
        s = dict(GOOD, B=1, hop=1, N=n, probe=1, what=1, mem=1)
        assert _call(checker, s)[:2] == (pitch_check(s)[0], 'who: ' + pitch_check(s)[1] if pitch_check(s)[0] else '')
    assert pitch_layout(GOOD)[:2] == [24, 128] and pitch_layout(dict(GOOD, tau_max=1024))[1] == 320 and pitch_layout(dict(GOOD, tau_min=1, tau_max=255))[1] == 64
    for wrong in [dict(), dict(mem=1), dict(path=1), dict(path=1, mem=1), dict(path=1, P=92), dict(B=1, Fa=8192, Fb=8192, path=1, P=16384),
                  dict(B=32, Fa=8192, Fb=8192), dict(B=1 << 18, Fa=1, Fb=1, path=1, P=1), dict(la=[1, 40, 7], lb=[52, 1, 9]), dict(gross=1e-30)]:
        s = dict(GOOD_F0, **wrong)
        assert _call(checker, s) == (0, '', f0_layout(s)), wrong
        assert f0_check(s) == (0, '')


def test_front_end_equals_its_restatement_on_random_calls(checker):
    rng = np.random.default_rng(23)
    pick = lambda *pool: pool[int(rng.integers(len(pool)))]
    seen = set()
    for _ in range(150):
        B = pick(3, 3, 1, 8, 0, -1)
        s = dict(B=B, N=pick(6000, 6000, 1, 1 << 24, (1 << 24) + 1, 0), rate=pick(22050, 16000, 0), hop=pick(256, 256, 1, 1024, 1025, 0),
                 win=pick(1024, 1024, 2, 2048, 2049, 1), tau_min=pick(45, 45, 1, 0, 367), tau_max=pick(367, 367, 1024, 1025, 2),
                 threshold=pick(0.1, 0.1, 1.0, 0.0, 1.5), mem=pick(0, 1, 1, 5), probe=pick(0, 0, 1), what=pick(-1, 0, 1, 2, 3),
                 null=','.join(n for n in ('audio', 'out') if rng.random() < 0.04),
                 len=pick(None, None, [int(pick(1, 1, 6000, 6001, 0)) for _ in range(max(B, 0))]))
        want = pitch_check(s)
        rc, why, layout = _call(checker, s)
        assert (rc, why) == (want[0], 'who: ' + want[1] if want[0] else ''), (s, rc, why)
        assert layout == (pitch_layout(s) if rc == 0 else None), s
        seen.add(re.sub(r'-?\d+', '#', why))
        B = pick(3, 3, 1, 64, 65, 0)
        s = dict(f0=1, B=B, Fa=pick(40, 40, 1, 8192, 8193, 0), Fb=pick(52, 52, 1, 8192, -1), P=pick(91, 1, 0, 16384, 16385), path=pick(0, 1, 1),
                 gross=pick(315.64, 315.64, 0.0, -1.0), mem=pick(0, 1, 1, 5), null=','.join(n for n in ('f0_a', 'f0_b', 'stats') if rng.random() < 0.04),
                 la=pick(None, None, [int(pick(1, 1, 40, 41, 0)) for _ in range(max(B, 0))]),
                 lb=pick(None, None, [int(pick(1, 1, 52, 53)) for _ in range(max(B, 0))]))
        want = f0_check(s)
        rc, why, layout = _call(checker, s)
        assert (rc, why) == (want[0], 'who: ' + want[1] if want[0] else ''), (s, rc, why)
        assert layout == (f0_layout(s) if rc == 0 else None), s
        seen.add(re.sub(r'-?\d+', '#', why))
    assert '' in seen and len(seen) >= 16, sorted(seen)


# ---- 5. the bindings' library calls ---------------------------------------------------------------------------------------------
def _sha(array):
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(array).tobytes()).hexdigest()[:12]


def _arr(x, dtype):
    return {'dtype': dtype, 'shape': list(np.shape(x)), 'sha': _sha(np.asarray(x).astype(dtype))}


def test_library_calls_of_the_bindings():
    x = np.random.default_rng(1).standard_normal((3, 3000))
    lens = [3000, 1024, 7]
    thr = float(np.float32(0.1))
    calls = record_calls(lambda e: e.pitch(x, lens))
    assert calls == [['pitch', ['engine', _arr(x, 'float32'), 3, 3000, _arr(lens, 'int32'), 22050, 256, 1024, 45, 367, pytest.approx(thr),
                                {'dtype': 'float32', 'shape': [3, 3, 12]}, 0, None]]]
    calls = record_calls(lambda e: e.pitch(x[0], rate=16000, hop=200, win=800, fmin=50, fmax=400, threshold=0.15))      # one row
    assert calls == [['pitch', ['engine', _arr(x[:1], 'float32'), 1, 3000, None, 16000, 200, 800, 40, 320, pytest.approx(0.15),
                                {'dtype': 'float32', 'shape': [3, 1, 16]}, 0, None]]]
    for what, code, shape in (('difference', 0, [3, 12, 368]), ('cmnd', 1, [3, 12, 368]), ('pick', 2, [2, 3, 12])):
        calls = record_calls(lambda e: e.pitch_probe(x, lens, what=what))
        assert calls == [['pitch_probe', ['engine', _arr(x, 'float32'), 3, 3000, _arr(lens, 'int32'), 22050, 256, 1024, 45, 367, pytest.approx(thr),
                                          code, {'dtype': 'float32', 'shape': shape}, 0, None]]], what
    a, b = np.abs(x[:, :40]) * 100, np.abs(x[:, :52]) * 100
    path = np.random.default_rng(2).integers(-1, 40, (3, 91, 2))
    gross = 1200 * np.log2(1.2)
    calls = record_calls(lambda e: e.f0_error(a, b, [40, 1, 7], None, path.astype(np.int64)))
    assert calls == [['f0_error', ['engine', _arr(a, 'float32'), _arr(b, 'float32'), 3, 40, 52, _arr([40, 1, 7], 'int32'), None, _arr(path, 'int32'),
                                   91, pytest.approx(gross), {'dtype': 'float32', 'shape': [6, 3]}, 0, None]]]
    calls = record_calls(lambda e: e.f0_error(a[0], b[0], gross_cents=50))
    assert calls == [['f0_error', ['engine', _arr(a[:1], 'float32'), _arr(b[:1], 'float32'), 1, 40, 52, None, None, None, 0, 50.0,
                                   {'dtype': 'float32', 'shape': [6, 1]}, 0, None]]]
    calls = record_calls(lambda e: e.f0_error(a[0], b[0], path=path[0]))                                     # one row and its [P, 2] path
    assert calls[0][1][8:10] == [_arr(path[:1], 'int32'), 91]


REFUSALS = {
    'stream': (lambda e, x: e.pitch(x, stream=object()), 'stream= needs device tensors'),
    'rank': (lambda e, x: e.pitch(x[None]), r'pitch: audio must be \[B, N\]'),
    'empty': (lambda e, x: e.pitch(x[:, :0]), r'pitch: audio must be \[B, N\]'),
    'rate': (lambda e, x: e.pitch(x, rate=0), 'pitch: rate = 0 must be a positive integer'),
    'hop': (lambda e, x: e.pitch(x, hop=2000), r'pitch: hop = 2000 is outside \[1, win = 1024\]'),
    'hop_float': (lambda e, x: e.pitch(x, hop=12.5), 'pitch: hop = 12.5 must be a positive integer'),
    'win': (lambda e, x: e.pitch(x, win=4096), r'pitch: win = 4096 is outside \[2, 2048\]'),
    'fmin_low': (lambda e, x: e.pitch(x, fmin=20.), r'give the lags \[45, 1102\]'),
    'one_lag': (lambda e, x: e.pitch(x, fmin=405., fmax=410.), r'give the lags \[54, 54\]'),
    'fmin_above_fmax': (lambda e, x: e.pitch(x, fmin=500., fmax=60.), 'must satisfy 0 < fmin < fmax'),
    'threshold': (lambda e, x: e.pitch(x, threshold=0.), r'pitch: threshold = 0.0 is outside \(0, 1\]'),
    'threshold_float32_zero': (lambda e, x: e.pitch(x, threshold=1e-50), r'pitch: threshold = 1e-50 is outside \(0, 1\] as a float32'),
    'threshold_float32_above': (lambda e, x: e.pitch_probe(x, threshold=1.5), r'pitch_probe: threshold = 1.5 is outside'),
    'lengths_shape': (lambda e, x: e.pitch(x, [4, 4]), r'pitch: lengths must hold one value per row, shape \(3,\)'),
    'lengths_low': (lambda e, x: e.pitch(x, [4, 0, 4]), r'pitch: lengths must lie in \[1, 3000\]'),
    'lengths_high': (lambda e, x: e.pitch(x, [4, 3001, 4]), r'pitch: lengths must lie in \[1, 3000\]'),
    'probe_what': (lambda e, x: e.pitch_probe(x, what='f0'), 'what must be one of'),
    'probe_lengths': (lambda e, x: e.pitch_probe(x, [0, 1, 1]), r'pitch_probe: lengths must lie in \[1, 3000\]'),
    'f0_rank': (lambda e, x: e.f0_error(x, x[0]), 'f0_error: f0_a and f0_b must be'),
    'f0_rows': (lambda e, x: e.f0_error(x, x[:2]), 'f0_error: f0_a and f0_b must be'),
    'f0_path_shape': (lambda e, x: e.f0_error(x, x, path=np.zeros((3, 5, 3), np.int32)), r'f0_error: path must be \[B = 3, P, 2\]'),
    'f0_path_rows': (lambda e, x: e.f0_error(x, x, path=np.zeros((2, 5, 2), np.int32)), r'f0_error: path must be \[B = 3, P, 2\]'),
    'f0_path_long': (lambda e, x: e.f0_error(x[:, :4], x[:, :5], path=np.zeros((3, 10, 2), np.int32)), 'a path of 10 pairs is longer than Fa \\+ Fb = 9'),
    'f0_gross': (lambda e, x: e.f0_error(x, x, gross_cents=float('inf')), 'gross_cents = inf must be finite and positive'),
    'f0_gross_zero': (lambda e, x: e.f0_error(x, x, gross_cents=0), 'gross_cents = 0 must be finite and positive'),
    'f0_frames': (lambda e, x: e.f0_error(np.zeros((1, 8193), np.float32), x[:1]), 'above 8192 frames a side'),
    'f0_lengths': (lambda e, x: e.f0_error(x, x, None, [1, 1, 3001]), r'f0_error: lengths_b must lie in \[1, 3000\]'),
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_a_bad_argument_raises_before_any_library_call(name):
    case, match = REFUSALS[name]
    x = np.zeros((3, 3000), np.float32)
    calls = None

    def guarded(eng):
        nonlocal calls
        calls = eng._lib.calls
        with pytest.raises(ValueError, match=match):
            case(eng, x)

    record_calls(guarded)
    assert calls == []


def test_hz_to_lags_and_the_frame_grid():
    from text_to_speech_amd.pitch import PITCH_DEFAULTS, frame_count, hz_to_lags
    assert hz_to_lags(22050, 60., 500.) == (45, 367) and hz_to_lags(16000, 50, 400) == (40, 320) and hz_to_lags(80, 2, 40) == (2, 40)
    assert PITCH_DEFAULTS == dict(rate=22050, hop=256, win=1024, fmin=60., fmax=500., threshold=0.1)
    assert [frame_count(n) for n in (1, 255, 256, 1024, 204800)] == [1, 1, 2, 5, 801]
    for bad in ((22050, 0., 500.), (22050, 500., 500.), (22050, float('nan'), 500.), (22050, 60., float('inf')), (0, 60., 500.), (22050.5, 60., 500.)):
        with pytest.raises(ValueError):
            hz_to_lags(*bad)


class _Engine:
    """Stands for an engine: records what it is asked and answers with recognisable planes."""

    def __init__(self):
        self.calls = []

    def pitch(self, audio, lengths=None, **kw):
        self.calls.append(('pitch', np.shape(audio), None if lengths is None else list(lengths), kw))
        B, F = np.shape(audio)[0], 1 + np.shape(audio)[1] // kw.get('hop', 256)
        out = np.zeros((3, B, F), np.float32)
        out[0, :, ::2], out[1], out[2] = 100.0, 220.5, 0.25
        return out

    def f0_error(self, a, b, la=None, lb=None, path=None, **kw):
        self.calls.append(('f0_error', np.shape(a), np.shape(b), la, lb, None if path is None else np.asarray(path).copy(), kw))
        B = np.shape(a)[0]
        return np.stack([np.full(B, 10.), np.arange(B), np.full(B, 30.), np.full(B, -5.), np.full(B, 2.), np.arange(B) * 0.5]).astype(np.float32)


def test_estimate_f0_and_metrics_name_their_results():
    from text_to_speech_amd import metrics
    from text_to_speech_amd.pitch import estimate_f0
    eng = _Engine()
    res = estimate_f0(eng, np.zeros((2, 1000), np.float32), [1000, 300], hop=100, fmin=80.)
    assert eng.calls == [('pitch', (2, 1000), [1000, 300], dict(hop=100, fmin=80.))]
    assert sorted(res) == ['aperiodicity', 'f0', 'frames', 'period', 'voiced']
    assert res['frames'].tolist() == [11, 4] and res['f0'].shape == (2, 11) and res['voiced'].dtype == bool
    assert np.array_equal(res['voiced'], res['f0'] > 0) and np.all(res['period'] == 220.5) and np.all(res['aperiodicity'] == 0.25)
    assert estimate_f0(eng, np.zeros((2, 1000), np.float32))['frames'].tolist() == [4, 4]
    eng.calls.clear()
    a = np.ones((3, 9), np.float32)
    paths = [np.array([[0, 0], [1, 1]]), np.zeros((0, 2), int), np.array([[0, 0], [0, 1], [1, 2]])]
    res = metrics.f0_error(eng, a, a, [9, 9, 1], None, paths, gross_cents=100.0)
    assert list(res) == ['pairs', 'voiced_pairs', 'rmse_cents', 'mean_cents', 'vuv_errors', 'gross_errors', 'vuv_error', 'gross_error']
    name, sa, sb, la, lb, path, kw = eng.calls[0]
    assert (name, sa, sb, la, lb, kw) == ('f0_error', (3, 9), (3, 9), [9, 9, 1], None, dict(gross_cents=100.0))
    assert path.shape == (3, 3, 2) and path.dtype == np.int32 and path[0].tolist() == [[0, 0], [1, 1], [-1, -1]] and np.all(path[1] == -1)
    assert np.allclose(res['vuv_error'], 0.2) and res['gross_error'].tolist() == [0.0, 0.5, 0.5]      # 0 / 0 voiced pairs: 0
    dense = np.zeros((3, 4, 2), np.int32)
    metrics.f0_error(eng, a, a, path=dense)
    assert eng.calls[1][5] is not None and eng.calls[1][5].shape == (3, 4, 2) and eng.calls[1][6] == {}


def test_runtime_hands_the_pitch_calls_to_its_engine():
    from text_to_speech_amd.runtime import HipRuntime
    eng = _Engine()
    rt = HipRuntime.__new__(HipRuntime)
    rt.engine = eng
    x = np.zeros((2, 600), np.float32)
    assert rt.pitch(x, [600, 5], hop=100).shape == (3, 2, 7)
    assert rt.f0_error(x, x, [3, 3], None, None, gross_cents=9.0).shape == (6, 2)
    assert eng.calls[0] == ('pitch', (2, 600), [600, 5], dict(hop=100)) and eng.calls[1][0] == 'f0_error' and eng.calls[1][6] == dict(gross_cents=9.0)
    eng.pitch_probe = lambda audio, lengths=None, **kw: ('probe', lengths, kw)
    assert rt.pitch_probe(x, [1, 2], what='pick') == ('probe', [1, 2], dict(what='pick'))


# ---- 6. the model methods on recording stand-ins ----------------------------------------------------------------------------------
from test_mel_dtw import _Dev, _SynthRuntime          # noqa: E402  (the stand-ins of the MCD tests: a tensor that logs what comes to the host)


def _fake_tracks(audio, lengths=None, **kw):
    """[3, B, F] whose f0 plane is recognisable: 100 Hz plus the row's mean sample, unvoiced on every third frame"""
    B, N = audio.shape
    out = np.zeros((3, B, 1 + N // 256), np.float32)
    out[0] = 100.0 + np.nan_to_num(np.asarray(audio, np.float64)).mean(axis=1, keepdims=True)
    out[0, :, ::3] = 0.0
    return out


def _fake_f0_stats(a, b, la, lb, path):
    return np.stack([pr.f0_error(a[r], b[r], int(la[r]), int(lb[r]), None if path is None else path[r]) for r in range(len(a))], axis=1).astype(np.float32)


def test_resynthesis_f0_vocodes_tracks_and_compares():
    from text_to_speech_amd.waveglow import WaveGlow
    log, calls = [], []

    class Engine:
        def pitch(self, audio, lengths=None, **kw):
            calls.append(('pitch', audio, lengths, kw))
            return _Dev(_fake_tracks(audio.array), log)

        def f0_error(self, a, b, la=None, lb=None, path=None, **kw):
            calls.append(('f0_error', a, b, la, lb, path, kw))
            F = a.shape[1]
            return _Dev(_fake_f0_stats(a.array, b.array, [F], [F], None), log)

    class Runtime:
        engine = Engine()

        def _uploaded(self, x):
            return _Dev(np.asarray(x, np.float32), log)

        def __call__(self, mel, **kw):
            calls.append(('infer', mel, kw))
            return _Dev(np.full((1, mel.shape[1] * 256 + 100), 7.0, np.float32), log)

    rng = np.random.default_rng(4)
    mels = [rng.standard_normal((n, 80)).astype(np.float32) for n in (12, 5)]
    waves = [rng.standard_normal(n).astype(np.float32) for n in (12 * 256 - 40, 5 * 256 + 300)]      # padded with zeros / cut to the mel's samples
    res = WaveGlow(Runtime()).resynthesis_f0(list(zip(waves, mels)), seed=3, sigma=0.8)
    assert res['names'] == ['f0_rmse_cents', 'f0_mean_cents', 'vuv_error', 'gross_error', 'voiced_pairs', 'pairs']
    assert res['per_item'].shape == (6, 2) and res['per_item'].dtype == np.float32
    assert [c[0] for c in calls] == ['infer', 'pitch', 'pitch', 'f0_error'] * 2
    for i, (wave, mel) in enumerate(zip(waves, mels)):
        infer, p_rec, p_voc, err = calls[4 * i:4 * i + 4]
        n = len(mel) * 256
        assert np.array_equal(infer[1].array, mel[None]) and infer[2] == {'seed': 3, 'sigma': 0.8}
        padded = np.zeros(n, np.float32)
        padded[:min(n, len(wave))] = wave[:n]
        assert np.array_equal(p_rec[1].array, padded[None]) and p_rec[2:] == (None, {'rate': 22050})
        assert p_voc[1].shape == (1, n) and np.all(p_voc[1].array == 7.0) and p_voc[2:] == (None, {'rate': 22050})      # cut to the mel's samples
        assert err[1].shape == err[2].shape == (1, len(mel) + 1) and err[3:] == (None, None, None, {})
        s = _fake_f0_stats(err[1].array, err[2].array, [len(mel) + 1], [len(mel) + 1], None)[:, 0]
        assert res['per_item'][:, i].tolist() == [s[2], s[3], s[4] / s[0], s[5] / s[1], s[1], s[0]]
    assert log == [(6, 1), (6, 1)]                                   # only the statistics came to the host
    assert res['per_item'][5].tolist() == [13, 6] and np.all(res['per_item'][4] > 0) and np.all(res['per_item'][0] > 0)
    assert res['mean']['pairs'] == 9.5 and set(res['mean']) == set(res['names'])
    with pytest.raises(ValueError, match='engine'):
        WaveGlow(lambda mel, **kw: None).resynthesis_f0(waves)


class _PitchRuntime(_SynthRuntime):
    """... that also tracks pitch and compares tracks"""

    def __init__(self, frames_of):
        super().__init__(frames_of)
        self.pitches, self.f0s = [], []

    def mel_dtw(self, a, b, lengths_a=None, lengths_b=None, **kwargs):
        stats = super().mel_dtw(a, b, lengths_a, lengths_b, **{k: v for k, v in kwargs.items() if k != 'return_path'})
        if not kwargs.get('return_path'):
            return stats
        self.dtws[-1] = self.dtws[-1][:4] + (kwargs,)
        B, K = len(lengths_a), a.shape[1] + b.shape[1] - 1
        path = np.full((B, K, 2), -1, np.int32)
        for r in range(B):                                           # some monotone path of the row's frames
            n = max(lengths_a[r], lengths_b[r])
            path[r, :n, 0], path[r, :n, 1] = np.minimum(np.arange(n), lengths_a[r] - 1), np.minimum(np.arange(n), lengths_b[r] - 1)
        return stats, _Dev(path, self.to_host)

    def pitch(self, audio, lengths=None, **kw):
        self.pitches.append((audio, lengths, kw))
        return _Dev(_fake_tracks(audio.array if isinstance(audio, _Dev) else audio), self.to_host)

    def f0_error(self, a, b, la=None, lb=None, path=None, **kw):
        self.f0s.append((a, b, la, lb, path, kw))
        return _Dev(_fake_f0_stats(a.array, b.array, la, lb, path.array), self.to_host)


class _Vocoder:
    def __init__(self, log):
        self.calls, self.log = [], log

    def infer(self, mel, **kw):
        self.calls.append((mel, kw))
        return _Dev(np.full((mel.shape[0], mel.shape[1] * 256), 3.0, np.float32), self.log)


def test_evaluate_synthesis_with_a_vocoder_appends_the_f0_figures(monkeypatch):
    import text_to_speech_amd.audio as audio_mod
    from text_to_speech_amd.tacotron2 import Tacotron2
    rng = np.random.default_rng(6)
    texts = ['Hello, World!', 'Hi', 'A somewhat longer sentence.']
    waves = [rng.standard_normal(n).astype(np.float32) for n in (9 * 256 + 17, 700, 30 * 256)]
    # the loaders, without an engine: the waveform as it is, a mel of 1 + n // 256 recognisable frames
    monkeypatch.setattr(audio_mod, 'load_audio', lambda data, rate=None, *, engine, **kw: np.asarray(data, np.float32))
    monkeypatch.setattr(audio_mod, 'load_mel', lambda data, rate=22050, *, engine, **kw: np.full((1 + len(data) // 256, 80), -4.0, np.float32)
                        + np.float32(len(data) % 7))
    n_tok = [len(Tacotron2(None).encode_text(Tacotron2(None).clean_text(t), cleaned=True)) for t in texts]
    rt = _PitchRuntime(lambda n: 0 if n == n_tok[1] else n + 3)      # 'Hi' produces no frame
    voc = _Vocoder(rt.to_host)
    model = Tacotron2(rt, lang='en')
    res = model.evaluate_synthesis(list(zip(texts, waves)), batch_size=2, max_length=2., vocoder=voc, pitch=dict(fmin=80., threshold=0.2))
    assert res['names'] == Tacotron2.SYNTHESIS_NAMES + ['f0_rmse_cents', 'vuv_error', 'gross_error', 'voiced_pairs']
    per = res['per_item']
    assert per.shape == (10, 3) and per.dtype == np.float32
    assert len(rt.infers) == len(rt.dtws) == len(voc.calls) == len(rt.f0s) == 2 and len(rt.pitches) == 4
    for call, rows in enumerate(([0], [2])):                         # of the first batch only row 0 produced frames
        i = rows[0]
        a, b, la, lb, kw = rt.dtws[call]
        assert kw == {'n_cep': 13, 'return_path': True} and la.tolist() == [n_tok[i] + 3] and lb.tolist() == [1 + len(waves[i]) // 256]
        mel, vkw = voc.calls[call]
        assert isinstance(mel, _Dev) and mel.shape[0] == 1 and list(vkw) == ['lengths'] and vkw['lengths'].tolist() == la.tolist()
        (syn, syn_len, kw1), (rec, rec_len, kw2) = rt.pitches[2 * call:2 * call + 2]
        assert kw1 == kw2 == dict(fmin=80., threshold=0.2)
        assert isinstance(syn, _Dev) and np.all(syn.array == 3.0) and syn_len.tolist() == [la[0] * 256]      # the vocoder's audio, on the device
        assert np.array_equal(rec, waves[i][None]) and rec_len.tolist() == [len(waves[i])] and rec_len.dtype == np.int32
        fa, fb, ea, eb, path, fkw = rt.f0s[call]
        assert isinstance(fa, _Dev) and isinstance(fb, _Dev) and isinstance(path, _Dev) and fkw == {}          # tracks and path stay there
        assert ea.tolist() == la.tolist() and eb.tolist() == lb.tolist()
        s = _fake_f0_stats(fa.array, fb.array, ea, eb, path.array)[:, 0]
        assert per[6:, i].tolist() == [s[2], s[4] / s[0], s[5] / max(s[1], 1), s[1]] and s[0] == max(la[0], lb[0]) and s[1] > 0
    assert np.isnan(per[6:, 1]).all() and per[2, 1] == 0             # the row without frames: no figure, as for the MCD
    assert np.isfinite(per[:, [0, 2]]).all()
    for k, name in enumerate(res['names']):
        assert res['mean'][name] == pytest.approx(float(per[k, [0, 2]].astype(np.float64).mean()), rel=1e-12)
    # only lengths, the [3, B] and the [6, B] statistics came to the host
    assert rt.to_host == [(2,), (3, 1), (6, 1), (1,), (3, 1), (6, 1)]
    # a recording shorter than 1024 samples has fewer pitch frames than mel frames: its table says so
    rt2 = _PitchRuntime(lambda n: n + 3)
    monkeypatch.setattr(audio_mod, 'load_mel', lambda data, rate=22050, *, engine, **kw: np.full((5, 80), -4.0, np.float32))
    model2 = Tacotron2(rt2, lang='en')
    model2.evaluate_synthesis([(texts[0], waves[1])], vocoder=_Vocoder(rt2.to_host))
    assert rt2.dtws[0][3].tolist() == [5] and rt2.f0s[0][3].tolist() == [1 + 700 // 256] and rt2.pitches[0][2] == {}
    # the default call is what it was: six names, no path asked for, no pitch call
    rt3 = _PitchRuntime(lambda n: n + 3)
    out = Tacotron2(rt3, lang='en').evaluate_synthesis([(texts[0], np.full((9, 80), -4.0, np.float32))])
    assert out['names'] == ['mcd_dtw', 'path_len', 'frames', 'target_frames', 'frame_ratio', 'stopped'] and out['per_item'].shape == (6, 1)
    assert rt3.dtws[0][4] == {'n_cep': 13} and rt3.pitches == [] and rt3.f0s == []
    # refusals
    with pytest.raises(ValueError, match=r'items\[0\] is a \(text, mel\) pair'):
        model.evaluate_synthesis([(texts[0], np.zeros((9, 80), np.float32))], vocoder=voc)
    with pytest.raises(ValueError, match='hop must stay 256'):
        model.evaluate_synthesis([(texts[0], waves[0])], vocoder=voc, pitch=dict(hop=128))
    with pytest.raises(ValueError, match='pitch= configures the tracker of vocoder='):
        model.evaluate_synthesis([(texts[0], waves[0])], pitch=dict(fmin=80.))
    with pytest.raises(ValueError, match='pitch and f0_error'):
        Tacotron2(_SynthRuntime(lambda n: n + 3), lang='en').evaluate_synthesis([(texts[0], waves[0])], vocoder=voc)
