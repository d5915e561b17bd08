"""CPU: the probabilistic-YIN call (include/tts_hip.h: tts_hip_pyin) without a GPU.

 1. the restatement tests/pyin_ref.py against closed forms, hand-made d' rows and a brute-force decode;
 2. every bound the GPU test uses (pyin_ref.check_run) holds a float32 numpy copy of the call (decode32) with room, and every
    planted mistake changes its stage by at least ten times the stage's bound (or, a discrete stage, changes it);
 3. the quality condition: at a noise of 0.15 the decode misses no voiced frame, voices none inside the gap, makes no gross error,
    and YIN on the same d' misses more than half;
 4. no case of tests/pyin_cases.py has a candidate within 1e-9 of a bin edge;
 5. the front end (csrc/pitch_call.h: pyin_check, pyin_layout, pyin_tables) through the stand-alone sanitizer build against a
    Python restatement, every refusal in order;
 6. host plumbing: beta_prior, pyin_geometry, estimate_f0(method=), f0_method= on recording stand-ins.
"""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pitch_ref as pr
import pyin_cases as yc
import pyin_ref as yr
from test_pitch import CSRC, EINVAL, _offsets, pitch_check

EPS = yr.EPS
TABLE4 = np.array([0.4, 0.3, 0.2, 0.1])          # thresholds 0.25, 0.5, 0.75, 1

# hand-made d' rows (lag 0 first): plateaus on either side, values on a threshold, a later trough that is no deeper
HAND = {
    'plateau_right': [1, 0.9, 0.6, 0.6, 0.8, 0.3, 0.9],            # 2 is a trough (<= on the right), 3 is not (not < on the left)
    'on_threshold': [1, 1.2, 0.5, 0.9, 0.25, 0.7, 0.9],            # d' = 0.5 and 0.25: s_i > d' leaves the threshold itself out
    'not_deeper': [1, 0.8, 0.3, 0.9, 0.4, 0.95, 0.3],              # 4 and 6 are not below the minimum before: p = 0
    'flat': [1, 1, 1, 1, 1, 1, 1],                                   # silence: no lag is below its left neighbour
    'falling': [1, 0.9, 0.8, 0.7, 0.6, 0.5, 0.45],                  # only tau_max is a trough
    'first_not_least': [1, 0.7, 0.9, 0.2, 0.8, 0.6, 0.9],
}
HAND_TROUGHS = {'plateau_right': [2, 5], 'on_threshold': [2, 4], 'not_deeper': [2, 4, 6], 'flat': [], 'falling': [6], 'first_not_least': [1, 3, 5]}


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def test_hand_made_rows_have_the_enumerated_troughs_and_probabilities():
    for name, q in HAND.items():
        flag = yr.troughs(q, 1, 6)
        assert list(np.nonzero(flag)[0]) == HAND_TROUGHS[name], name
    p = yr.trough_probs(HAND['on_threshold'], yr.troughs(HAND['on_threshold'], 1, 6), TABLE4, 0.5)
    # lag 2 (0.5): thresholds 0.75 and 1; lag 4 (0.25): the threshold 0.5 (0.25 itself is not above 0.25), and the least: + 0.5 * 0.4
    assert np.allclose(p, [0, 0, 0.3, 0, 0.3 + 0.5 * 0.4, 0, 0], atol=1e-15)
    p = yr.trough_probs(HAND['not_deeper'], yr.troughs(HAND['not_deeper'], 1, 6), TABLE4, 0.5)
    assert np.allclose(p, [0, 0, 0.6 + 0.5 * 0.4, 0, 0, 0, 0], atol=1e-15)            # the smallest lag of the tie 0.3 = 0.3 is the least
    p = yr.trough_probs(HAND['first_not_least'], yr.troughs(HAND['first_not_least'], 1, 6), TABLE4, 0.5)
    assert np.allclose(p, [0, 0.3, 0, 0.7 + 0, 0, 0, 0], atol=1e-15)                  # no threshold is at or below 0.2


def test_a_frames_probabilities_sum_to_the_prior_above_the_smallest_trough():
    rng = np.random.default_rng(1)
    table, s = yr.prior(), yr.thresholds(100)
    for _ in range(200):
        q = np.concatenate([[1.0], rng.uniform(0, 1.3, 40)])
        flag = yr.troughs(q, 2, 40)
        p = yr.trough_probs(q, flag, table, 0.01)
        if not flag.any():
            assert p.sum() == 0
            continue
        least = q[flag].min()
        assert abs(p.sum() - (table[s > least].sum() + float(np.float32(0.01)) * table[s <= least].sum())) < 1e-14
        assert np.all(p >= 0) and np.all(p[~flag] == 0)


def test_silence_is_unvoiced():
    out = yr.decode(np.ones((3, 41)), rate=80, tau_min=2, tau_max=40, prior_table=yr.prior(), no_trough_prob=0.01, fmin=2.0, bps=2,
                    n_bins=100, max_step=5, switch_prob=0.01)
    assert np.all(out['v'] == 0) and np.all(out['obs'] == 0) and np.all(out['cand'] == 0)
    assert np.all(out['path'] >= 100) and np.all(out['f0'] == 0)


def test_the_prior_and_the_geometry():
    table = yr.prior()
    x = np.arange(101) / 100
    closed = 1 - (1 - x) ** 18 * (1 + 18 * x)
    assert np.allclose(table, np.diff(closed), atol=1e-15) and abs(table.sum() - 1) < 1e-15
    assert yr.geometry(22050, 256, 60., 500.) == (368, 51)
    lt = yr.log_transition(5, 2, 0.01)
    assert np.allclose(np.exp(lt).sum(1), 1.0, atol=1e-15)            # every row a distribution, the truncated edge rows too
    assert lt[0, 3] == -np.inf and np.isfinite(lt[0, 2])


def test_the_decode_is_the_best_of_all_paths():
    rng = np.random.default_rng(2)
    for F in (1, 2, 3, 6):
        for ms in (1, 2):
            logobs = np.log(rng.uniform(0.01, 1, (F, 4)))
            logA = yr.log_transition(2, ms, 0.2)
            got = yr.viterbi(logobs, logA)
            scores = {path: yr.path_score(path, logobs, logA) for path in itertools.product(range(4), repeat=F)}
            best = max(scores.values())
            assert abs(got['score'] - best) < 1e-12 and abs(scores[tuple(got['path'])] - best) < 1e-12
            assert np.all(got['delta'].max(1) == 0)
    # a tie: equal observations everywhere -> the smallest last state, and the smallest predecessor all the way
    got = yr.viterbi(np.zeros((4, 4)), yr.log_transition(2, 2, 0.5))
    assert list(got['path']) == [0, 0, 0, 0]


# ---- 2. the bounds ----------------------------------------------------------------------------------------------------------------
CASES = yc.cases()


def _dp32(case, b):
    c = CASES[case]
    n, g, cfg = int(c['lengths'][b]), c['grid'], c['cfg']
    t = pr.track32(c['audio'][b], n, rate=cfg['rate'], hop=g['hop'], win=g['win'], tau_min=cfg['tau_min'], tau_max=cfg['tau_max'], threshold=0.1)
    fr = pr.frames(c['audio'][b], n, g['hop'], g['win'], cfg['tau_max']).astype(np.float32)
    d = np.stack([np.cumsum((fr[:, :g['win']] - fr[:, tau:tau + g['win']]) ** 2, axis=1, dtype=np.float32)[:, -1] for tau in range(cfg['tau_max'] + 1)], 1)
    S = np.concatenate([np.zeros((len(d), 1), np.float32), np.cumsum(d[:, 1:], axis=1, dtype=np.float32)], axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        dp = np.where(S == 0, np.float32(1), d * np.arange(cfg['tau_max'] + 1, dtype=np.float32) / np.where(S == 0, np.float32(1), S)).astype(np.float32)
    dp[:, 0] = 1
    assert len(t['tau']) == len(dp)
    return dp


@pytest.fixture(scope='module')
def copies():
    """(case, row) -> (dp float32, decode32 of it) for the small cases"""
    out = {}
    for name in ('lags_2_3_step1', 'lags_2_3_step2', 'bins_1', 'bins_63', 'bins_64', 'bins_65', 'on_threshold', 'default'):
        for b in range(len(CASES[name]['lengths'])):
            if name == 'default' and b not in (0, 2):
                continue
            dp = _dp32(name, b)
            out[name, b] = (dp, yr.decode32(dp, **CASES[name]['cfg']))
    return out


def _as_run(o):
    return dict(p=o['p'], obs=o['obs'], cand=o['cand'], delta=o['delta'], back=o['back'], path=o['path'], planes=np.stack([o['f0'], o['pitch'], o['v']]))


def test_a_float32_copy_lies_within_every_bound(copies):
    worst = {}
    for (name, b), (dp, o) in copies.items():
        for stage, ratio in yr.check_run(_as_run(o), dp, CASES[name]['cfg'], f'{name}[{b}]').items():
            worst[stage] = max(worst.get(stage, 0), ratio)
    print('float32 copy, largest error / bound per stage:', {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1 for v in worst.values())


def test_the_end_to_end_bound_is_ten_float32_copies_wide():
    """F0_END_TO_END of tests/test_pitch.py (the same d' and the same interpolation) on the sine rows of these cases: a float32
    copy decoding the same voiced state as the all-float64 restatement lies within a tenth of it (seen: 3.0e-7 of 6.3e-6)"""
    from test_pitch import F0_END_TO_END
    worst, frames = 0.0, 0
    for name, c in CASES.items():
        for b, kind in enumerate(c['kinds']):
            n = int(c['lengths'][b])
            Fb, nb = pr.frame_count(n, c['grid']['hop']), c['cfg']['n_bins']
            if kind not in ('sine_int', 'sine_frac') or Fb <= 4:
                continue
            o = yr.decode32(_dp32(name, b), **c['cfg'])
            ref = yr.track(c['audio'][b], n, hop=c['grid']['hop'], win=c['grid']['win'], **c['cfg'])
            same = (ref['path'] == o['path']) & (ref['path'] < nb) & (ref['cand'][np.arange(Fb), ref['path'] % nb] > 0)
            frames += int(same.sum())
            worst = max(worst, float((np.abs(o['f0'][same] - ref['f0'][same]) / ref['f0'][same]).max()))
    print(f'float32 copy, f0 end to end: {worst:.3g} on {frames} frames')
    assert frames >= 50 and worst <= F0_END_TO_END / 10


# which stage a mistake shows in, and the inputs it shows on
STAGE = {'trough_left_le': 'p', 'trough_right_lt': 'p', 'threshold_le': 'p', 'prefix_includes_self': 'p', 'no_trough_on_first': 'p',
         'prior_density': 'p', 'bin_truncated': 'obs', 'bins_ascending': 'obs', 'cand_largest_lag': 'cand', 'unvoiced_not_divided': 'delta',
         'triangle_unnormalised': 'delta', 'switch_wrong_branch': 'delta', 'no_renorm': 'delta', 'ties_largest': 'back',
         'backtrack_off_by_one': 'path'}


def _hand_decode(mistake=None):
    """the hand-made rows as six frames of one row, and a second row of random d'"""
    rng = np.random.default_rng(3)
    dp = np.array(list(HAND.values()), np.float64)
    more = np.concatenate([np.ones((8, 1)), rng.uniform(0.05, 1.2, (8, 6))], 1)
    cfg = dict(rate=6, tau_min=1, tau_max=6, prior_table=yr.prior(2, 18, 4, 'prior_density' if mistake == 'prior_density' else None),
               no_trough_prob=0.25, fmin=1.0, bps=2, n_bins=8, max_step=2, switch_prob=0.3)
    return [(q, yr.decode(q, mistake=mistake, **cfg)) for q in (dp, more)], cfg


def test_every_planted_mistake_changes_its_stage_by_ten_bounds_or_more():
    assert set(STAGE) == set(yr.MISTAKES) and len(yr.MISTAKES) >= 15
    right, cfg = _hand_decode()
    tie = np.zeros((4, 16))                                               # equal scores: ties everywhere
    for mistake in yr.MISTAKES:
        wrong, _ = _hand_decode(mistake)
        stage = STAGE[mistake]
        if mistake == 'ties_largest':
            logA = yr.log_transition(8, 2, 0.5)
            assert not np.array_equal(yr.viterbi(tie, logA)['back'], yr.viterbi(tie, logA, mistake)['back'])
            continue
        change = max(float(np.abs(np.asarray(w[stage], np.float64) - np.asarray(r[stage], np.float64)).max()) for (_, w), (_, r) in zip(wrong, right))
        if stage == 'path':
            assert change >= 1, mistake
            continue
        bound = {'p': yr.bound_p(cfg['prior_table']),
                 'obs': max(yr.bound_obs(r['p'][t], r['flag'][t]) for _, r in right for t in range(len(r['p']))),
                 'cand': float(yr.bound_cand(6.5)),
                 'delta': max(yr.bound_delta(r['delta'][t - 1], r['logobs'][t]) for _, r in right for t in range(1, len(r['delta'])))}[stage]
        print(f'{mistake}: changes {stage} by {change:.3g}, the bound is {bound:.3g}')
        assert change >= 10 * bound, (mistake, change, bound)


# ---- 3. the quality condition ----------------------------------------------------------------------------------------------------
def test_quality_condition_at_a_noise_of_0_15():
    """The condition of the issue on the restatement (measured when this was written: pYIN misses 0 voiced frames, voices 0 frames
    of the gap, makes 0 gross errors; YIN misses 93 of 138)."""
    rate, hop, win, fmin, fmax = 22050, 256, 1024, 60., 500.
    x, f, voiced = yc.quality_signal(0.15)
    tau_min, tau_max = int(np.ceil(rate / fmax)), int(np.floor(rate / fmin))
    n_bins, max_step = yr.geometry(rate, hop, fmin, fmax)
    out = yr.track(x, len(x), rate=rate, hop=hop, win=win, tau_min=tau_min, tau_max=tau_max, prior_table=yr.prior(), no_trough_prob=0.01,
                   fmin=fmin, bps=10, n_bins=n_bins, max_step=max_step, switch_prob=0.01)
    F = len(out['f0'])
    centre = np.arange(F) * hop                                         # frame t reads [t hop - win / 2, t hop + win / 2 + tau_max)
    gap = (int(0.5 * rate), int(0.75 * rate))
    inside_voiced = (centre >= win) & (centre + win < len(x)) & ((centre + win < gap[0]) | (centre - win >= gap[1]))
    inside_gap = (centre - win >= gap[0]) & (centre + win < gap[1])
    yin_voiced, _ = pr.pick(out['dp'], tau_min, tau_max, 0.1)
    got = out['f0'] > 0
    truth = f[np.minimum(centre + 79, len(x) - 1)]                   # a difference at lag tau is centred tau / 2 behind t hop
    cents = 1200 * np.log2(np.where(got, out['f0'], truth) / truth)
    missed, false, gross = int((inside_voiced & ~got).sum()), int((inside_gap & got).sum()), int((inside_voiced & got & (np.abs(cents) > 1200 * np.log2(1.2))).sum())
    yin_missed = int((inside_voiced & ~yin_voiced).sum())
    print(f'pYIN misses {missed} of {inside_voiced.sum()} voiced frames, voices {false} of {inside_gap.sum()} frames of the gap, {gross} gross errors; '
          f'YIN misses {yin_missed}; largest deviation {np.abs(cents[inside_voiced & got]).max():.1f} cents')
    assert inside_voiced.sum() > 100 and inside_gap.sum() >= 10
    assert missed == 0 and false == 0 and gross == 0
    assert yin_missed > inside_voiced.sum() / 2


# ---- 4. the bin-rounding guard ---------------------------------------------------------------------------------------------------
def test_no_case_has_a_candidate_on_a_bin_edge(copies):
    for (name, b), (dp, _) in copies.items():
        pos = yr.positions(dp, CASES[name]['cfg'])
        frac = np.abs(pos - np.floor(pos) - 0.5)
        assert not len(pos) or frac.min() > 1e-9, (name, b, float(frac.min()))


# ---- 5. the front end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    return os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')


GOOD = dict(B=3, N=6000, rate=22050, hop=256, win=1024, tau_min=45, tau_max=367, mem=0, probe=0, what=-1, n_bins=368, bps=10, max_step=51,
            n_thresh=4, switch=0.01, no_trough=0.01, fmin=60.0, null='', len=None, prior=None, tables=0)


def _call(exe, s):
    """-> (status, message, the layout numbers or None, the tables or None)"""
    args = [f'{k}={v}' for k, v in s.items() if k not in ('null', 'len', 'prior')]
    args += [f'{k}=' + ','.join(str(v) for v in s[k]) for k in ('len', 'prior') if s.get(k) is not None]
    args += [f"null={s['null']}"] if s['null'] else []
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, '--pyin'] + args, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    rc, _, msg = lines[0].partition(' ')
    return (int(rc), msg, [int(v) for v in lines[1].split()] if len(lines) > 1 else None,
            np.array([float(v) for v in lines[2:]], np.float32) if len(lines) > 2 else None)


def _out_elems(s):
    BF = s['B'] * (1 + s['N'] // s['hop'])
    if not s['probe']:
        return 3 * BF
    return BF * (s['tau_max'] + 1) if s['what'] == 0 else BF if s['what'] == 4 else BF * 2 * s['n_bins']


def pyin_check(s):
    """pyin_check restated -> (status, message)"""
    first = pitch_check(dict(s, threshold=0.5, probe=0, what=-1))
    if first[0]:
        return first
    if not 1 <= s['n_bins'] <= 1024:
        return EINVAL, f"n_bins = {s['n_bins']} is outside [1, 1024]"
    if not 1 <= s['bps'] <= 100:
        return EINVAL, f"bins_per_semitone = {s['bps']} is outside [1, 100]"
    if not 1 <= s['max_step'] <= s['n_bins']:
        return EINVAL, f"max_step = {s['max_step']} is outside [1, n_bins = {s['n_bins']}]"
    if not 1 <= s['n_thresh'] <= 1024:
        return EINVAL, f"n_thresh = {s['n_thresh']} is outside [1, 1024]"
    if 'prior' in s['null'].split(','):
        return EINVAL, 'prior is NULL'
    for i, v in enumerate(([1 / s['n_thresh']] * s['n_thresh'] if s['prior'] is None else s['prior'])[:s['n_thresh']]):
        v = np.float32(v)
        if not (np.isfinite(v) and v >= 0):
            return EINVAL, f'prior[{i}] = {float(v):g} must be finite and not negative'
    sw, nt = np.float32(s['switch']), np.float32(s['no_trough'])
    if not 0 < sw < 1:
        return EINVAL, f'switch_prob = {float(sw):g} is outside (0, 1)'
    if not 0 <= nt <= 1:
        return EINVAL, f'no_trough_prob = {float(nt):g} is outside [0, 1]'
    if not (math.isfinite(float(s['fmin'])) and float(s['fmin']) > 0):
        return EINVAL, f"fmin = {float(s['fmin']):g} must be finite and positive"
    if s['probe'] and not 0 <= s['what'] <= 4:
        return EINVAL, f"what = {s['what']} is no stage (0 trough, 1 observation, 2 delta, 3 back, 4 path)"
    BF = s['B'] * (1 + s['N'] // s['hop'])
    if _out_elems(s) * 4 >= 1 << 31:
        return EINVAL, f'out too large ({_out_elems(s)} floats: 2^31 bytes or more); split the batch'
    if BF * s['n_bins'] * 4 >= 1 << 31:
        return EINVAL, f"observations too large ({BF * s['n_bins']} floats: 2^31 bytes or more); split the batch"
    if BF * 2 * s['n_bins'] * 2 >= 1 << 31:
        return EINVAL, f"backpointers too large ({BF * 2 * s['n_bins']} states: 2^31 bytes or more); split the batch"
    return 0, ''


def pyin_layout(s):
    """pyin_layout restated -> [F, threads, vit_threads, lens, in, out, cum, tables, obs, cand, vprob, back, path, out_elems, bytes]"""
    host, B, F, nb = s['mem'] == 0, s['B'], 1 + s['N'] // s['hop'], s['n_bins']
    offsets, at = _offsets([B * 4, B * s['N'] * 4 * host, _out_elems(s) * 4 * host, (s['n_thresh'] + 1) * 4, (s['max_step'] + 1 + nb + 2) * 4,
                            B * F * nb * 4, B * F * nb * 4, B * F * 4, B * F * 2 * nb * 2, B * F * 4])
    return [F, (-(-(s['tau_max'] + 1) // 4) + 63) // 64 * 64, (nb + 63) // 64 * 64, *offsets, _out_elems(s), at]


def test_front_end_refuses_by_name_in_the_documented_order(checker):
    refusals = [
        # what pitch_check refuses comes first, in its order
        (dict(null='audio', n_bins=0), 'audio is NULL'), (dict(null='out', prior=['nan'] * 4), 'out is NULL'), (dict(B=0, n_bins=0), 'B = 0 must be at least 1'),
        (dict(hop=0, bps=0), 'hop = 0 is outside [1, win = 1024]'), (dict(tau_max=1025, n_thresh=0), 'lags [45, 1025] must satisfy 1 <= tau_min < tau_max <= 1024'),
        (dict(mem=2, max_step=0), 'bad mem kind 2'), (dict(len=[1, 0, 1], fmin=0), 'lengths[1] = 0 is outside [1, N = 6000]'),
        (dict(B=1, N=(1 << 24) + 1, n_bins=0), 'N = 16777217: above 16777216 samples'),
        (dict(B=32, N=1 << 24, n_bins=0), 'audio too large (B = 32, N = 16777216: 2^31 bytes or more); split the batch'),
        # then the call's own, one by one
        (dict(n_bins=0), 'n_bins = 0 is outside [1, 1024]'), (dict(n_bins=1025), 'n_bins = 1025 is outside [1, 1024]'),
        (dict(bps=0), 'bins_per_semitone = 0 is outside [1, 100]'), (dict(bps=101), 'bins_per_semitone = 101 is outside [1, 100]'),
        (dict(max_step=0), 'max_step = 0 is outside [1, n_bins = 368]'), (dict(max_step=369), 'max_step = 369 is outside [1, n_bins = 368]'),
        (dict(n_thresh=0), 'n_thresh = 0 is outside [1, 1024]'), (dict(n_thresh=1025), 'n_thresh = 1025 is outside [1, 1024]'),
        (dict(null='prior'), 'prior is NULL'), (dict(prior=[0.1, 'nan', 0.3, 0.4]), 'prior[1] = nan must be finite and not negative'),
        (dict(prior=[0.1, 0.2, 'inf', -1]), 'prior[2] = inf must be finite and not negative'), (dict(prior=[0.1, 0.2, 0.3, -0.5]), 'prior[3] = -0.5 must be finite and not negative'),
        (dict(switch=0), 'switch_prob = 0 is outside (0, 1)'), (dict(switch=1), 'switch_prob = 1 is outside (0, 1)'), (dict(switch='nan'), 'switch_prob = nan is outside (0, 1)'),
        (dict(no_trough=-0.5), 'no_trough_prob = -0.5 is outside [0, 1]'), (dict(no_trough=1.5), 'no_trough_prob = 1.5 is outside [0, 1]'),
        (dict(no_trough='nan'), 'no_trough_prob = nan is outside [0, 1]'),
        (dict(fmin=0), 'fmin = 0 must be finite and positive'), (dict(fmin='inf'), 'fmin = inf must be finite and positive'), (dict(fmin='nan'), 'fmin = nan must be finite and positive'),
        (dict(probe=1, what=5), 'what = 5 is no stage (0 trough, 1 observation, 2 delta, 3 back, 4 path)'),
        (dict(probe=1, what=-1), 'what = -1 is no stage (0 trough, 1 observation, 2 delta, 3 back, 4 path)'),
        (dict(B=1, N=1000000, hop=1, win=4, tau_min=1, tau_max=3, probe=1, what=2, mem=1), f'out too large ({1000001 * 736} floats: 2^31 bytes or more); split the batch'),
        (dict(B=1, N=1500000, hop=1, win=4, tau_min=1, tau_max=3, mem=1), f'observations too large ({1500001 * 368} floats: 2^31 bytes or more); split the batch'),
        (dict(B=1, N=1500000, hop=1, win=4, tau_min=1, tau_max=3, mem=1, n_bins=300, max_step=51), 'who'),
        # pairs of faults: first match wins
        (dict(n_bins=0, bps=0), 'n_bins = 0 is outside [1, 1024]'), (dict(bps=0, max_step=0), 'bins_per_semitone = 0 is outside [1, 100]'),
        (dict(max_step=0, n_thresh=0), 'max_step = 0 is outside [1, n_bins = 368]'), (dict(n_thresh=0, null='prior'), 'n_thresh = 0 is outside [1, 1024]'),
        (dict(null='prior', switch=0), 'prior is NULL'), (dict(prior=[0, 0, 0, -1], switch=0), 'prior[3] = -1 must be finite and not negative'),
        (dict(switch=2, no_trough=2), 'switch_prob = 2 is outside (0, 1)'), (dict(no_trough=2, fmin=-1), 'no_trough_prob = 2 is outside [0, 1]'),
        (dict(fmin=-1, probe=1, what=9), 'fmin = -1 must be finite and positive'),
    ]
    seen = set()
    for wrong, msg in refusals:
        s = dict(GOOD, **wrong)
        want = pyin_check(s)
        if msg == 'who':                                                 # 300 bins: the observations fit, the backpointers do not? neither: 1.8e9 bytes each
            assert want == (0, '') and _call(checker, s)[:3] == (0, '', pyin_layout(s)), wrong
            continue
        assert _call(checker, s)[:3] == (EINVAL, 'who: ' + msg, None), wrong
        assert want == (EINVAL, msg), (wrong, want)
        seen.add(msg.split('=')[0].split('(')[0])
    assert len(seen) >= 18, sorted(seen)
    # the backpointers alone: 2 n_bins uint16 a frame are as many bytes as the observations' n_bins floats, so the observations'
    # refusal always comes first; the restatement and the library agree at the edge
    top = (1 << 29) // 368
    for n in (top - 1, top):
        s = dict(GOOD, B=1, hop=1, N=n, win=4, tau_min=1, tau_max=3, mem=1)
        want = pyin_check(s)
        assert _call(checker, s)[:2] == (want[0], 'who: ' + want[1] if want[0] else ''), n
    assert pyin_check(dict(GOOD, B=1, hop=1, N=top - 2, win=4, tau_min=1, tau_max=3, mem=1)) == (0, '') != pyin_check(dict(GOOD, B=1, hop=1, N=top, win=4, tau_min=1, tau_max=3, mem=1))


def test_front_end_accepts_sizes_and_builds_its_tables(checker):
    for wrong in [dict(), dict(mem=1), dict(n_bins=1, max_step=1), dict(n_bins=1024, max_step=1024, bps=100, n_thresh=1024),
                  dict(B=1, N=1, hop=1, win=2, tau_min=1, tau_max=2), dict(switch=1e-30), dict(no_trough=0), dict(no_trough=1), dict(len=[1, 6000, 77]),
                  dict(prior=[0, 0, 0, 0]), dict(fmin=1e-300), *(dict(probe=1, what=w, mem=m) for w in range(5) for m in (0, 1))]:
        s = dict(GOOD, **wrong)
        assert _call(checker, s)[:3] == (0, '', pyin_layout(s)), wrong
        assert pyin_check(s) == (0, '')
    for nb, ms, sp, table in ((5, 2, 0.01, [0.4, 0.3, 0.2, 0.1]), (368, 51, 0.01, None), (3, 3, 0.3, [0.25, 0.25, 0.25, 0.25]), (1, 1, 0.5, None)):
        s = dict(GOOD, n_bins=nb, max_step=ms, switch=sp, prior=table, tables=1)
        rc, msg, layout, got = _call(checker, s)
        assert (rc, msg) == (0, '') and layout == pyin_layout(s)
        table = np.asarray([0.25] * 4 if table is None else table, np.float32).astype(np.float64)
        i = np.arange(nb)
        w = np.maximum(0, ms + 1 - np.abs(i[:, None] - i[None, :]))
        want = np.concatenate([[0], np.cumsum(table), np.log(ms + 1 - np.arange(ms + 1)), np.log(w.sum(1)),
                               [math.log1p(-float(np.float32(sp))), math.log(float(np.float32(sp)))]])
        assert got.shape == want.shape and np.all(np.abs(got - want) <= EPS * np.abs(want) * 1.01 + 1e-45), (nb, ms)
        # the triangle over the norm is the restatement's transition
        lt = yr.log_transition(nb, ms, sp)[:nb, :nb]
        mine = want[5 + np.abs(i[:, None] - i[None, :]).clip(max=ms)] - want[5 + ms + 1 + i][:, None] + want[-2]
        assert np.allclose(np.where(np.isfinite(lt), mine, -np.inf), lt, atol=1e-12)


# ---- 6. host plumbing -------------------------------------------------------------------------------------------------------------
def test_beta_prior_and_geometry_helpers():
    from text_to_speech_amd import pitch
    assert np.allclose(pitch.beta_prior(), yr.prior(), atol=1e-16) and pitch.beta_prior().dtype == np.float64
    for a, b, n in ((2, 18, 100), (1, 1, 7), (3, 5, 1024), (2, 18, 1)):
        table = pitch.beta_prior(a, b, n)
        assert table.shape == (n,) and abs(table.sum() - 1) < 1e-13 and np.all(table >= 0)
    assert np.allclose(pitch.beta_prior(1, 1, 4), 0.25)
    try:
        from scipy.stats import beta
    except ImportError:
        beta = None
    if beta is not None:
        for a, b in ((2, 18), (3, 5), (1, 4), (7, 1)):
            x = np.arange(101) / 100
            assert np.abs(beta.cdf(x, a, b) - np.array([pitch.beta_cdf(v, a, b) for v in x])).max() < 1e-13
    for bad in ((0, 18, 100), (2, 0.5, 100), (2, 18, 0)):
        with pytest.raises(ValueError):
            pitch.beta_prior(*bad)
    assert pitch.pyin_geometry(22050, 256, 60., 500.) == (368, 51) == yr.geometry(22050, 256, 60., 500.)
    assert pitch.pyin_geometry(16000, 128, 50., 800., 5, 10.0) == yr.geometry(16000, 128, 50., 800., 5, 10.0)
    for bad in (dict(fmin=500., fmax=60.), dict(bps=0), dict(hop=0), dict(max_transition_rate=float('nan'))):
        with pytest.raises(ValueError):
            pitch.pyin_geometry(**dict(dict(rate=22050, hop=256, fmin=60., fmax=500.), **bad))


class _Engine:
    """a recording stand-in: notes the calls, returns planes that say who made them"""
    def __init__(self):
        self.calls = []

    def _planes(self, who, audio, lengths, kw):
        self.calls.append((who, kw))
        B, N = np.atleast_2d(audio).shape
        out = np.zeros((3, B, 1 + N // int(kw.get('hop', 256))), np.float32)
        out[0], out[1], out[2] = (100, 1, 2) if who == 'pitch' else (200, 3, 4)
        return out

    def pitch(self, audio, lengths=None, **kw):
        return self._planes('pitch', audio, lengths, kw)

    def pyin(self, audio, lengths=None, **kw):
        return self._planes('pyin', audio, lengths, kw)


def test_estimate_f0_chooses_the_method():
    from text_to_speech_amd import pitch
    eng, audio = _Engine(), np.zeros((2, 1000), np.float32)
    yin = pitch.estimate_f0(eng, audio, [1000, 300], threshold=0.2)
    assert eng.calls == [('pitch', dict(threshold=0.2))] and set(yin) == {'f0', 'period', 'aperiodicity', 'voiced', 'frames'}
    assert set(pitch.estimate_f0(eng, audio, method='yin')) == set(yin)
    got = pitch.estimate_f0(eng, audio, [1000, 300], method='pyin', switch_prob=0.02)
    assert eng.calls[-1] == ('pyin', dict(switch_prob=0.02))
    assert set(got) == {'f0', 'pitch', 'voiced_prob', 'voiced', 'frames'}
    assert np.all(got['f0'] == 200) and np.all(got['pitch'] == 3) and np.all(got['voiced_prob'] == 4) and got['voiced'].all()
    assert list(got['frames']) == [4, 2]
    with pytest.raises(ValueError, match='F0 method'):
        pitch.estimate_f0(eng, audio, method='swipe')
    only_yin = type('E', (), {'pitch': eng.pitch})()
    with pytest.raises(ValueError, match='pyin'):
        pitch.estimate_f0(only_yin, audio, method='pyin')


def test_f0_method_reaches_the_tracker_of_evaluate_synthesis(monkeypatch):
    import text_to_speech_amd.audio as audio_mod
    from test_pitch import _PitchRuntime, _Vocoder
    from text_to_speech_amd.tacotron2 import Tacotron2

    class Runtime(_PitchRuntime):
        """... that also has the second tracker"""
        def __init__(self, frames_of):
            super().__init__(frames_of)
            self.pyins = []

        def pyin(self, audio, lengths=None, **kw):
            out = super().pitch(audio, lengths, **kw)
            self.pyins.append(self.pitches.pop())
            return out

    rng = np.random.default_rng(6)
    items = [('Hello, World!', rng.standard_normal(9 * 256 + 17).astype(np.float32))]
    monkeypatch.setattr(audio_mod, 'load_audio', lambda data, rate=None, *, engine, **kw: np.asarray(data, np.float32))
    monkeypatch.setattr(audio_mod, 'load_mel', lambda data, rate=22050, *, engine, **kw: np.full((1 + len(data) // 256, 80), -4.0, np.float32))
    rt = Runtime(lambda n: n + 3)
    voc = _Vocoder(rt.to_host)
    model = Tacotron2(rt, lang='en')
    res = model.evaluate_synthesis(items, vocoder=voc, f0_method='pyin', pitch=dict(fmin=80.), f0_config=dict(switch_prob=0.02))
    assert res['names'] == Tacotron2.SYNTHESIS_NAMES + Tacotron2.SYNTHESIS_F0_NAMES and res['per_item'].shape == (10, 1)
    assert rt.pitches == [] and len(rt.pyins) == 2 and len(rt.f0s) == 1
    assert [kw for _, _, kw in rt.pyins] == [dict(fmin=80., switch_prob=0.02)] * 2
    assert rt.pyins[0][1].tolist() == [(len(model.encode_text(model.clean_text(items[0][0]), cleaned=True)) + 3) * 256]
    yin = model.evaluate_synthesis(items, vocoder=voc)                 # the default is the threshold tracker, with the values of before
    assert len(rt.pitches) == 2 and len(rt.pyins) == 2 and np.array_equal(yin['per_item'], res['per_item'])
    with pytest.raises(ValueError, match='f0_method must be one of'):
        model.evaluate_synthesis(items, vocoder=voc, f0_method='swipe')
    with pytest.raises(ValueError, match='f0_method= chooses the tracker of vocoder='):
        model.evaluate_synthesis(items, f0_method='pyin')
    with pytest.raises(ValueError, match='pyin and f0_error'):
        Tacotron2(_PitchRuntime(lambda n: n + 3), lang='en').evaluate_synthesis(items, vocoder=voc, f0_method='pyin')
    with pytest.raises(ValueError, match='hop must stay 256'):
        model.evaluate_synthesis(items, vocoder=voc, f0_method='pyin', f0_config=dict(hop=128))
