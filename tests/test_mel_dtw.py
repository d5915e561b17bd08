"""CPU: MCD along a DTW path without a GPU.

1. tests/mel_dtw_ref.py (the float64 restatement every GPU result is held to) against closed forms: D D^T = I, identical rows,
   r-fold repetition, the DP optimum against every enumerated monotone path for la, lb <= 5, the tie order.
2. The GPU test's bounds: a float32 numpy copy of the restatement stays inside every one of them on every case, each planted
   mistake moves its figure at least ten bounds on the case that shows it best, and the cases whose float64 path is decided by a
   margin (mel_dtw_cases.STABLE_PATHS) are exactly the ones found here.
3. The front end of tts_hip_mel_dtw / tts_hip_mel_dtw_probe in C++ (csrc/mel_dtw_call.h: mel_dtw_check, mel_dtw_layout,
   mel_dtw_dct) against a Python restatement written here, refusal by refusal, at each limit and on random calls.  The C++ side
   is csrc/host_check.cpp's --mel-dtw mode, a stand-alone program built with -fsanitize=address,undefined.
4. Every library call `HipEngine.mel_dtw` / `mel_dtw_probe` make for host arrays, on the recording stand-in of
   tests/test_engine_calls.py, with the expectations inline; bad arguments raise before any library call.
5. `metrics`, `Tacotron2.evaluate_synthesis` and `WaveGlow.copy_synthesis` on recording stand-in runtimes: batching, padding
   values, input order, the 0-frame row, `stopped`, and what crosses to the host.
"""
import itertools
import os
import re
import shutil
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import mel_dtw_cases as mc
import mel_dtw_ref as mr
from test_engine_calls import run as record_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
EINVAL = -1


# ---- 1. the restatement --------------------------------------------------------------------------------------------------------
def test_dct_rows_are_orthonormal():
    for n_mel in (2, 5, 80, 128):
        D = mr.dct_table(n_mel, n_mel - 1, c0=True, rounded=False)
        assert D.shape == (n_mel, n_mel) and np.allclose(D @ D.T, np.eye(n_mel), rtol=0, atol=1e-13)
        assert np.array_equal(mr.dct_table(n_mel, n_mel - 1, rounded=False), D[1:])             # without c0: rows 1 ..
    assert np.allclose(mr.dct_table(80, 13, c0=True, rounded=False)[0], 1 / np.sqrt(80), rtol=1e-15)
    assert np.abs(mr.dct_table(80, 13) - mr.dct_table(80, 13, rounded=False)).max() <= mr.EPS * np.sqrt(2 / 80)


def test_identical_and_repeated_rows_cost_nothing_along_the_known_path():
    a = mc.log_mel(np.random.default_rng(1), 7)
    out = mr.mel_dtw(a, a.copy())
    assert np.array_equal(out['stats'], [0, 7, 0]) and out['path'] == [(t, t) for t in range(7)]
    for r in (2, 3):
        out = mr.mel_dtw(a, np.repeat(a, r, axis=0))
        assert np.array_equal(out['stats'], [0, 7 * r, 0])
        assert out['path'] == [(j // r, j) for j in range(7 * r)]
        back = mr.mel_dtw(np.repeat(a, r, axis=0), a)                                         # and the other way round
        assert np.array_equal(back['stats'], [0, 7 * r, 0]) and back['path'] == [(i, i // r) for i in range(7 * r)]
    assert mr.mel_dtw(a[:3], np.repeat(a[:3], 2, axis=0))['path'] == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]   # by hand
    # without alignment: the diagonal below the shorter length
    un = mr.mel_dtw(a, a[:4] + np.float32(1), align=False)
    assert un['path'] == [(t, t) for t in range(4)] and un['stats'][1] == 4
    d = mr.distance(un['cepstra_a'], un['cepstra_b'])
    assert un['stats'][0] == pytest.approx(sum(d[t, t] for t in range(4)), rel=1e-15)
    assert un['stats'][2] == pytest.approx(10 * np.sqrt(2) / np.log(10) * un['stats'][0] / 4, rel=1e-15)
    # a constant offset o of every channel moves only c0: sqrt(n_mel) o per frame
    c0 = mr.mel_dtw(a, a + np.float32(1), c0=True, align=False)
    assert np.allclose(np.diag(c0['distance']), np.sqrt(80.0), rtol=1e-6) and np.allclose(np.diag(un['distance'][:4, :4]), 0, atol=1e-5)


def test_dp_optimum_is_the_minimum_over_every_monotone_path():
    rng = np.random.default_rng(2)
    for la, lb in itertools.product(range(1, 6), repeat=2):
        d = rng.uniform(0.1, 5.0, (la, lb))
        C, step = mr.accumulate(d)
        assert C[-1, -1] == pytest.approx(mr.enumerate_optimum(d), rel=1e-14), (la, lb)
        path = mr.backtrack(step)
        assert path[0] == (0, 0) and path[-1] == (la - 1, lb - 1) and max(la, lb) <= len(path) <= la + lb - 1
        assert all((i1 - i0, j1 - j0) in ((1, 1), (1, 0), (0, 1)) for (i0, j0), (i1, j1) in zip(path, path[1:]))
        assert sum(d[i, j] for i, j in path) == pytest.approx(C[-1, -1], rel=1e-14)
        assert np.array_equal(step, mr.argmin_codes(C))


def test_ties_resolve_diagonal_then_up_then_left():
    C, step = mr.accumulate(np.ones((3, 3)))                      # C = [[1, 2, 3], [2, 2, 3], [3, 3, 3]]
    assert C.tolist() == [[1, 2, 3], [2, 2, 3], [3, 3, 3]]
    # (1, 2): diagonal 2 = left 2 < up 3 -> diagonal; (2, 1): diagonal 2 = up 2 < left 3 -> diagonal; the first row and column
    # have one neighbour each
    assert step.tolist() == [[0, 2, 2], [1, 0, 0], [1, 0, 0]] and mr.backtrack(step) == [(0, 0), (1, 1), (2, 2)]
    # up = left = 3 below the diagonal's 10: up
    C, step = mr.accumulate(np.array([[1.0, 1.0, 2.0], [1.0, 9.0, 1.0], [2.0, 1.0, 1.0]]))
    assert (C[1, 1], C[1, 2], C[2, 1]) == (10, 3, 3) and step[2, 2] == 1 and C[2, 2] == 4
    # and each of the three by value alone
    assert mr.accumulate(np.array([[1.0, 9.0], [1.0, 1.0]]))[1][1, 1] == 0       # diagonal 1, up 10, left 2
    C, step = mr.accumulate(np.array([[1.0, 1.0, 1.0], [9.0, 9.0, 1.0]]))          # (1, 2): diagonal 2, up 3, left 11
    assert step[1, 2] == 0
    C, step = mr.accumulate(np.array([[1.0, 9.0, 1.0], [1.0, 1.0, 1.0]]))          # (1, 2): diagonal 10, up 11, left 2
    assert (C[0, 1], C[0, 2], C[1, 1]) == (10, 11, 2) and step[1, 2] == 2
    C, step = mr.accumulate(np.array([[1.0, 1.0], [9.0, 1.0], [1.0, 1.0]]))        # (2, 1): diagonal 10, up 2, left 11
    assert (C[1, 0], C[1, 1], C[2, 0]) == (10, 2, 11) and step[2, 1] == 1
    assert mr.argmin_codes(np.full((2, 2), 7.0)).tolist() == [[0, 2], [1, 0]]


# ---- 2. the bounds ---------------------------------------------------------------------------------------------------------------
def _inside_every_bound(name):
    """The GPU test's stage checks applied to the float32 copy of the restatement -> the largest error / bound of each."""
    a, b = mc.pair(name)
    la, lb, _, n_mel, n_cep, c0 = mc.CASES[name]
    f = mr.mel_dtw(a, b, n_cep=n_cep, c0=c0, dtype=np.float32)
    D = mr.dct_table(n_mel, n_cep, c0)
    worst = {}
    for key, m in (('cepstra_a', a), ('cepstra_b', b)):
        worst[key] = (np.abs(f[key].astype(np.float64) - mr.cepstra(m, D)) / mr.cepstra_bound(m, D)).max()
    ca, cb = f['cepstra_a'].astype(np.float64), f['cepstra_b'].astype(np.float64)
    ref_d = mr.distance(ca, cb)
    worst['distance'] = (np.abs(f['distance'] - ref_d) / np.maximum((n_cep + 4) * mr.EPS * ref_d, 1e-300)).max()
    ref_C, _ = mr.accumulate(f['distance'].astype(np.float64))
    ij = np.add.outer(np.arange(la), np.arange(lb)) + 1
    worst['cost'] = (np.abs(f['cost'] - ref_C) / np.maximum(ij * mr.EPS * ref_C, 1e-300)).max()
    assert np.array_equal(f['step'], mr.argmin_codes(f['cost']))
    ref = mr.mel_dtw(a, b, n_cep=n_cep, c0=c0, cepstra_in=(ca, cb))['stats'][0]
    worst['end to end'] = abs(f['stats'][0] - ref) / max(mr.cost_bound(n_cep, la, lb, ref), 1e-300)
    return worst


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_float32_copy_of_the_restatement_is_inside_every_gpu_bound(name):
    worst = _inside_every_bound(name)
    print(name, {k: f'{v:.3g}' for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# the case that shows each planted mistake best, and the figure it moves: the cost (0) or the MCD (2)
CAUGHT_BY = {'c0 kept': ('97x130_warped', 0), 'dct without the half sample': ('97x130_warped', 0),
             'one coefficient short': ('97x130_warped', 0), 'sqrt missing': ('97x130_warped', 0),
             'no diagonal step': ('97x130_warped', 0), 'diagonal counted twice': ('97x130_warped', 0),
             'pad frames included': ('40x52_warped_c0', 0),      # (a constant pad frame has only a c0)
             'last frame dropped': ('97x130_warped', 0), 'ln instead of log10': ('97x130_warped', 2)}


@pytest.mark.parametrize('mistake', mr.MISTAKES)
def test_gpu_bound_is_a_tenth_of_every_planted_mistake(mistake):
    name, figure = CAUGHT_BY[mistake]
    a, b = mc.pair(name)
    la, lb, _, _, n_cep, c0 = mc.CASES[name]
    # as in a batch: the synthesized mel padded with zeros behind its frames, the target with the vocoder's padding value
    pa, pb = np.concatenate([a, np.zeros((6, a.shape[1]), np.float32)]), np.concatenate([b, np.full((3, b.shape[1]), -11, np.float32)])
    ref = mr.mel_dtw(pa, pb, la, lb, n_cep, c0)['stats']
    assert np.array_equal(ref, mr.mel_dtw(a, b, n_cep=n_cep, c0=c0)['stats'])                  # the pads are not read
    wrong = mr.mel_dtw(pa, pb, la, lb, n_cep, c0, mistake=mistake)['stats']
    bound = mr.cost_bound(n_cep, la, lb, ref[0])
    if figure == 2:                                               # the MCD's bound: the cost's, scaled, plus its two roundings
        bound = mr.MCD_DB_FACTOR * bound / ref[1] + 2 * mr.EPS * ref[2]
    effect = abs(wrong[figure] - ref[figure]) / bound
    print(f'{mistake}: effect / bound = {effect:.3g}')
    assert effect >= 10.0, (mistake, effect)
    assert set(CAUGHT_BY) == set(mr.MISTAKES)


def test_stable_paths_are_the_cases_decided_by_a_margin():
    stable = []
    for name, (la, lb, kind, _, n_cep, c0) in mc.CASES.items():
        out = mr.mel_dtw(*mc.pair(name), n_cep=n_cep, c0=c0)
        if mr.margin_along(out['cost'], out['path']) > 2 * mr.cost_bound(n_cep, la, lb, out['stats'][0]):
            stable.append(name)
            f32 = mr.mel_dtw(*mc.pair(name), n_cep=n_cep, c0=c0, dtype=np.float32)
            assert f32['path'] == out['path'], name               # and there the float32 copy walks the same path
    assert tuple(stable) == mc.STABLE_PATHS and len(stable) >= 4
    assert all(n in stable for n, c in mc.CASES.items() if c[2] in ('identical', 'repeat'))
    assert set(mc.RAGGED) <= set(mc.CASES) and all(mc.CASES[n][3:] == (80, 13, False) for n in mc.RAGGED)


def test_cases_are_log_mel_like():
    for name in mc.CASES:
        a, b = mc.pair(name)
        la, lb, _, n_mel, _, _ = mc.CASES[name]
        assert a.shape == (la, n_mel) and b.shape == (lb, n_mel) and a.dtype == b.dtype == np.float32
        assert min(a.min(), b.min()) >= np.float32(mc.LOG_FLOOR) and max(a.max(), b.max()) <= mc.LOG_CEIL
    a = mc.log_mel(np.random.default_rng(3), 400)
    assert np.abs(np.diff(a, axis=0)).mean() < 0.5 * np.abs(a - a.mean(axis=0)).mean()       # smooth in time
    x, y, la, lb = mc.ragged_batch()
    assert all(np.isnan(x[r, la[r]:]).all() and np.isfinite(x[r, :la[r]]).all() for r in range(5)) and np.isnan(y).any()


# ---- 3. the call's front end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    return os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')


GOOD = dict(B=3, Ta=40, Tb=52, n_mel=80, n_cep=13, flags=1, mem=0, probe=0, what=-1, path=0, null='', la=None, lb=None)
MAX_FRAMES, MAX_CELLS, MAX_ROW_FRAMES = 8192, 1 << 25, 1 << 19


def _call(exe, s, dct=False):
    """-> (status, message, [R, W, K, skew_i, aligned] or None, the fourteen layout numbers or None, the DCT values)"""
    args = [f'{k}={v}' for k, v in s.items() if k not in ('null', 'la', 'lb')]
    args += [f'{k}=' + ','.join(str(v) for v in s[k]) for k in ('la', 'lb') if s[k] is not None]
    args += [f"null={s['null']}"] if s['null'] else []
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, '--mel-dtw'] + args + (['dct=1'] if dct else []), capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    rc, _, msg = lines[0].partition(' ')
    if len(lines) == 1:
        return int(rc), msg, None, None, None
    return int(rc), msg, [int(v) for v in lines[1].split()], [int(v) for v in lines[2].split()], [float(v) for v in lines[3:]]


def dtw_check(s):
    """mel_dtw_check restated -> (status, message)"""
    for name in ('a', 'b', 'out' if s['probe'] else 'stats'):
        if name in s['null'].split(','):
            return EINVAL, f'{name} is NULL'
    for name in ('B', 'Ta', 'Tb'):
        if s[name] < 1:
            return EINVAL, f'{name} = {s[name]} must be at least 1'
    if not 2 <= s['n_mel'] <= 128:
        return EINVAL, f"n_mel = {s['n_mel']} is outside [2, 128]"
    if not 1 <= s['n_cep'] <= s['n_mel'] - 1:
        return EINVAL, f"n_cep = {s['n_cep']} is outside [1, n_mel - 1 = {s['n_mel'] - 1}]"
    if s['flags'] & ~3:
        return EINVAL, f"flags = {s['flags']} holds unknown bits (1 align, 2 c0)"
    if s['mem'] not in (0, 1):
        return EINVAL, f"bad mem kind {s['mem']}"
    if s['probe'] and not 0 <= s['what'] <= 4:
        return EINVAL, f"what = {s['what']} is no stage (0 cepstra_a, 1 cepstra_b, 2 distance, 3 cost, 4 step)"
    for key, T in (('la', 'Ta'), ('lb', 'Tb')):
        for row, n in enumerate((s[key] or [])[:s['B']]):
            if not 1 <= n <= s[T]:
                return EINVAL, f'len_{key[1]}[{row}] = {n} is outside [1, {T} = {s[T]}]'
    if s['Ta'] > MAX_FRAMES or s['Tb'] > MAX_FRAMES:
        return EINVAL, f"Ta = {s['Ta']}, Tb = {s['Tb']}: above {MAX_FRAMES} frames"
    if s['B'] * s['Ta'] * s['Tb'] > MAX_CELLS:
        return EINVAL, f"B*Ta*Tb too large (B = {s['B']}, Ta = {s['Ta']}, Tb = {s['Tb']}: above {MAX_CELLS} cells); split the batch"
    if s['B'] * (s['Ta'] + s['Tb']) > MAX_ROW_FRAMES:
        return EINVAL, f"B*(Ta+Tb) too large (B = {s['B']}, Ta = {s['Ta']}, Tb = {s['Tb']}: above {MAX_ROW_FRAMES} frames); split the batch"
    return 0, ''


def dtw_layout(s):
    """mel_dtw_layout restated -> ([R, W, K, skew_i, aligned], [the thirteen offsets, out_elems, bytes])"""
    B, Ta, Tb, n_mel = s['B'], s['Ta'], s['Tb'], s['n_mel']
    R, W, K = s['n_cep'] + (1 if s['flags'] & 2 else 0), min(Ta, Tb), Ta + Tb - 1
    probe, host = bool(s['probe']), s['mem'] == 0
    aligned = s['what'] >= 2 if probe else bool(s['flags'] & 1)
    out_elems = 0 if not probe else B * Ta * R if s['what'] == 0 else B * Tb * R if s['what'] == 1 else B * Ta * Tb
    sizes = [B * Ta * n_mel * 4 * host, B * Tb * n_mel * 4 * host, 2 * B * 4, B * Ta * R * 4, B * Tb * R * 4, B * K * W * 4 * aligned,
             B * K * W * aligned, B * K * W * 4 * (probe and s['what'] == 3), B * 4 * aligned, 3 * B * 4 * (host and not probe),
             B * K * 2 * 4 * (host and not probe and bool(s['path'])), out_elems * 4 * host]
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += (n + 255) // 256 * 256
    return [R, W, K, int(Ta < Tb), int(aligned)], offsets + [out_elems, at]


def test_front_end_refuses_by_name_before_any_gpu_work(checker):
    refusals = [
        (dict(null='a'), 'a is NULL'), (dict(null='b'), 'b is NULL'), (dict(null='stats'), 'stats is NULL'),
        (dict(null='out', probe=1, what=3), 'out is NULL'),
        (dict(B=0), 'B = 0 must be at least 1'), (dict(Ta=0), 'Ta = 0 must be at least 1'), (dict(Tb=-2), 'Tb = -2 must be at least 1'),
        (dict(n_mel=1, n_cep=1), 'n_mel = 1 is outside [2, 128]'), (dict(n_mel=129), 'n_mel = 129 is outside [2, 128]'),
        (dict(n_cep=0), 'n_cep = 0 is outside [1, n_mel - 1 = 79]'), (dict(n_cep=80), 'n_cep = 80 is outside [1, n_mel - 1 = 79]'),
        (dict(flags=4), 'flags = 4 holds unknown bits (1 align, 2 c0)'), (dict(flags=-1), 'flags = -1 holds unknown bits (1 align, 2 c0)'),
        (dict(mem=2), 'bad mem kind 2'), (dict(mem=-1), 'bad mem kind -1'),
        (dict(probe=1, what=5), 'what = 5 is no stage (0 cepstra_a, 1 cepstra_b, 2 distance, 3 cost, 4 step)'),
        (dict(probe=1, what=-1), 'what = -1 is no stage (0 cepstra_a, 1 cepstra_b, 2 distance, 3 cost, 4 step)'),
        (dict(la=[40, 0, 1]), 'len_a[1] = 0 is outside [1, Ta = 40]'), (dict(la=[41, 1, 1]), 'len_a[0] = 41 is outside [1, Ta = 40]'),
        (dict(lb=[1, 1, 53]), 'len_b[2] = 53 is outside [1, Tb = 52]'), (dict(lb=[-3, 1, 1]), 'len_b[0] = -3 is outside [1, Tb = 52]'),
        (dict(B=1, Ta=8193, Tb=1), 'Ta = 8193, Tb = 1: above 8192 frames'), (dict(B=1, Ta=1, Tb=8193), 'Ta = 1, Tb = 8193: above 8192 frames'),
        (dict(B=1, Ta=8192, Tb=4097), 'B*Ta*Tb too large (B = 1, Ta = 8192, Tb = 4097: above 33554432 cells); split the batch'),
        (dict(B=2147483647, Ta=8192, Tb=8192), 'B*Ta*Tb too large (B = 2147483647, Ta = 8192, Tb = 8192: above 33554432 cells); split the batch'),
        (dict(B=65, Ta=8192, Tb=1), 'B*(Ta+Tb) too large (B = 65, Ta = 8192, Tb = 1: above 524288 frames); split the batch'),
        (dict(B=4096, Ta=8192, Tb=1, n_mel=128, n_cep=127, mem=0),
         'B*(Ta+Tb) too large (B = 4096, Ta = 8192, Tb = 1: above 524288 frames); split the batch'),
        (dict(B=(1 << 18) + 1, Ta=1, Tb=1), 'B*(Ta+Tb) too large (B = 262145, Ta = 1, Tb = 1: above 524288 frames); split the batch'),
        # first match wins, in the documented order
        (dict(null='stats,b', B=0), 'b is NULL'), (dict(B=0, Ta=0, n_mel=1), 'B = 0 must be at least 1'),
        (dict(n_mel=1, n_cep=0, flags=8), 'n_mel = 1 is outside [2, 128]'), (dict(n_cep=0, flags=8, mem=3), 'n_cep = 0 is outside [1, n_mel - 1 = 79]'),
        (dict(flags=8, mem=3, la=[0, 0, 0]), 'flags = 8 holds unknown bits (1 align, 2 c0)'), (dict(mem=3, la=[0, 0, 0]), 'bad mem kind 3'),
        (dict(la=[1, 1, 99], lb=[0, 1, 1]), 'len_a[2] = 99 is outside [1, Ta = 40]'),
        (dict(B=1, Ta=8193, Tb=8193, la=[8193], lb=[9000]), 'len_b[0] = 9000 is outside [1, Tb = 8193]'),
        (dict(B=9, Ta=8193, Tb=8192), 'Ta = 8193, Tb = 8192: above 8192 frames'),
    ]
    seen = set()
    for wrong, msg in refusals:
        s = dict(GOOD, **wrong)
        rc, why, *rest = _call(checker, s)
        assert (rc, why, rest) == (EINVAL, 'who: ' + msg, [None] * 3), (wrong, rc, why)
        assert dtw_check(s) == (EINVAL, msg), wrong
        seen.add(re.sub(r'-?\d+', '#', re.sub(r'^(len_)?\w+( is NULL)?', r'\2', msg)))
    assert len(seen) >= 9, sorted(seen)                             # one message per kind of refusal


def test_front_end_accepts_and_sizes_at_the_limits(checker):
    for wrong in [dict(), dict(B=1, Ta=1, Tb=1, n_mel=2, n_cep=1), dict(n_mel=128, n_cep=127, flags=3), dict(flags=0), dict(flags=2, path=1),
                  dict(B=1, Ta=8192, Tb=4096), dict(B=1, Ta=4096, Tb=8192, mem=1, path=1), dict(B=1 << 18, Ta=1, Tb=1, mem=1), dict(B=64, Ta=8191, Tb=1), dict(B=64, Ta=1, Tb=8191, mem=1, path=1),
                  dict(B=8, Ta=2048, Tb=2048, mem=1), dict(B=8, Ta=800, Tb=900, mem=1, path=1),
                  dict(la=[1, 40, 7], lb=[52, 1, 9]), dict(la=[1, 40, 7]), dict(mem=1, path=1), dict(mem=0, path=1),
                  *(dict(probe=1, what=w, mem=m) for w in range(5) for m in (0, 1))]:
        s = dict(GOOD, **wrong)
        rc, why, shape, layout, _ = _call(checker, s)
        assert (rc, why) == (0, '') == dtw_check(s), (wrong, why)
        assert (shape, layout) == tuple(dtw_layout(s)), wrong
        assert all(v % 256 == 0 for v in layout[:12] + layout[13:])
    # the workspace the cell limit implies: ten bytes a cell for the aligned programme
    shape, layout = dtw_layout(dict(GOOD, B=8, Ta=2048, Tb=2048, mem=1))
    assert 8 * 2048 * 2048 == MAX_CELLS and shape[1:3] == [2048, 4095] and layout[-1] <= 10 * MAX_CELLS + 8 * 4096 * 14 * 4 + 4096
    assert dtw_layout(dict(GOOD, B=8, Ta=800, Tb=900, mem=1))[0] == [13, 800, 1699, 1, 1]
    # ... and what the frame limit adds for the thinnest and the widest accepted calls: cepstra and staged mels of 128 floats a frame
    MiB = 1 << 20
    for thin in (dict(B=64, Ta=8191, Tb=1), dict(B=1 << 18, Ta=1, Tb=1), dict(B=32, Ta=8192, Tb=8192 // 64), dict(B=8, Ta=2048, Tb=2048)):
        s = dict(GOOD, n_mel=128, n_cep=127, flags=3, mem=0, path=1, **thin)
        assert dtw_check(s) == (0, '') and dtw_layout(s)[1][-1] <= (320 + 256 + 256 + 8) * MiB, thin
        assert _call(checker, s)[3] == dtw_layout(s)[1]


def test_front_end_equals_its_restatement_on_random_calls(checker):
    rng = np.random.default_rng(22)
    pick = lambda *pool: pool[int(rng.integers(len(pool)))]
    seen = set()
    for _ in range(250):
        B = pick(3, 3, 1, 8, 0, -1)
        s = dict(B=B, Ta=pick(40, 40, 1, 8192, 8193, 0, 900), Tb=pick(52, 52, 1, 4096, 4097, -1, 800), n_mel=pick(80, 80, 128, 2, 1, 129),
                 n_cep=pick(13, 13, 1, 79, 127, 0, 128), flags=pick(1, 1, 0, 2, 3, 4, -2), mem=pick(0, 1, 1, 5), probe=pick(0, 0, 1),
                 what=pick(-1, 0, 1, 2, 3, 4, 5), path=pick(0, 1), null=','.join(n for n in ('a', 'b', 'stats', 'out') if rng.random() < 0.04),
                 la=pick(None, None, [int(pick(1, 1, 40, 41, 0, 8192)) for _ in range(max(B, 0))]),
                 lb=pick(None, None, [int(pick(1, 1, 52, 53, -1, 4096)) for _ in range(max(B, 0))]))
        want = dtw_check(s)
        rc, why, shape, layout, _ = _call(checker, s)
        assert (rc, why) == (want[0], 'who: ' + want[1] if want[0] else ''), (s, rc, why)
        assert (shape, layout) == (tuple(dtw_layout(s)) if rc == 0 else (None, None)), s
        seen.add(re.sub(r'-?\d+', '#', why))
    assert '' in seen and len(seen) >= 10, sorted(seen)


def test_dct_table_of_the_library_is_the_restatements(checker):
    for n_mel, n_cep, flags in ((80, 13, 1), (80, 13, 3), (128, 127, 3), (2, 1, 0), (5, 4, 2)):
        *_, values = _call(checker, dict(GOOD, n_mel=n_mel, n_cep=n_cep, flags=flags), dct=True)
        want = mr.dct_table(n_mel, n_cep, bool(flags & 2))
        got = np.asarray(values, np.float32).reshape(want.shape)
        # float64 cosines of two libraries may differ in the last place: at most one float32 step, where the rounding flips
        assert np.abs(got.astype(np.float64) - want).max() <= 2 * mr.EPS * np.sqrt(2 / n_mel) and np.mean(got == want.astype(np.float32)) > 0.99


# ---- 4. the bindings' library calls ----------------------------------------------------------------------------------------------
def _sha(array):
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(array).tobytes()).hexdigest()[:12]


def test_library_calls_of_the_bindings():
    a, b, la, lb = mc.ragged_batch()
    arr = lambda x, dtype: {'dtype': dtype, 'shape': list(x.shape), 'sha': _sha(x.astype(dtype))}
    calls = record_calls(lambda e: e.mel_dtw(a.astype(np.float64), b, la.tolist(), lb.astype(np.int64), return_path=True))
    assert calls == [['mel_dtw', ['engine', arr(a, 'float32'), arr(b, 'float32'), 5, 97, 257, 80, arr(la, 'int32'), arr(lb, 'int32'), 13, 1,
                                  {'dtype': 'float32', 'shape': [3, 5]}, {'dtype': 'int32', 'shape': [5, 353, 2]}, 0, None]]]
    calls = record_calls(lambda e: e.mel_dtw(a[0], b[0], n_cep=20, include_c0=True, align=False))       # one row, no batch axis
    assert calls == [['mel_dtw', ['engine', arr(a[:1], 'float32'), arr(b[:1], 'float32'), 1, 97, 257, 80, None, None, 20, 2,
                                  {'dtype': 'float32', 'shape': [3, 1]}, None, 0, None]]]
    for what, code, shape in (('cepstra_a', 0, [5, 97, 14]), ('cepstra_b', 1, [5, 257, 14]), ('distance', 2, [5, 97, 257]),
                              ('cost', 3, [5, 97, 257]), ('step', 4, [5, 97, 257])):
        calls = record_calls(lambda e: e.mel_dtw_probe(a, b, la, None, include_c0=True, what=what))
        assert calls == [['mel_dtw_probe', ['engine', arr(a, 'float32'), arr(b, 'float32'), 5, 97, 257, 80, arr(la, 'int32'), None, 13, 3,
                                            code, {'dtype': 'float32', 'shape': shape}, 0, None]]], what


REFUSALS = {
    'stream': (lambda e, a, b: e.mel_dtw(a, b, stream=object()), 'stream= needs device tensors'),
    'rank': (lambda e, a, b: e.mel_dtw(a[0, 0], b), r'mel_dtw: a and b must be \[B, Ta, n_mel\]'),
    'mixed_rank': (lambda e, a, b: e.mel_dtw(a[0], b), r'mel_dtw: a and b must be'),
    'rows': (lambda e, a, b: e.mel_dtw(a[:2], b), r'mel_dtw: a and b must be'),
    'channels': (lambda e, a, b: e.mel_dtw(a[..., :79], b), r'mel_dtw: a and b must be'),
    'empty': (lambda e, a, b: e.mel_dtw(a[:, :0], b), r'mel_dtw: a and b must be'),
    'n_mel': (lambda e, a, b: e.mel_dtw(a[..., :1], b[..., :1]), r'n_mel = 1 is outside \[2, 128\]'),
    'n_cep': (lambda e, a, b: e.mel_dtw(a, b, n_cep=80), r'n_cep = 80 is outside \[1, n_mel - 1 = 79\]'),
    'n_cep_float': (lambda e, a, b: e.mel_dtw(a, b, n_cep=12.5), 'n_cep = 12.5 is outside'),
    'lengths_shape': (lambda e, a, b: e.mel_dtw(a, b, [4, 4]), r'mel_dtw: lengths_a must hold one value per row, shape \(3,\)'),
    'lengths_low': (lambda e, a, b: e.mel_dtw(a, b, [4, 0, 4]), r'mel_dtw: lengths_a must lie in \[1, 6\]'),
    'lengths_high': (lambda e, a, b: e.mel_dtw(a, b, None, [9, 10, 1]), r'mel_dtw: lengths_b must lie in \[1, 9\]'),
    'lengths_float': (lambda e, a, b: e.mel_dtw(a, b, [4., 4., 4.]), 'mel_dtw: lengths_a must be integers'),
    'probe_what': (lambda e, a, b: e.mel_dtw_probe(a, b, what='path'), 'what must be one of'),
    'probe_lengths': (lambda e, a, b: e.mel_dtw_probe(a, b, None, [0, 1, 1]), r'mel_dtw_probe: lengths_b must lie in \[1, 9\]'),
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_a_bad_argument_raises_before_any_library_call(name):
    case, match = REFUSALS[name]
    a, b = np.zeros((3, 6, 80), np.float32), np.zeros((3, 9, 80), np.float32)
    calls = None

    def guarded(eng):
        nonlocal calls
        calls = eng._lib.calls
        with pytest.raises(ValueError, match=match):
            case(eng, a, b)

    record_calls(guarded)
    assert calls == []


# ---- 5. host logic on recording stand-ins ---------------------------------------------------------------------------------------
class _Dev:
    """Stands for a CUDA tensor: whatever is brought to the host is written down."""

    def __init__(self, array, log):
        self.array, self.log, self.shape = array, log, array.shape

    def detach(self):
        return self

    def cpu(self):
        self.log.append(tuple(self.array.shape))
        return self

    def numpy(self):
        return self.array

    def __getitem__(self, idx):
        return _Dev(self.array[idx], self.log)


def _fake_stats(a, b, la, lb, **kw):
    return np.stack([mr.mel_dtw(a[r], b[r], la[r], lb[r], n_cep=kw.get('n_cep', 13), align=kw.get('align', True))['stats']
                     for r in range(len(a))], axis=1).astype(np.float32)


class _SynthRuntime:
    """Stands for HipRuntime behind a Tacotron2: the decode answers `frames_of[text length]` frames per row, the DTW call the
    restatement."""
    Out = namedtuple('Out', ['decoder_output', 'mel', 'stop_tokens', 'attention_weights', 'lengths'])

    def __init__(self, frames_of):
        self.frames_of, self.infers, self.dtws, self.to_host = frames_of, [], [], []

    def __call__(self, inputs, **kwargs):
        tokens = inputs[0] if isinstance(inputs, tuple) else inputs
        self.infers.append((inputs, kwargs))
        n_tok = (tokens != 0).sum(axis=1)
        cap = int(np.float32(n_tok.max()) * np.float32(kwargs['max_length']))
        lengths = np.asarray([min(self.frames_of(int(n)), cap) for n in n_tok], np.int32)
        mel = -5 + np.sin(np.arange(len(tokens) * cap * 80, dtype=np.float32).reshape(len(tokens), cap, 80) * np.float32(0.37))
        return self.Out(None, _Dev(mel, self.to_host), None, None, _Dev(lengths, self.to_host))

    def mel_dtw(self, a, b, lengths_a=None, lengths_b=None, **kwargs):
        self.dtws.append((a, b, lengths_a, lengths_b, kwargs))
        return _Dev(_fake_stats(a.array, b, lengths_a, lengths_b, **kwargs), self.to_host)


def test_evaluate_synthesis_batches_pads_and_reports():
    from text_to_speech_amd.tacotron2 import SV2TTSTacotron2, Tacotron2
    rng = np.random.default_rng(6)
    texts = ['Hello, World!', 'Hi', 'A somewhat longer sentence.', 'Good morning', 'Bye']
    mels = [mc.log_mel(rng, n) for n in (9, 4, 30, 1, 6)]
    toks = [np.asarray(Tacotron2(None).encode_text(Tacotron2(None).clean_text(t), cleaned=True), np.int32) for t in texts]
    n_tok = [len(t) for t in toks]
    # 'Hi' stops at once with no frame, 'Bye' runs into the cap of its batch (it is alone: 2 frames per token), the rest stop early
    frames_of = lambda n: {n_tok[1]: 0, n_tok[4]: 10 ** 6}.get(n, n + 3)
    rt = _SynthRuntime(frames_of)
    model = Tacotron2(rt, lang='en')
    model.pad_mel_value = -11.
    res = model.evaluate_synthesis(list(zip(texts, mels)), batch_size=2, max_length=2., n_cep=12)
    assert res['names'] == Tacotron2.SYNTHESIS_NAMES == ['mcd_dtw', 'path_len', 'frames', 'target_frames', 'frame_ratio', 'stopped']
    per = res['per_item']
    assert per.shape == (6, 5) and per.dtype == np.float32
    assert [len(i) for i, _ in rt.infers] == [2, 2, 1] and len(rt.dtws) == 3                # batch boundaries, in input order
    want_frames = []
    for call, ((tok, kwargs), (a, b, la, lb, kw)) in enumerate(zip(rt.infers, rt.dtws)):
        rows = list(range(2 * call, min(2 * call + 2, 5)))
        Tin, T = max(n_tok[i] for i in rows), max(len(mels[i]) for i in rows)
        assert kwargs == {'max_length': 2., 'deterministic': True, 'on_device': True} and kw == {'n_cep': 12}
        assert tok.shape == (len(rows), Tin) and tok.dtype == np.int32
        for r, i in enumerate(rows):
            assert np.array_equal(tok[r, :n_tok[i]], toks[i]) and np.all(tok[r, n_tok[i]:] == 0)      # 0-padded
        cap = 2 * Tin
        frames = [min(frames_of(n_tok[i]), cap) for i in rows]
        want_frames += frames
        keep = [r for r, n in enumerate(frames) if n > 0]
        assert isinstance(a, _Dev) and a.shape == (len(keep), cap, 80)                             # the mel never left the device ...
        assert isinstance(b, np.ndarray) and b.shape == (len(keep), T, 80) and b.dtype == np.float32
        assert la.dtype == lb.dtype == np.int32 and la.tolist() == [frames[r] for r in keep]
        assert lb.tolist() == [len(mels[rows[r]]) for r in keep]
        for k, r in enumerate(keep):
            n = len(mels[rows[r]])
            assert np.array_equal(b[k, :n], mels[rows[r]]) and np.all(b[k, n:] == -11.)              # the model's padding value
        stats = _fake_stats(a.array, b, la, lb, n_cep=12)
        assert np.array_equal(per[0, [rows[r] for r in keep]], stats[2]) and np.array_equal(per[1, [rows[r] for r in keep]], stats[1])
        assert per[5, rows].tolist() == [float(n < cap) for n in frames]
    # ... and only the lengths [B] and the statistics [3, rows that produced frames] came to the host
    assert rt.to_host == [(2,), (3, 1), (2,), (3, 2), (1,), (3, 1)]
    assert per[2].tolist() == want_frames and per[3].tolist() == [9, 4, 30, 1, 6]
    assert want_frames[1] == 0 and want_frames[4] == 2 * n_tok[4]
    assert np.isnan(per[[0, 1, 4], 1]).all() and per[2, 1] == 0 and per[3, 1] == 4 and per[5, 1] == 1   # the 0-frame row
    assert per[5].tolist() == [1, 1, 1, 1, 0]                                                         # 'Bye' ran into its cap
    ok = [0, 2, 3, 4]
    assert np.isfinite(per[:, ok]).all() and np.array_equal(per[4, ok], (per[2, ok].astype(np.float64) / per[3, ok]).astype(np.float32))
    assert set(res['mean']) == set(res['names'])
    for k, name in enumerate(res['names']):                                                           # the 0-frame row is not in the means
        assert isinstance(res['mean'][name], float) and res['mean'][name] == pytest.approx(float(per[k, ok].astype(np.float64).mean()), rel=1e-12)
    # defaults: batches of 8, ten frames per token, 13 coefficients, the model's own padding value (0)
    rt2 = _SynthRuntime(lambda n: n + 3)
    out = Tacotron2(rt2, lang='en').evaluate_synthesis(list(zip(texts, mels)), deterministic=False)
    assert len(rt2.infers) == 1 and rt2.infers[0][1] == {'max_length': 10., 'deterministic': False, 'on_device': True}
    assert rt2.dtws[0][4] == {'n_cep': 13} and rt2.dtws[0][0] is not None and np.all(rt2.dtws[0][1][1, 4:] == 0.)
    assert out['per_item'].shape == (6, 5) and np.isfinite(out['per_item']).all() and np.all(out['per_item'][5] == 1)
    # every row without frames: no DTW call, NaN means
    rt3 = _SynthRuntime(lambda n: 0)
    out = Tacotron2(rt3, lang='en').evaluate_synthesis(list(zip(texts[:2], mels[:2])))
    assert rt3.dtws == [] and np.isnan(out['mean']['mcd_dtw']) and out['per_item'][2].tolist() == [0, 0]
    # refusals
    with pytest.raises(ValueError, match=r'items\[1\]: the text encodes to no token'):
        model.evaluate_synthesis([(texts[0], mels[0]), ('', mels[1])])
    with pytest.raises(ValueError, match='at least one item'):
        model.evaluate_synthesis([])
    with pytest.raises(ValueError, match='batch_size'):
        model.evaluate_synthesis([(texts[0], mels[0])], batch_size=0)
    with pytest.raises(ValueError, match=r'items\[0\] must be a'):
        model.evaluate_synthesis([texts[0]])
    with pytest.raises(ValueError, match='mel_dtw'):
        Tacotron2(lambda *a, **k: None, lang='en').evaluate_synthesis([(texts[0], mels[0])])
    # the speaker of an SV2TTS model rides along as for infer: one row of it per batch row
    spk = rng.standard_normal((3, 256)).astype(np.float32)
    rt4 = _SynthRuntime(lambda n: n + 3)
    SV2TTSTacotron2(rt4, lang='en', embeddings=spk).evaluate_synthesis(list(zip(texts[:3], mels[:3])), batch_size=2, embeddings=2)
    for (tokens, emb), _ in rt4.infers:
        assert emb.shape == (tokens.shape[0], 256) and np.all(emb == spk[2])


def test_copy_synthesis_vocodes_analyses_and_compares():
    from text_to_speech_amd.waveglow import WaveGlow
    log, calls = [], []

    class Engine:
        def mel_stft(self, audio):
            calls.append(('mel_stft', audio))
            frames = audio.shape[1] // 256 + 1
            return _Dev(np.full((1, frames, 80), -3.0, np.float32), log)

        def mel_dtw(self, a, b, lengths_a=None, lengths_b=None, **kw):
            calls.append(('mel_dtw', a, b, lengths_a, lengths_b, kw))
            return _Dev(_fake_stats(a.array, b.array, [a.shape[1]], [b.shape[1]], **kw), log)

    class Runtime:
        engine = Engine()

        def _uploaded(self, x):
            return _Dev(np.asarray(x, np.float32), log)

        def __call__(self, mel, **kw):
            calls.append(('infer', mel, kw))
            return _Dev(np.zeros((1, mel.shape[1] * 256 + 100), np.float32), log)

    mels = [mc.log_mel(np.random.default_rng(8), n) for n in (12, 5)]
    res = WaveGlow(Runtime()).copy_synthesis(mels, n_cep=10, seed=3, sigma=0.8)
    assert res['names'] == ['mcd', 'frames'] and res['per_item'].shape == (2, 2) and res['per_item'].dtype == np.float32
    assert [c[0] for c in calls] == ['infer', 'mel_stft', 'mel_dtw'] * 2
    for i, mel in enumerate(mels):
        infer, stft, dtw = calls[3 * i:3 * i + 3]
        assert np.array_equal(infer[1].array, mel[None]) and infer[2] == {'seed': 3, 'sigma': 0.8}
        assert stft[1].shape == (1, len(mel) * 256)                                                # cut to the mel's samples
        assert dtw[1] is infer[1] and dtw[2].shape == (1, len(mel) + 1, 80) and dtw[3:] == (None, None, {'n_cep': 10, 'align': False})
        want = _fake_stats(mel[None], dtw[2].array, [len(mel)], [len(mel) + 1], n_cep=10, align=False)
        assert res['per_item'][:, i].tolist() == [want[2, 0], len(mel)]
    assert log == [(3, 1), (3, 1)]                                                                 # only the statistics came to the host
    assert res['mean'] == {'mcd': pytest.approx(float(res['per_item'][0].astype(np.float64).mean())), 'frames': 8.5}
    with pytest.raises(ValueError, match='engine'):
        WaveGlow(lambda mel, **kw: None).copy_synthesis(mels)
    with pytest.raises(ValueError, match=r'mels\[0\] must be \[T, 80\]'):
        WaveGlow(Runtime()).copy_synthesis([mels[0][None]])


def test_metrics_name_the_statistics_and_cut_the_paths():
    from text_to_speech_amd import metrics
    seen = []

    class Engine:
        def mel_dtw(self, a, b, lengths_a=None, lengths_b=None, **kw):
            seen.append((lengths_a, lengths_b, kw))
            stats = np.array([[4., 6.], [2., 3.], [9., 8.]], np.float32)
            path = np.full((2, 5, 2), -1, np.int32)
            path[0, :2], path[1, :3] = [[0, 0], [1, 1]], [[0, 0], [0, 1], [1, 2]]
            return (stats, path) if kw.get('return_path') else stats

    assert metrics.MCD_DB_FACTOR == mr.MCD_DB_FACTOR == pytest.approx(6.141851463713754, rel=1e-15)
    out = metrics.mel_cepstral_distortion(Engine(), 'a', 'b', [1, 2], n_cep=5, align=False)
    assert {k: v.tolist() for k, v in out.items()} == {'mcd': [9., 8.], 'cost': [4., 6.], 'path_len': [2., 3.]}
    assert seen == [([1, 2], None, dict(n_cep=5, include_c0=False, align=False, stream=None))]
    paths = metrics.dtw_path(Engine(), 'a', 'b', include_c0=True)
    assert [p.tolist() for p in paths] == [[[0, 0], [1, 1]], [[0, 0], [0, 1], [1, 2]]] and paths[0].dtype == np.int32
    assert seen[1] == (None, None, dict(n_cep=13, include_c0=True, return_path=True))


def test_runtime_hands_mel_dtw_to_its_engine():
    from text_to_speech_amd.runtime import HipRuntime
    seen = []

    class Engine:
        def mel_dtw(self, *args, **kw):
            seen.append((args, kw))
            return 'stats'

    assert HipRuntime('unused', engine=Engine()).mel_dtw('a', 'b', [1], n_cep=7, return_path=True) == 'stats'
    assert seen == [(('a', 'b', [1], None), dict(n_cep=7, return_path=True))]
