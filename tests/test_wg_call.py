"""CPU: the front end of every WaveGlow call in C++ (csrc/wg_call.h: the reasons a call is refused, and the int table a call
with lengths stages to the device, as pure host code) against `packing_plan` (tests/waveglow_packed_ref.py) for packed calls
and a numpy restatement written here for ragged ones.  The C++ side is csrc/host_check.cpp's --wg-call mode, built with
-fsanitize=address,undefined like the weight-file loader (tests/test_host_sanitizer.py): `lengths` is untrusted input."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from waveglow_packed_ref import header_gap_frames, packing_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
MAX_FRAMES = 31744                                    # one run's limit (kMaxFramesPerRun)
MAX_BT = 1 << 25                                      # B * T * 32 <= 2^30 groups


@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    exe = os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')
    assert os.path.exists(exe)
    return exe


def _call(exe, T, packed, chunkB, lengths=(), **settings):
    """-> (status, message, table or None); table = dict(F, n_gap, info, run_tails, counts)."""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    args = [exe, '--wg-call', str(T), str(int(packed)), str(chunkB)] + [f'{k}={v}' for k, v in settings.items()]
    r = subprocess.run(args + [str(int(n)) for n in lengths], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    status, _, message = lines[0].partition(' ')
    if int(status) != 0:
        assert len(lines) == 1
        return int(status), message, None
    assert len(lines) == 5 and message == ''
    ints = lambda line, tag: [int(x) for x in line.split()[1:]] if line.split()[0] == tag else None
    F, n_gap = (int(x) for x in lines[1].split())
    return 0, '', dict(F=F, n_gap=n_gap, info=ints(lines[2], 'info'), run_tails=ints(lines[3], 'run_tails'),
                       counts=ints(lines[4], 'counts'))


# ---- packed: [start | len | flags | gaps] ----------------------------------------------------------------------------------
PLAN_CASES = [((0, 3, 0, 0, 2, 0), 5), ((7,), 9), ((1,), 1), ((0, 0), 4), ((4, 4, 4), 4),        # those of test_packing_plan
              ((800, 523, 77, 1, 640, 799, 300, 0), 800)]


def _assert_packed(exe, lengths, T):
    gap = header_gap_frames()
    rc, msg, t = _call(exe, T, True, 0, lengths)
    assert rc == 0, msg
    p, B = packing_plan(lengths, T, gap), len(lengths)
    info = t['info']
    assert t['F'] == p['F'] and t['n_gap'] == len(p['gaps']) and len(info) == 2 * B + p['F'] + len(p['gaps'])
    assert info[:B] == p['starts'] and info[B:2 * B] == list(lengths)
    assert info[2 * B:2 * B + p['F']] == p['flags'] and info[2 * B + p['F']:] == p['gaps']
    assert t['run_tails'] == [] and t['counts'] == [256 * n for n in lengths]


@pytest.mark.parametrize('lengths,T', PLAN_CASES)
def test_packed_table_equals_packing_plan(checker, lengths, T):
    _assert_packed(checker, lengths, T)


def test_packed_table_equals_packing_plan_on_random_lengths(checker):
    rng = np.random.default_rng(11)
    for i in range(300):
        B, T = int(rng.integers(1, 13)), int(rng.integers(1, 41))
        lengths = rng.integers(0, T + 1, B)
        lengths[rng.random(B) < (0.0, 0.3, 0.9)[i % 3]] = 0                    # none, some, mostly empty rows
        _assert_packed(checker, tuple(int(n) for n in lengths), T)


# ---- ragged: [lengths | tail frames run by run] -----------------------------------------------------------------------------
def ragged_table(lengths, T, chunkB):
    """The tail frames (t >= lengths[b]) of each run of chunkB rows, indexed inside that run, one list per run."""
    B = len(lengths)
    return [[(b - b0) * T + t for b in range(b0, min(b0 + chunkB, B)) for t in range(lengths[b], T)]
            for b0 in range(0, B, chunkB)]


def _assert_ragged(exe, lengths, T, chunkB_arg):
    rc, msg, t = _call(exe, T, False, chunkB_arg, lengths)
    assert rc == 0, msg
    B, chunkB = len(lengths), chunkB_arg or MAX_FRAMES // T
    runs = ragged_table(lengths, T, chunkB)
    assert t['F'] == 0 and t['n_gap'] == 0 and t['counts'] == [256 * n for n in lengths]
    assert t['info'][:B] == list(lengths) and t['run_tails'] == [len(r) for r in runs]
    assert len(t['info']) == B + sum(T - n for n in lengths)
    at = B
    for r, want in enumerate(runs):                                            # one contiguous slice per run, in run order
        got = t['info'][at:at + len(want)]
        assert got == want, (r, got[:8], want[:8])
        rows = min(chunkB, B - r * chunkB)
        assert all(0 <= f < rows * T and f % T >= lengths[r * chunkB + f // T] for f in got)
        at += len(want)
    assert at == len(t['info'])


@pytest.mark.parametrize('lengths,T,chunkB', [
    ((15990, 16000, 15000), 16000, 0),          # 31744 // 16000 = 1 row per run: three runs, the second without tails
    ((11990, 12000, 11000), 12000, 0),          # 2 rows per run: 3 rows leave a last run of one
    ((6, 0, 3), 6, 0),                          # one run of everything
    ((3, 5, 0, 4, 1), 5, 2),                    # chunkB does not divide B
    ((2, 2, 2, 2), 2, 3),                       # no tails at all
    ((0,), 7, 1),
])
def test_ragged_table_equals_the_restatement(checker, lengths, T, chunkB):
    _assert_ragged(checker, lengths, T, chunkB)


def test_ragged_table_equals_the_restatement_on_random_lengths(checker):
    rng = np.random.default_rng(12)
    for _ in range(200):
        B, T = int(rng.integers(1, 13)), int(rng.integers(1, 41))
        _assert_ragged(checker, tuple(int(n) for n in rng.integers(0, T + 1, B)), T, int(rng.integers(1, B + 2)))


def test_counts_without_lengths(checker):
    rc, _, t = _call(checker, 6, False, 0, B=3, noise=2)
    assert rc == 0 and t['info'] == [] and t['run_tails'] == [] and t['counts'] == [6 * 256] * 3


# ---- refusals: one row per reason -------------------------------------------------------------------------------------------
FULL = (MAX_FRAMES - 4) // 2                          # two such rows and their gap fill one run exactly
REFUSALS = [
    # (T, packed, lengths, settings, substrings of the message)
    (6, 0, (), dict(B=3, precision=3), ['precision']),
    (6, 0, (), dict(B=3, precision=-1), ['precision']),
    (6, 0, (), dict(B=3, mem=7), ['bad mem kind 7']),
    (6, 0, (), dict(B=3, noise=2, null='keys'), ['NULL']),
    (6, 0, (), dict(B=3, noise=2, null='offsets'), ['NULL']),
    (6, 0, (), dict(B=0), ['bad argument', 'B = 0']),
    (6, 0, (), dict(B=-2), ['bad argument', 'B = -2']),
    (6, 0, (), dict(B=3, null='mel'), ['bad argument']),
    (6, 0, (), dict(B=3, null='audio'), ['bad argument']),
    (0, 0, (), dict(B=3), ['bad argument']),
    (16384, 0, (), dict(B=MAX_BT // 16384 + 1), ['B*T too large']),
    (16384, 0, (), dict(B=MAX_BT // 16384 + 1, **{'async': 1}), ['B*T too large']),     # the async calls have the limit too
    (6, 1, (), dict(B=3), ['packed needs lengths', 'NULL']),
    (6, 0, (6, 7, 3), {}, ['lengths[1] = 7']),
    (6, 1, (6, 2, -1), {}, ['lengths[2] = -1']),
    (6, 0, (6, 7, 3), dict(noise=2, **{'async': 1}), ['lengths[1] = 7']),
    (MAX_FRAMES + 1, 0, (), dict(B=1), ['windowed inference', f'T = {MAX_FRAMES + 1} frames', str(MAX_FRAMES)]),
    (MAX_FRAMES + 1, 0, (5,), {}, ['windowed inference']),
    (FULL + 1, 1, (FULL, FULL + 1), {}, [f'F = {MAX_FRAMES + 1} frames', str(MAX_FRAMES)]),
]


@pytest.mark.parametrize('T,packed,lengths,settings,needles', REFUSALS)
def test_refusals(checker, T, packed, lengths, settings, needles):
    rc, msg, t = _call(checker, T, packed, 0, lengths, **settings)
    assert rc == -1 and t is None and msg.startswith('who: '), (rc, msg)
    assert all(n in msg for n in needles), msg


def test_the_limits_themselves_are_accepted(checker):
    rc, msg, t = _call(checker, MAX_FRAMES, False, 0, B=1)
    assert rc == 0, msg
    rc, msg, t = _call(checker, FULL, True, 0, (FULL, FULL))
    assert rc == 0 and t['F'] == MAX_FRAMES, msg
    rc, msg, t = _call(checker, 16384, False, 0, B=MAX_BT // 16384)
    assert rc == 0, msg
    # T alone does not limit a packed call, and the mem kind is no argument of an async call
    rc, msg, t = _call(checker, 40000, True, 0, (3, 2))
    assert rc == 0 and t['F'] == 5 + header_gap_frames(), msg
    rc, msg, t = _call(checker, 6, False, 0, B=3, mem=7, **{'async': 1})
    assert rc == 0, msg


def test_refusal_precedence(checker):
    """First match in the order csrc/wg_call.h documents: precision, mem kind, keys / offsets, B, mel / audio / T, B * T,
    packed without lengths, lengths[b], the one-run limit."""
    order = [dict(precision=5), dict(mem=9), dict(noise=2, null='keys')]
    needles = ['precision', 'bad mem kind', 'keys / offsets']
    for i, needle in enumerate(needles):
        settings = {}
        for s in order[i:]:
            settings.update(s)
        rc, msg, _ = _call(checker, 0, True, 0, B=0, **settings)               # B, T and packed-without-lengths are wrong too
        assert rc == -1 and needle in msg, msg
    assert 'B = 0' in _call(checker, 0, True, 0, B=0, null='mel')[1]
    assert 'T = 0' in _call(checker, 0, True, 0, B=1 << 30)[1]
    assert 'B*T too large' in _call(checker, MAX_FRAMES + 1, True, 0, B=1 << 20)[1]
    assert 'packed needs lengths' in _call(checker, MAX_FRAMES + 1, True, 0, B=2)[1]
    assert 'lengths[0] = -3' in _call(checker, MAX_FRAMES + 1, False, 0, (-3, 1))[1]


# ---- the inverse direction's test hook (tts_hip_waveglow_probe_rows): wg_probe_check ---------------------------------------
def probe_refusal(T, packed, lengths, B, precision=0, mem=0, flow=0, what=0, layer=0, null=''):
    """The first reason wg_probe_check gives, as a substring of its message (None: accepted), restated from
    include/tts_hip.h: the reasons of the ragged / packed call for the same mel / B / T / lengths / packed / precision / mem
    (its audio pointer is not looked at), then flow, what, layer, what 2 outside fp32, B * T above one run, out NULL."""
    B = len(lengths) if lengths else B
    if not 0 <= precision <= 2:
        return 'precision must be'
    if mem not in (0, 1):
        return f'bad mem kind {mem}'
    if B <= 0:
        return f'B = {B} must be positive'
    if 'mel' in null or T <= 0:
        return 'mel or audio is NULL, or T'
    if B * T * 32 > 1 << 30:
        return 'B*T too large'
    if packed and not lengths:
        return 'packed needs lengths'
    for b, n in enumerate(lengths):
        if not 0 <= n <= T:
            return f'lengths[{b}] = {n} is outside'
    if packed:
        rows = sum(n > 0 for n in lengths)
        if sum(lengths) + header_gap_frames() * max(rows - 1, 0) > MAX_FRAMES:
            return 'the packed row holds F = '
    elif T > MAX_FRAMES:
        return 'windowed inference'
    if not 0 <= flow <= 11:
        return f'flow = {flow} is outside [0, 11]'
    if not 0 <= what <= 2:
        return f'what = {what} must be'
    if not 0 <= layer <= 7:
        return f'layer = {layer} is outside [0, 7]'
    if what == 2 and precision != 0:
        return f'what = 2 (cond) needs precision 0 (f32), got {precision}'
    if not packed and B * T > MAX_FRAMES:
        return f'B * T = {B * T} frames exceeds one run'
    if 'out' in null:
        return 'out is NULL'
    return None


def _probe(exe, T, packed, lengths=(), B=-1, **kw):
    """(status, message) of the C++ check and the restatement's needle for the same request."""
    settings = dict(kw)
    if not lengths:
        settings['B'] = B
    settings.setdefault('flow', 0)                    # (any of flow= / what= / layer= selects the probe's check)
    rc, msg, _ = _call(exe, T, packed, 0, lengths, **settings)
    return rc, msg, probe_refusal(T, packed, lengths, B, **kw)


PROBE_REQUESTS = [
    # accepted: a plain call, a ragged one, a packed one, the limits themselves
    (6, 0, (), dict(B=3)), (6, 0, (6, 0, 3), dict(flow=11, what=1, layer=7)), (6, 1, (6, 0, 3), dict(precision=2, what=0)),
    (6, 0, (), dict(B=2, what=2, layer=7)), (MAX_FRAMES // 4, 0, (), dict(B=4)), (FULL, 1, (FULL, FULL), {}),
    (40000, 1, (3, 2), {}),                           # T alone does not limit a packed probe either
    (6, 0, (), dict(B=3, null='audio')),              # the probe has no audio argument: that pointer is not looked at
    # the call's own reasons, in the call's order
    (6, 0, (), dict(B=3, precision=3)), (6, 0, (), dict(B=3, mem=7)), (6, 0, (), dict(B=0)), (6, 0, (), dict(B=3, null='mel')),
    (0, 0, (), dict(B=3)), (16384, 0, (), dict(B=MAX_BT // 16384 + 1)), (6, 1, (), dict(B=3)), (6, 0, (6, 7, 3), {}),
    (6, 1, (6, 2, -1), {}), (MAX_FRAMES + 1, 0, (), dict(B=1)), (FULL + 1, 1, (FULL, FULL + 1), {}),
    # the probe's own
    (6, 0, (), dict(B=3, flow=-1)), (6, 0, (), dict(B=3, flow=12)), (6, 0, (), dict(B=3, what=-1)), (6, 0, (), dict(B=3, what=3)),
    (6, 0, (), dict(B=3, layer=-1)), (6, 0, (), dict(B=3, layer=8)), (6, 0, (), dict(B=3, what=2, precision=1)),
    (6, 0, (6, 1, 2), dict(what=2, precision=2)), (MAX_FRAMES // 4 + 1, 0, (), dict(B=4)),
    (MAX_FRAMES // 2 + 1, 0, (5, 7), {}),              # a ragged probe is one run of B * T frames whatever the lengths
    (6, 0, (), dict(B=3, null='out')), (6, 1, (6, 0, 3), dict(null='out')),
]


@pytest.mark.parametrize('T,packed,lengths,kw', PROBE_REQUESTS)
def test_probe_check_equals_the_restatement(checker, T, packed, lengths, kw):
    rc, msg, want = _probe(checker, T, packed, lengths, **kw)
    if want is None:
        assert rc == 0, msg
    else:
        assert rc == -1 and msg.startswith('who: ') and want in msg, (msg, want)


def test_probe_check_every_kind_of_refusal_is_in_the_table(checker):
    wants = {probe_refusal(T, packed, lengths, kw.get('B', -1), **{k: v for k, v in kw.items() if k != 'B'})
             for T, packed, lengths, kw in PROBE_REQUESTS}
    reasons = ['precision must be', 'bad mem kind', 'must be positive', 'mel or audio is NULL', 'B*T too large', 'packed needs lengths',
               'lengths[', 'the packed row holds', 'windowed inference', 'flow = ', 'what = 3', 'layer = ', 'what = 2 (cond)',
               'exceeds one run', 'out is NULL']
    assert None in wants and all(any(w and r in w for w in wants) for r in reasons)


def test_probe_check_precedence_on_random_requests(checker):
    """Several things wrong at once: the first match in the documented order is the one reported."""
    rng = np.random.default_rng(13)
    pick = lambda values, p_first: values[0] if rng.random() < p_first else values[int(rng.integers(1, len(values)))]
    seen = set()
    for _ in range(250):
        T = pick([6, 0, MAX_FRAMES + 1], 0.8)
        packed = int(rng.random() < 0.3)
        lengths = pick([(), (6, 0, 3), (6, 7, 3), (-1, 2)], 0.4)
        kw = dict(B=pick([3, 0, MAX_FRAMES], 0.7), precision=pick([0, 1, 2, 3, -1], 0.5), mem=pick([0, 1, 5], 0.5),
                  flow=pick([11, 0, -1, 12], 0.6), what=pick([0, 1, 2, 3], 0.4), layer=pick([0, 7, 8, -2], 0.6),
                  null=pick(['', 'out', 'mel', 'mel,out'], 0.6))
        if not kw['null']:
            del kw['null']
        rc, msg, want = _probe(checker, T, packed, lengths, **kw)
        seen.add(want)
        assert (rc == 0 and want is None) or (rc == -1 and want is not None and want in msg), (T, packed, lengths, kw, msg, want)
    assert None in seen and len(seen) >= 12
