"""CPU: the inputs of tests/silence_cases.py reach what they are named after (conditions on the inputs and on the
restatement, not measurements), the reference side of the probe stages agrees with trim_rms / trim_threshold /
trim_mean_window, and the host side of HipEngine.remove_silence_probe and its C check (no GPU call).

Everything up to test_probe_wrapper_asks_for_the_width_first checks tests/silence_ref.py and tests/silence_cases.py only: it
establishes that they are fit to judge the GPU code by (tests/test_silence_stages_gpu.py does that)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import silence_cases as sc
import silence_ref as sr

U = 2.0 ** -53


def _settings(kw):
    return {k: v for k, v in kw.items() if k not in ('mode', 'replace_by')}


@pytest.mark.parametrize('name', sc.RMS_NAMES)
def test_block_peaks_stand_far_from_the_threshold(name):
    c = sc.rms_cases()[name]
    assert sorted(sc.rms_cases()) == sorted(sc.RMS_NAMES)
    for kw in c.kws:
        m = sr.rms_margin(c.x, c.rate, **kw)
        assert m >= 0.96 and m >= sr.MARGINS['rms']
    loud = np.abs(c.x) >= 0.25
    assert (np.abs(c.x[loud]) <= 0.5).all() and (np.abs(c.x[~loud]) <= 2e-3).all()
    t = np.flatnonzero(loud)
    assert (np.sign(c.x[t]) == np.where(t % 2 == 0, 1, -1)).all()


def test_carry_reaches_every_carry():
    c = sc.rms_cases()['carry']
    kw, L = c.kws[0], len(c.x)
    assert kw['min_voice_time'] == 0.002 and kw['block_size'] == 16 and L == 20000 * 16 - 5
    assert sorted((k['min_voice_time'], k['replace_by']) for k in c.kws) == [(0, 0), (0, 8), (0.002, 0), (0.002, 8)]
    assert c.modes == sr.RMS_MODES
    flags = sr.rms_flags(c.x, c.rate, **kw)
    assert len(flags) == 20000                                  # 20 chunks of flags
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[2], flags, [2]]))))
    assert runs.min() >= 1 and runs.max() <= 4
    straddled = [m for m in range(sc.CHUNK, len(flags), sc.CHUNK) if flags[m - 1] and flags[m]]
    assert len(straddled) >= 3                                  # a silent run over a chunk edge: prev_loud is carried
    listed = sr.rms_listed(c.x, c.rate, **kw)
    links = sr.rms_links(listed, L, c.rate, **kw)
    merged = sr.rms_silences(c.x, c.rate, **_settings(kw))
    print(f'carry: {len(listed)} listed, {len(merged)} merged, silent runs over the flag chunk edges {straddled}')
    assert len(listed) > 2 * sc.CHUNK and len(merged) > sc.CHUNK            # ns, nm and the in-place pass are carried
    assert links[sc.CHUNK - 1] and links[2 * sc.CHUNK - 1]      # a chain over listed 1024 and one over 2048
    assert len(merged) == 1 + links.count(False)
    assert len(sr.rms_silences(c.x, c.rate, **dict(_settings(kw), min_voice_time=0))) == len(listed)
    # no pair's decision depends on the fusing: this case tests the carries alone
    fused = [sc.fused_link(listed[k][1], listed[k + 1][0], L, c.rate, 16, 0.002) for k in range(len(links))]
    assert fused == links
    assert sc.fused_ends_row(listed[-1][1], L, c.rate, 16) == (abs(min(L / c.rate, listed[-1][1] * (16 / c.rate)) * c.rate - L) <= 1)


def test_cap_edge_fills_the_list():
    c = sc.rms_cases()['cap_edge']
    kw, = c.kws
    flags = sr.rms_flags(c.x, c.rate, **kw)
    assert len(flags) == 2051 and flags[0] and flags[-1] and (flags[::2] == 1).all() and (flags[1::2] == 0).all()
    listed = sr.rms_listed(c.x, c.rate, **kw)
    # cap (audio_call.h): NB // (q + 1) + 1 with q = max(1, (int)(min_silence / bt) - 1) = 1
    assert len(listed) == 1026 == 2051 // 2 + 1 and len(listed) > sc.CHUNK
    assert len(sr.rms_silences(c.x, c.rate, **_settings(kw))) == 1026


def test_chunk_rows_end_at_the_chunk_edge():
    cases = sc.rms_cases()
    f = {n: sr.rms_flags(cases[n].x, cases[n].rate, **cases[n].kws[0]) for n in ('one_chunk', 'one_over_silent', 'one_over_loud')}
    assert [len(v) for v in f.values()] == [1024, 1025, 1025]
    assert list(f['one_over_silent'][1021:]) == [0, 1, 1, 1]    # a run over flag 1024, listed by the second chunk
    assert list(f['one_over_loud'][1021:]) == [0, 1, 1, 0]      # a run that ends with the first chunk; its end reads flag 1024
    assert (1022, 1025) in sr.rms_listed(cases['one_over_silent'].x, 22050, **cases['one_over_silent'].kws[0])
    assert (1022, 1024) in sr.rms_listed(cases['one_over_loud'].x, 22050, **cases['one_over_loud'].kws[0])
    assert len(cases['one_over_loud'].x) % 16 != 0


def test_gap20_is_decided_by_one_rounding():
    c = sc.rms_cases()['gap20']
    kw, = c.kws
    assert c.rate == 16000 and set(kw) == {'replace_by'}        # every other setting at the reference's default
    assert sr.rms_listed(c.x, c.rate) == [(0, 10), (30, 42), (67, 78)]
    assert sr.rms_links(sr.rms_listed(c.x, c.rate), len(c.x), c.rate) == [True, False]
    assert 30 * 0.01 - 10 * 0.01 == 0.19999999999999998 and 160 / 16000 == 0.01
    assert sc.fused_link(10, 30, len(c.x), 16000, 160, 0.2) is False        # the fused form gives exactly 0.2: no merge
    assert sc.fma(30.0, 0.01, -10 * 0.01) == 0.2
    assert sc.fused_link(42, 67, len(c.x), 16000, 160, 0.2) is False
    kept = tuple(len(sr.trim_rms(c.x, c.rate, mode=m, **kw)) for m in sr.RMS_MODES)
    assert kept == sc.KEPT['gap20']
    # unmerged (min_voice_time a hair lower keeps the voice of 20 blocks): what a kernel that fuses would return
    assert tuple(len(sr.trim_rms(c.x, c.rate, mode=m, min_voice_time=0.19, **kw)) for m in sr.RMS_MODES) == sc.GAP20_UNMERGED


@pytest.mark.parametrize('name,rate,bs,j', [('tail_one_loud_22050', 22050, 220, 25), ('tail_one_loud_16000', 16000, 160, 21)])
def test_tail_one_loud_is_decided_by_one_rounding(name, rate, bs, j):
    c = sc.rms_cases()[name]
    L = len(c.x)
    assert c.rate == rate and L == j * bs + 1 and abs(c.x[-1]) >= 0.25
    (i, jj), = sr.rms_listed(c.x, rate)
    assert jj == j
    e = min(L / rate, j * (bs / rate))
    assert e * rate == j * bs and abs(e * rate - L) <= 1        # the doubles: the silence ends one sample before the row
    assert not sc.fused_ends_row(j, L, rate, bs)                # the unrounded product is a hair smaller
    kept = tuple(len(sr.trim_rms(c.x, rate, mode=m, **c.kws[0])) for m in sr.RMS_MODES)
    rb = int(0.1 * rate)
    assert kept == (i * bs + rb, L, i * bs + rb, i * bs + rb)
    if name in sc.KEPT:
        assert kept == sc.KEPT[name]


# ---------------------------------------------------------------------------------------------- the reference of the stages
@pytest.mark.parametrize('case', sr.CASES, ids=[c[0] for c in sr.CASES])
def test_mask_gives_the_samples_of_the_restatement(case):
    name, inp, method, kw = case
    rate, x = sr.make_input(inp)
    mask = sr.keep_mask(method, x, rate, **kw)
    assert mask.dtype == np.uint8 and mask.shape == x.shape and set(np.unique(mask)) <= {0, 1}
    assert np.array_equal(x[mask != 0], sr.run(method, x, rate, **kw))
    if method == 'rms':
        ref = sc.rms_reference(x, rate, **kw)
        assert np.array_equal(ref['out'], sr.run(method, x, rate, **kw))
        assert (np.diff(ref['d0']) >= 0).all() and 0 <= ref['cut'] <= len(x)
        assert ref['n'] == (len(sr.rms_silences(x, rate, **_settings(kw))) if kw['mode'] == 'remove' else 1)
        assert ref['tile_offsets'][0] == 0 and len(ref['tile_offsets']) == -(-len(x) // 2048)
        assert ref['tile_offsets'][-1] + int(mask[(len(ref['tile_offsets']) - 1) * 2048:].sum()) == len(ref['out'])


@pytest.mark.parametrize('name', sc.RMS_NAMES)
def test_stage_reference_of_the_new_cases(name):
    c = sc.rms_cases()[name]
    for kw in c.calls():
        ref = sc.rms_reference(c.x, c.rate, **kw)
        assert np.array_equal(ref['out'], sr.trim_rms(c.x, c.rate, **kw)), kw


def test_longdouble_prefix_and_mask_agree_with_the_fp64_restatement():
    rate, x = sr.make_input('mw_pattern')
    P = sr.square_prefix(x)
    assert P.dtype == np.longdouble and np.finfo(np.longdouble).eps < 2.0 ** -60 and len(P) == len(x) + 1 and P[0] == 0
    assert float(P[-1]) == pytest.approx(float(np.sum(np.square(x), dtype=np.float64)), rel=1e-13)
    mask, margin = sr.mean_window_long(x, rate)
    assert np.array_equal(mask, sr.keep_mask('remove', x, rate)) and margin == pytest.approx(sr.mean_window_margin(x, rate), rel=1e-6)


# ---------------------------------------------------------------------------------------------- the long batch
def test_long_rows_reach_the_second_chunk_of_tiles():
    rows = sc.long_rows()
    assert tuple(len(r) for r in rows) == sc.LONG_LENGTHS == (2048 * 1025 + 777, 2048 * 1024, 2048 * 1024 + 1, 30000)
    assert [-(-len(r) // sc.TILE) for r in rows] == [1026, 1024, 1025, 15]
    assert abs(rows[0][:100]).max() > 0.1 and abs(rows[3][:2048]).max() < 0.01     # voice first; the short row starts in a pause
    a = sc.long_batch()
    assert a.nbytes < 35e6 and all(np.isnan(a[b, len(r):]).all() and not np.isnan(a[b, :len(r)]).any() for b, r in enumerate(rows))
    for b, x in enumerate(rows):
        mask, margin = sc.long_reference(b, 'rms')
        assert margin >= sr.MARGINS['rms']
        mask, margin = sc.long_reference(b, 'remove')
        print(f'long row {b}: mean-window margin {margin:.3e}, keeps {int(mask.sum())} of {len(x)}')
        assert margin >= sc.LONG_MARGIN
        assert np.array_equal(mask, sr.keep_mask('remove', x, sc.LONG_RATE))       # the fp64 restatement agrees at this margin
        assert 0.5 * len(x) < mask.sum() < len(x)
    # the kept samples of the long row straddle the chunk edge of the compaction's scan
    for method in ('rms', 'remove'):
        assert int(sc.long_reference(0, method)[0].sum()) == sc.LONG_KEPT[method]
        off = sc.tile_offsets(sc.long_reference(0, method)[0])
        assert len(off) == 1026 and 0 < off[1023] < off[1024] < off[1025]


def test_prefix_bound_refuses_a_sequential_and_an_fp32_sum():
    x = sc.long_rows()[0]
    P = sr.square_prefix(x)
    sq = x * x
    seq = np.concatenate([[0.0], np.cumsum(sq.astype(np.float64))])
    ratio = float((np.abs(seq - P)[1:] / (P[1:] * U)).max())
    print(f'np.cumsum in fp64 over {len(x)} squares: {float(abs(seq[-1] - P[-1])):.3e} off at P[L] = {float(P[-1]):.4e}, '
          f'worst ratio {ratio:.1f} (bound {sc.PREFIX_DEPTH})')
    assert sc.PREFIX_DEPTH < 64 < ratio
    f32 = np.concatenate([[0.0], np.cumsum(sq, dtype=np.float32)]).astype(np.float64)
    assert float((np.abs(f32 - P)[1:] / (P[1:] * U)).max()) > 1e6


# ---------------------------------------------------------------------------------------------- host side, no GPU call
class _FakeLib:
    """Stands for the C library: records the probe calls, reports a width and fills `out` with a ramp."""

    def __init__(self, width):
        self.width, self.calls = width, []

    def tts_hip_remove_silence_probe(self, h, audio, B, N, lengths, method, mode, rate, threshold, min_silence, block_size,
                                     replace_by, min_voice_time, what, out, width, mem):
        self.calls.append(dict(B=B, N=N, lengths=lengths, args=(method, mode, rate, threshold, min_silence, block_size, replace_by,
                                                                  min_voice_time), what=what, out=out, mem=mem))
        width._obj.value = self.width
        if out is not None:
            ramp = (np.arange(B * self.width) % 251).astype(np.uint8)
            ctypes.memmove(out, ramp.ctypes.data, ramp.nbytes)
        return 0


def _engine(width):
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine.__new__(HipEngine)
    eng._lib, eng._h = _FakeLib(width), None
    return eng


def test_probe_wrapper_asks_for_the_width_first():
    eng = _engine(37)
    x = np.zeros((2, 4000), np.float32)
    flags = eng.remove_silence_probe(x, 22050, 'flags', lengths=[4000, 100], mode='remove', replace_by=0.1)
    first, second = eng._lib.calls
    assert first['out'] is None and second['out'] is not None                # the width alone, then the stage
    assert first['args'] == second['args'] == (0, 3, 22050, -25.0, 0.1, 220, 2205, 0.2)
    assert (first['what'], first['B'], first['N'], first['mem']) == (0, 2, 4000, 0) == tuple(second[k] for k in ('what', 'B', 'N', 'mem'))
    assert flags.dtype == np.uint8 and flags.shape == (2, 37) and flags[1, 0] == 37
    for what, (stage, dtype) in {'intervals': (1, np.int32), 'mask': (2, np.uint8), 'tile_offsets': (3, np.int32)}.items():
        eng = _engine(5)
        out = eng.remove_silence_probe(x[0], 22050, what, method='threshold')
        assert out.dtype == dtype and out.shape == (1, 5) and eng._lib.calls[1]['what'] == stage
        assert eng._lib.calls[1]['args'] == (1, 0, 22050, 0.1, 0.0, 1, 1, 0.0) and eng._lib.calls[1]['lengths'] is None
    eng = _engine(4001)
    out = eng.remove_silence_probe(x, 22050, 'prefix', method='remove')
    assert out.dtype == np.float64 and out.shape == (2, 4001) and eng._lib.calls[1]['args'][:5] == (2, 0, 22050, 0.025, 0.15)


def test_probe_wrapper_refuses_what_remove_silence_refuses():
    eng = _engine(1)
    x = np.zeros(3000, np.float32)
    with pytest.raises(ValueError, match='what must be one of'):
        eng.remove_silence_probe(x, 22050, 'runs')
    for kw, needle in ((dict(method='threshold', mode='remove'), "remove_silence_probe: mode 'remove'"),
                       (dict(method='remove'), 'remove_silence_probe: a row of L = 3000.*w = 3307'),
                       (dict(replace_by=-1), 'remove_silence_probe: replace_by'), (dict(block_size=0), 'block_size'),
                       (dict(method='ffmpeg'), 'unknown method'), (dict(threshold=float('nan')), 'threshold'),
                       (dict(min_voice_time=-1.), 'min_voice_time'), (dict(lengths=[3001]), 'lengths')):
        with pytest.raises(ValueError, match=needle):
            eng.remove_silence_probe(x, 22050, 'mask', **kw)
    with pytest.raises(ValueError, match='rate'):
        eng.remove_silence_probe(x, None, 'mask')
    assert eng._lib.calls == []


# ---------------------------------------------------------------------------------------------- the C check of the probe
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')


@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    return os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')


def _probe_check(exe, lengths=(), **settings):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    args = [exe, '--audio-call', 'silence', 'probe=1'] + [f'{k}={v}' for k, v in settings.items()] + [str(n) for n in lengths]
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    status, _, message = lines[0].partition(' ')
    return int(status), message, [[int(v) for v in line.split()] for line in lines[1:]]


OK = dict(N=4100, B=2, rate=22050, block_size=220)


def test_probe_check_gives_every_stage_its_width(checker):
    NB, cap, NT = -(-4100 // 220), -(-4100 // 220) // 10 + 1, 3
    want = {(0, 0): (NB, 1), (0, 1): (2 + 2 * cap, 4), (0, 2): (4100, 1), (0, 3): (NT, 4),
            (1, 1): (4, 4), (1, 2): (4100, 1), (1, 3): (NT, 4),
            (2, 2): (4100, 1), (2, 3): (NT, 4), (2, 4): (4101, 8)}
    for method in (0, 1, 2):
        for what in range(5):
            rc, msg, rows = _probe_check(checker, **dict(OK, method=method, what=what, threshold=0.025))
            if (method, what) in want:
                assert rc == 0 and rows[0][:3] == [NT, NB if method == 0 else 0, cap if method == 0 else 1], (method, what, msg)
                assert tuple(rows[1]) == want[(method, what)], (method, what)
            else:
                assert rc == -1 and msg == f'who: method {method} has no stage {what}', (method, what, msg)
    # out NULL asks for the width alone
    rc, msg, rows = _probe_check(checker, **dict(OK, what=1, null='out'))
    assert rc == 0 and rows[1] == [2 + 2 * cap, 4]


def test_probe_check_refuses_what_the_call_refuses_first(checker):
    for settings, needle in ((dict(what=5), 'no stage 5 (0 .. 4)'), (dict(what=-1), 'no stage -1 (0 .. 4)'),
                             (dict(what=0, null='lens'), 'bad argument'), (dict(what=0, null='audio'), 'bad argument'),
                             (dict(what=9, method=3), 'method 3 not 0'), (dict(what=9, rate=0), 'rate = 0 <= 0'),
                             (dict(what=4, method=0, mode=4), 'mode 4 not 0'), (dict(what=2, overlap=1), 'out overlaps audio'),
                             (dict(what=2, mem=5), 'bad mem kind 5'), (dict(what=0, method=2, threshold=0), 'threshold = 0 <= 0'),
                             (dict(what=2, block_size=0), 'block_size = 0 < 1')):
        rc, msg, rows = _probe_check(checker, **dict(OK, **settings))
        assert rc == -1 and rows == [] and msg.startswith('who: ') and needle in msg, (settings, msg)
    rc, msg, _ = _probe_check(checker, (4100, 0), **dict(OK, what=2))
    assert rc == -1 and 'lengths[1] = 0 outside [1, N = 4100]' in msg
