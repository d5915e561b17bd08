"""GPU: silence removal (csrc/silence.hip) past its scan carries and at its rounding edges, stage by stage
(`HipEngine.remove_silence_probe`) against the numpy restatement (tests/silence_cases.py, tests/silence_ref.py).  The
conditions that make these inputs fit for it are tests/test_silence_stages.py's."""
import ctypes

import numpy as np
import pytest

import silence_cases as sc
import silence_ref as sr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _check_rms_call(eng, c, kw):
    """One call and its four stages on one row, everything exact."""
    ref = sc.rms_reference(c.x, c.rate, **kw)
    L, what = len(c.x), f'{c.name} {kw}'
    y = eng.remove_silence(c.x, c.rate, **kw)
    assert y.dtype == np.float32 and len(y) == len(ref['out']), (what, len(y), len(ref['out']))
    assert np.array_equal(y, ref['out']), what
    flags = eng.remove_silence_probe(c.x, c.rate, 'flags', **kw)
    assert flags.shape[0] == 1 and flags.shape[1] >= len(ref['flags']) and np.array_equal(flags[0, :len(ref['flags'])], ref['flags']), what
    iv = eng.remove_silence_probe(c.x, c.rate, 'intervals', **kw)[0]
    cap = (len(iv) - 2) // 2
    n = int(iv[0])
    assert (n, int(iv[1])) == (ref['n'], ref['cut']), what
    d0, d1 = iv[2:2 + n], iv[2 + cap:2 + cap + n]
    wrong = np.flatnonzero((d0 != ref['d0']) | (d1 != ref['d1']))
    assert wrong.size == 0, f'{what}: {wrong.size} of {n} intervals differ, first at {wrong[0]}: ' \
                            f'({d0[wrong[0]]}, {d1[wrong[0]]}) for ({ref["d0"][wrong[0]]}, {ref["d1"][wrong[0]]})'
    mask = eng.remove_silence_probe(c.x, c.rate, 'mask', **kw)
    assert mask.shape == (1, L) and np.array_equal(mask[0], ref['mask']), what
    off = eng.remove_silence_probe(c.x, c.rate, 'tile_offsets', **kw)
    assert off.shape == (1, -(-L // sc.TILE)) and np.array_equal(off[0], ref['tile_offsets']), what
    return y


@pytest.mark.parametrize('name', sc.RMS_NAMES)
def test_rms_case_and_its_stages_are_exact(gpu_engine, name):
    c = sc.rms_cases()[name]
    for kw in c.calls():
        assert sr.rms_margin(c.x, c.rate, **kw) >= sr.MARGINS['rms']          # a condition on the input, as on the CPU
        _check_rms_call(gpu_engine, c, kw)


def test_carry_again_gives_the_same_bits(gpu_engine):
    c = sc.rms_cases()['carry']
    kw = dict(c.kws[0], mode='remove')
    first = gpu_engine.remove_silence(c.x, c.rate, **kw)
    iv = gpu_engine.remove_silence_probe(c.x, c.rate, 'intervals', **kw)
    n = int(iv[0, 0])
    cap = (iv.shape[1] - 2) // 2
    gpu_engine.remove_silence(sc.rms_cases()['cap_edge'].x, 22050, **sc.rms_cases()['cap_edge'].calls()[0])   # another call between
    again = gpu_engine.remove_silence(c.x, c.rate, **kw)
    iv2 = gpu_engine.remove_silence_probe(c.x, c.rate, 'intervals', **kw)
    assert first.tobytes() == again.tobytes()
    assert np.array_equal(iv[0, :2 + n], iv2[0, :2 + n]) and np.array_equal(iv[0, 2 + cap:2 + cap + n], iv2[0, 2 + cap:2 + cap + n])


# the cases batched by rate, under the settings of the batch's first case (a row made for other settings is one more input)
BATCHES = {'chunk_rows': ('one_over_silent', 'one_chunk', 'carry', 'one_over_loud'), 'cap_edge': ('cap_edge', 'one_over_silent'),
           'gap20': ('gap20', 'tail_one_loud_16000'), 'tail': ('tail_one_loud_22050', 'cap_edge', 'one_chunk')}


@pytest.mark.parametrize('mode', sr.RMS_MODES)
@pytest.mark.parametrize('batch', BATCHES)
def test_ragged_batch_of_the_cases_equals_one_row_calls(gpu_engine, batch, mode):
    """Every row of a ragged batch is what its one-row call and the restatement give, stage by stage: zeros behind the kept
    samples, no NaN from behind the lengths."""
    cases = sc.rms_cases()
    first = cases[BATCHES[batch][0]]
    kw = dict(first.kws[0], mode=mode)
    rows = [cases[n].x for n in BATCHES[batch]]
    assert all(cases[n].rate == first.rate for n in BATCHES[batch])
    lens = [len(r) for r in rows]
    a = np.full((len(rows), max(lens)), np.nan, np.float32)
    for b, r in enumerate(rows):
        a[b, :len(r)] = r
    out, n = gpu_engine.remove_silence(a, first.rate, lengths=lens, **kw)
    masks = gpu_engine.remove_silence_probe(a, first.rate, 'mask', lengths=lens, **kw)
    flags = gpu_engine.remove_silence_probe(a, first.rate, 'flags', lengths=lens, **kw)
    iv = gpu_engine.remove_silence_probe(a, first.rate, 'intervals', lengths=lens, **kw)
    cap = (iv.shape[1] - 2) // 2
    for b, r in enumerate(rows):
        assert sr.rms_margin(r, first.rate, **kw) >= sr.MARGINS['rms']
        ref = sc.rms_reference(r, first.rate, **kw)
        one = gpu_engine.remove_silence(r, first.rate, **kw)
        assert int(n[b]) == len(one) == len(ref['out']), (b, mode)
        assert np.array_equal(out[b, :n[b]], one) and np.array_equal(one, ref['out']), (b, mode)
        assert not out[b, n[b]:].any() and not np.isnan(out[b]).any()
        assert np.array_equal(masks[b, :len(r)], ref['mask']) and np.array_equal(flags[b, :len(ref['flags'])], ref['flags'])
        k = ref['n']
        assert (int(iv[b, 0]), int(iv[b, 1])) == (k, ref['cut'])
        assert np.array_equal(iv[b, 2:2 + k], ref['d0']) and np.array_equal(iv[b, 2 + cap:2 + cap + k], ref['d1']), (b, mode)


def test_threshold_method_stages(gpu_engine):
    for name, inp, method, kw in sr.CASES:
        if method != 'threshold' or inp == 'wav':
            continue
        rate, x = sr.make_input(inp)
        (a, cut) = sr.threshold_intervals(x, **kw)
        iv = gpu_engine.remove_silence_probe(x, rate, 'intervals', method='threshold', **kw)
        assert iv.shape == (1, 4) and list(iv[0]) == [1, cut, 0, a[0][1]], name
        mask = gpu_engine.remove_silence_probe(x, rate, 'mask', method='threshold', **kw)
        assert np.array_equal(mask[0], sr.keep_mask('threshold', x, rate, **kw)), name


def test_prefix_of_small_rows(gpu_engine):
    """The mean-window inputs of the end-to-end tests, leading silence (a small sum before a large one) among them: the
    prefix against the longdouble prefix under the same bound as the long rows, and the mask."""
    for inp in ('mw_pattern', 'mw_exact', 'mw_16k'):
        rate, x = sr.make_input(inp)
        L = len(x)
        P = sr.square_prefix(x)
        got = gpu_engine.remove_silence_probe(x, rate, 'prefix', method='remove')
        assert got.dtype == np.float64 and got.shape == (1, L + 1) and got[0, 0] == 0
        ratio = float((np.abs(got[0, 1:] - P[1:]) / (U * P[1:])).max())
        print(f'{inp}: worst |P_gpu - P| / (2^-53 P) = {ratio:.2f} (bound {sc.PREFIX_DEPTH}; recorded {sc.PREFIX_MEASURED["small"]})')
        assert ratio <= sc.PREFIX_DEPTH, inp
        mask = gpu_engine.remove_silence_probe(x, rate, 'mask', method='remove')
        assert np.array_equal(mask[0], sr.keep_mask('remove', x, rate)), inp


def test_long_batch_crosses_the_tile_chunk(gpu_engine):
    """Rows of 1026, 1024, 1025 and 15 tiles: two calls (rms remove, mean-window) and two probe calls (tile offsets of the
    rms call, prefix of the mean-window call)."""
    a, lens, rows = sc.long_batch(), list(sc.LONG_LENGTHS), sc.long_rows()
    for method, kw in sc.LONG_CALLS:
        out, n = gpu_engine.remove_silence(a, sc.LONG_RATE, lengths=lens, method=method, **kw)
        for b, x in enumerate(rows):
            mask, margin = sc.long_reference(b, method)
            assert margin >= (sr.MARGINS['rms'] if method == 'rms' else sc.LONG_MARGIN)
            want = x[mask != 0]
            assert int(n[b]) == len(want), (method, b, int(n[b]), len(want))
            assert np.array_equal(out[b, :n[b]], want), (method, b)
            assert not out[b, n[b]:].any() and not np.isnan(out[b]).any(), (method, b)
    off = gpu_engine.remove_silence_probe(a, sc.LONG_RATE, 'tile_offsets', lengths=lens, method='rms', **sc.LONG_CALLS[0][1])
    for b, x in enumerate(rows):
        want = sc.tile_offsets(sc.long_reference(b, 'rms')[0])
        assert np.array_equal(off[b, :len(want)], want), b          # the tiles at and behind 1024 among them
    assert off.shape[1] == 1026 and off[0, 1025] > off[0, 1024] > off[0, 1023] > 0
    prefix = gpu_engine.remove_silence_probe(a, sc.LONG_RATE, 'prefix', lengths=lens, method='remove')
    worst = 0.0
    for b, x in enumerate(rows):
        P = sr.square_prefix(x)
        got = prefix[b, :len(x) + 1]
        assert got[0] == 0
        ratio = np.abs(got[1:] - P[1:]) / (U * P[1:])
        at = int(ratio.argmax())
        print(f'long row {b}: worst |P_gpu - P| / (2^-53 P) = {float(ratio[at]):.2f} at t = {at + 1} (bound {sc.PREFIX_DEPTH})')
        worst = max(worst, float(ratio[at]))
        assert float(ratio[at]) <= sc.PREFIX_DEPTH, (b, at + 1)
    print(f'long batch: worst ratio {worst:.2f}; recorded {sc.PREFIX_MEASURED["long"]}')


def test_one_long_row_equals_its_row_of_the_batch(gpu_engine):
    """The ragged batch against a one-row call, on the row with a second chunk of tiles."""
    x = sc.long_rows()[0]
    for method, kw in sc.LONG_CALLS:
        mask, _ = sc.long_reference(0, method)
        one = gpu_engine.remove_silence(x, sc.LONG_RATE, method=method, **kw)
        assert np.array_equal(one, x[mask != 0]), method


def test_probe_refusals_launch_nothing(gpu_engine):
    lib, h = gpu_engine._lib, gpu_engine._h
    a = np.zeros((2, 4096), np.float32)
    out = np.full((2, 4200), 7, np.int64)
    width = ctypes.c_int32(-5)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    ok = dict(method=0, mode=0, rate=22050, threshold=-25., min_silence=0.1, block_size=220, replace_by=100, min_voice_time=0.2,
              what=2)

    def call(audio=a, B=2, N=4096, lengths=None, o=out, w=ctypes.byref(width), mem=0, **kw):
        k = {**ok, **kw}
        return lib.tts_hip_remove_silence_probe(h, p(audio), B, N, lengths, k['method'], k['mode'], k['rate'], k['threshold'],
                                                k['min_silence'], k['block_size'], k['replace_by'], k['min_voice_time'], k['what'],
                                                None if o is None else p(o), w, mem)

    bad = [dict(what=-1), dict(what=5), dict(what=4), dict(method=1, what=0), dict(method=2, threshold=0.025, what=0),
           dict(method=2, threshold=0.025, what=1), dict(method=1, what=4), dict(method=3), dict(mode=4), dict(mode=3, method=1),
           dict(rate=0), dict(block_size=0), dict(replace_by=-1), dict(threshold=float('nan')), dict(min_silence=-0.1),
           dict(method=2, threshold=0.025, min_silence=0.2, what=4), dict(w=None), dict(mem=7), dict(B=65536, N=16),
           dict(lengths=p(np.array([4097, 10], np.int32)))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.tts_hip_last_error(h).startswith(b'remove_silence_probe:'), (kw, lib.tts_hip_last_error(h))
    assert (out == 7).all() and width.value == -5
    assert call(o=None) == 0 and width.value == 4096            # the width alone
    assert call(o=None, what=0) == 0 and width.value == -(-4096 // 220)
    assert (out == 7).all()
    # the engine still works after the refused calls
    assert np.array_equal(gpu_engine.remove_silence(np.ones(5000, np.float32), 16000), np.ones(5000, np.float32))
