"""GPU: every tts_hip_waveglow_infer* entry point goes through one front end (csrc/wg_call.h, waveglow_call in csrc/engine.hip;
`HipEngine.waveglow_infer` is one path in front of it).  So every route to one result gives the same bits, every refusal
reads the same through every symbol and launches nothing, and a ragged call over more than one run is its runs.

The shape is the smallest with an empty, a full and a partial row: B = 3, T = 6, lengths (6, 0, 3) -- 18 frames, one gap in the
packed row.  Other tests assert some of these equalities on other inputs (tests/test_waveglow_ragged_gpu.py::
test_ragged_tails, tests/test_row_streams_gpu.py::test_waveglow_row_seeds_equal_explicit_noise); none on these."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, T, LENGTHS = 3, 6, (6, 0, 3)
KEYS, OFFS = (11, 2 ** 63 + 5, 77), (0, 9, 4)
SEED, OFFSET = 5, 3
PCODE = {'f32': 0, 'f16': 1, 'f16x3': 2}
ROWS = {'plain': dict(), 'ragged': dict(lengths=LENGTHS), 'packed': dict(lengths=LENGTHS, packed=True)}
SENTINEL = 7.0

p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr()) if hasattr(a, 'data_ptr') else a.ctypes.data_as(ctypes.c_void_p)
u64 = lambda v: ctypes.c_uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope='module')
def case():
    import torch
    mel = np.random.default_rng(21).uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    z = np.random.default_rng(22).standard_normal((B, T * 32, 8)).astype(np.float32)
    return dict(mel=mel, z=z, dmel=torch.as_tensor(mel).cuda(), dz=torch.as_tensor(z).cuda(),
                lens=np.asarray(LENGTHS, np.int32), keys=np.asarray(KEYS, np.uint64), offs=np.asarray(OFFS, np.uint64))


def _three_routes(eng, case, z=None, **kw):
    """Host arrays, device tensors and a caller's stream, as numpy arrays."""
    import torch
    host = eng.waveglow_infer(case['mel'], z=None if z is None else z.cpu().numpy(), **kw)
    assert isinstance(host, np.ndarray)
    dev = eng.waveglow_infer(case['dmel'], z=z, **kw)
    st = torch.cuda.Stream()
    on_stream = eng.waveglow_infer(case['dmel'], z=z, stream=st, **kw)
    st.synchronize()
    return [host, dev.cpu().numpy(), on_stream.cpu().numpy()]


def _raw(eng, case, sym, mid, tail):
    """A C entry point on host arrays: (h, mel, B, T, *mid, sigma, audio, *tail, TTS_HIP_MEM_HOST) -> audio."""
    out = np.full((B, T * 256), SENTINEL, np.float32)
    rc = getattr(eng._lib, sym)(eng._h, p(case['mel']), B, T, *mid, 1.0, p(out), *tail, 0)
    assert rc == 0, eng._lib.tts_hip_last_error(eng._h)
    return out


def _assert_all_equal(outs, what):
    assert np.isfinite(outs[0]).all() and outs[0].any()
    for i, o in enumerate(outs[1:], 1):
        assert o.shape == outs[0].shape and np.array_equal(o, outs[0]), f'{what}: route {i} differs from route 0'


@pytest.mark.parametrize('rows', ['plain', 'ragged', 'packed'])
@pytest.mark.parametrize('prec', ['f32', 'f16'])
def test_every_route_to_one_result_gives_the_same_bits(gpu_engine, case, prec, rows):
    eng, kw = gpu_engine, dict(precision=prec, **ROWS[rows])
    code = (PCODE[prec],)
    # the caller's z
    outs = _three_routes(eng, case, z=case['dz'], **kw)
    if rows == 'plain':
        sym = {'f32': 'tts_hip_waveglow_infer', 'f16': 'tts_hip_waveglow_infer_f16'}[prec]
        outs.append(_raw(eng, case, sym, (p(case['z']),), ()))
        outs.append(_raw(eng, case, 'tts_hip_waveglow_infer_ragged', (None, p(case['z'])), code))     # lengths = NULL
    else:
        outs.append(_raw(eng, case, f'tts_hip_waveglow_infer_{rows}', (p(case['lens']), p(case['z'])), code))
    _assert_all_equal(outs, f'{prec} {rows} z')
    if rows != 'plain':
        for b, n in enumerate(LENGTHS):
            assert not outs[0][b, n * 256:].any()
    # seed = that z drawn by random_normal
    zs = eng.random_normal((B, T * 32, 8), SEED, OFFSET)
    outs = [eng.waveglow_infer(case['dmel'], z=zs, **kw).cpu().numpy()]
    outs += _three_routes(eng, case, seed=SEED, offset=OFFSET, **kw)
    if rows == 'plain':
        outs.append(_raw(eng, case, 'tts_hip_waveglow_infer_seeded', (u64(SEED), u64(OFFSET)), code))
    _assert_all_equal(outs, f'{prec} {rows} seed')
    # row_seeds = that z drawn by random_normal_rows (only a row's real frames are drawn: the rest is never read)
    counts = None if rows == 'plain' else [n * 256 for n in LENGTHS]
    zr = eng.random_normal_rows(T * 256, KEYS, OFFS, counts=counts).view(B, T * 32, 8)
    outs = [eng.waveglow_infer(case['dmel'], z=zr, **kw).cpu().numpy()]
    outs += _three_routes(eng, case, row_seeds=(KEYS, OFFS), **kw)
    outs.append(_raw(eng, case, 'tts_hip_waveglow_infer_rows_seeded',
                     (None if rows == 'plain' else p(case['lens']), p(case['keys']), p(case['offs'])), code + (int(rows == 'packed'),)))
    _assert_all_equal(outs, f'{prec} {rows} row_seeds')


# ---- refusals ----------------------------------------------------------------------------------------------------------------
SYMBOLS = ['tts_hip_waveglow_infer', 'tts_hip_waveglow_infer_f16', 'tts_hip_waveglow_infer_f16x3', 'tts_hip_waveglow_infer_seeded',
           'tts_hip_waveglow_infer_async', 'tts_hip_waveglow_infer_ragged', 'tts_hip_waveglow_infer_ragged_async',
           'tts_hip_waveglow_infer_packed', 'tts_hip_waveglow_infer_packed_async', 'tts_hip_waveglow_infer_rows_seeded',
           'tts_hip_waveglow_infer_rows_seeded_async']
PER_PRECISION = SYMBOLS[:3]               # no precision argument
has_rows = lambda s: 'rows_seeded' in s
takes_lengths = lambda s: any(k in s for k in ('ragged', 'packed', 'rows_seeded'))
is_async = lambda s: s.endswith('_async')

BAD_LENGTHS = np.asarray((6, 7, 3), np.int32)
LONG_LENGTHS = np.asarray((16000, 16000, 0), np.int32)                      # F = 32000 + 4 gap frames > 31744
# reason -> (overrides of the good call, substring of the message, the symbols and packed flags it applies to)
REASONS = {
    'mel NULL': (dict(mel=None), 'bad argument', lambda s, packed: True),
    'audio NULL': (dict(audio=None), 'bad argument', lambda s, packed: True),
    'B = 0': (dict(B=0), 'B = 0', lambda s, packed: True),
    'T = 0': (dict(T=0), 'bad argument', lambda s, packed: True),
    'B * T above 2^25': (dict(B=2049, T=16384), 'B*T too large', lambda s, packed: True),
    'precision': (dict(precision=3), 'precision', lambda s, packed: s not in PER_PRECISION),
    'mem kind': (dict(mem=7), 'bad mem kind 7', lambda s, packed: not is_async(s)),
    'packed without lengths': (dict(lengths=None), 'packed needs lengths', lambda s, packed: packed),
    'lengths[1] above T': (dict(lengths=BAD_LENGTHS), 'lengths[1] = 7', lambda s, packed: takes_lengths(s)),
    'T above one run': (dict(B=1, T=31745, lengths=None), 'windowed inference', lambda s, packed: not packed),
    'F above one run': (dict(T=16000, lengths=LONG_LENGTHS), 'F = 32004 frames', lambda s, packed: packed),
    'keys NULL': (dict(keys=None), 'NULL', lambda s, packed: has_rows(s)),
    'offsets NULL': (dict(offsets=None), 'NULL', lambda s, packed: has_rows(s)),
}


def _c_args(sym, c, packed):
    if has_rows(sym):
        mid, tail = (p(c['lengths']), p(c['keys']), p(c['offsets'])), (c['precision'], int(packed))
    elif sym.endswith('_seeded'):
        mid, tail = (u64(SEED), u64(OFFSET)), (c['precision'],)
    elif takes_lengths(sym):
        mid, tail = (p(c['lengths']), p(c['z'])), (c['precision'],)
    else:
        mid, tail = (p(c['z']),), (() if sym in PER_PRECISION else (c['precision'],))
    return (p(c['mel']), c['B'], c['T']) + mid + (1.0, p(c['audio'])) + tail + (c['stream'] if is_async(sym) else c['mem'],)


@pytest.mark.parametrize('sym', SYMBOLS)
def test_refusals_through_every_entry_point(gpu_engine, case, sym):
    """Each reason that applies to the symbol: TTS_HIP_EINVAL, the symbol and the reason in the message, and nothing copied or
    launched: the audio buffer keeps its bytes.  (Device buffers: a refused call must not touch them, whatever sizes it named.)"""
    import torch
    lib, h = gpu_engine._lib, gpu_engine._h
    audio = torch.full((B, T * 256), SENTINEL, device='cuda')
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    good = dict(mel=case['dmel'], B=B, T=T, lengths=case['lens'], z=case['dz'], keys=case['keys'], offsets=case['offs'],
                audio=audio, precision=0, mem=1, stream=ctypes.c_void_p(int(st.cuda_stream)))
    ran = 0
    for packed in ([False, True] if has_rows(sym) else ['packed' in sym]):
        for reason, (override, needle, applies) in REASONS.items():
            if not applies(sym, packed):
                continue
            rc = getattr(lib, sym)(h, *_c_args(sym, dict(good, **override), packed))
            msg = lib.tts_hip_last_error(h).decode()
            assert rc == -1 and sym + ':' in msg and needle in msg, (reason, packed, rc, msg)
            ran += 1
    assert ran >= 6
    gpu_engine.synchronize()
    st.synchronize()
    assert bool((audio == SENTINEL).all())
    rc = getattr(lib, sym)(h, *_c_args(sym, good, 'packed' in sym))             # and the good call is a good call
    assert rc == 0, lib.tts_hip_last_error(h)
    gpu_engine.synchronize()
    st.synchronize()
    assert bool(torch.isfinite(audio).all()) and not bool((audio == SENTINEL).any())


# ---- a ragged call over more than one run -------------------------------------------------------------------------------------
def test_ragged_call_over_two_runs_is_its_runs(gpu_engine):
    """T = 15873: one row per run (2 x 15873 > 31744), so the two-row call is two one-row ragged runs, each with its own slice
    of the staged tail list -- bit-equal to the one-row calls, no tolerance."""
    import torch
    T2, lengths = 15873, (40, 15873)
    g = torch.Generator(device='cuda').manual_seed(3)
    mel = torch.rand((2, T2, 80), device='cuda', generator=g) * 12.7 - 11.5
    z = torch.randn((2, T2 * 32, 8), device='cuda', generator=g)
    both = gpu_engine.waveglow_infer(mel, z=z, precision='f16', lengths=lengths)
    assert bool(torch.isfinite(both).all())
    for b, n in enumerate(lengths):
        one = gpu_engine.waveglow_infer(mel[b:b + 1].contiguous(), z=z[b:b + 1].contiguous(), precision='f16', lengths=lengths[b:b + 1])
        assert torch.equal(one[0], both[b]), f'row {b}'
        assert bool(both[b, :n * 256].any()) and not bool(both[b, n * 256:].any())
