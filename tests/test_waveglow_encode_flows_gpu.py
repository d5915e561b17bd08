"""GPU: the forward flow (tts_hip_waveglow_encode) flow by flow against float64, through its test hook
(HipEngine.waveglow_encode_probe, tts_hip_waveglow_encode_probe), and its row statistics recomputed from its own z and sums.

One test is one (case, form, flow k): the input of flow k is the GPU's own stored state after flow k - 1, the reference is
`waveglow_encode_ref.flow_step` on that input in float64 (one WN block of the oracle), and three things are compared -- the
stored state after flow k, the increment of the per-position sum of s, and (flows 3, 7, 11) the channels the plain call's z
gets from this flow.  Every call first asserts which form and tile family ran (`waveglow_cases.pick_variant`).

Bounds.  The floor of each quantity is the RMS distance of the float32 run of `flow_step` on the same input from the float64
run -- from the restatement alone -- and the engine is allowed TEN floors (waveglow_encode_ref.StepCheck; the margin of
waveglow_encode_ref.Case).  The channels that leave after flows 3 and 7 are passed on untouched by the coupling: floor 0, they
must be the input's bits.  Positions behind a row's length must be exactly 0 and are left out of every RMS.
Statistics: the kernels add float64 terms and store one float32, so |stat - float64 sum of the GPU's own terms| <=
2^-23 |value| + 1e-12 sum |term| (the second term: another float64 order); stats[2] within 2^-23 relative of
lengths[b] * 32 * sum log|det| in float64; an empty row's statistics exactly 0.  Derived, not measured.

Cases (frames; what pick_variant says must run): b5_t13 ragged (65, direct, 128x64, phase blocks padded by 63), b16_t9 (144,
the Winograd start, 64-row: init and all twelve flows in both forms, and flows 3, 4, 7, 8 on non-orthogonal kernels), 9 x 16
ragged with 113 real frames of 144 (Winograd: the PADDED count selects the form) and 12 x 16 ragged with 161 real frames,
b2_t128 (256-row), b1_t257 (64-row padded by 63; one row of 257 frames: the statistics kernel's stride runs twice), b1_t383
(128-row padded by one), 256 channels at 1 x 150 (direct, 64-row, three blocks per phase).

Measured on MI355X, worst over the flows of a case, in floors (state and final channels / slog increment; the channels that
leave after flows 3 and 7 were the input's bits everywhere):
  b5_t13_ragged    direct   128x64   1.34 / 1.59        b16_t9           winograd 64-row   1.87 / 2.14
  b16_t9_direct    direct   64-row   1.35 / 1.49        b16_t9_replaced  winograd 64-row   1.71 / 2.51
  c256_b1_t150     direct   64-row   1.30 / 1.38        b9_t16_ragged    winograd 64-row   1.75 / 1.91
  (the init step: 1.00 in every case)                   b12_t16_ragged   winograd 64-row   1.76 / 1.94
                                                        b2_t128          winograd 256-row  1.65 / 1.78
                                                        b1_t257          winograd 64-row   1.64 / 1.78
                                                        b1_t383          winograd 128-row  1.62 / 1.75
State floors 5.9e-8 .. 8.7e-8 RMS (general kernels: up to 2.6e-7), slog floors 0.9e-7 .. 1.5e-7.  The Winograd form sits about
0.4 floors above the direct one, as in the inverse direction (6.0e-7 against 5.0e-7, include/tts_hip.h).  Statistics: at most
0.4 of their bound; stats[2] equal to the float32 of the float64 product in every row.  Nothing failed.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np
import pytest

import waveglow_cases as wc
import waveglow_encode_ref as ref

pytestmark = pytest.mark.gpu

ALL_STEPS = tuple(range(-1, 12))


class Case(NamedTuple):
    name: str
    B: int
    T: int
    steps: tuple                        # -1: the init step, 0 .. 11: flows
    ran: tuple                          # (form, tile family) the call must report
    forms: tuple = ('winograd',)        # the handle's form setting(s); 'winograd' is its default
    lengths: Optional[tuple] = None
    model: str = 'session'              # 'session' | 'replaced' (replace_invertible_kernels) | 'c256' (n_channels = 256)


CASES = (
    Case('b5_t13_ragged', 5, 13, (-1, 0, 3, 7, 11), ('direct', '128x64'), lengths=(13, 0, 6, 13, 1)),
    Case('b16_t9', 16, 9, ALL_STEPS, ('winograd', '64-row')),
    Case('b16_t9_direct', 16, 9, ALL_STEPS, ('direct', '64-row'), forms=('direct',)),
    Case('b16_t9_replaced', 16, 9, (3, 4, 7, 8), ('winograd', '64-row'), model='replaced'),
    # 113 real frames in 144 padded ones: below the Winograd start by the real count, at it by the padded one
    Case('b9_t16_ragged', 9, 16, (0, 3, 11), ('winograd', '64-row'), lengths=(16, 0, 1, 16, 16, 16, 16, 9, 7)),
    # ... and a batch that is at the Winograd start by both counts (161 real frames of 192)
    Case('b12_t16_ragged', 12, 16, (0, 3, 11), ('winograd', '64-row'), lengths=(16, 0, 1, 16, 16, 16, 16, 16, 16, 16, 9, 7)),
    Case('b2_t128', 2, 128, (0, 11), ('winograd', '256-row')),
    Case('b1_t257', 1, 257, (0, 7, 11), ('winograd', '64-row')),
    Case('b1_t383', 1, 383, (11,), ('winograd', '128-row')),
    Case('c256_b1_t150', 1, 150, (0, 7, 11), ('direct', '64-row'), model='c256'),
)
CASE_BY_NAME = {c.name: c for c in CASES}
# the statistics: a row above 256 frames without lengths, ragged rows of 300 / 257 / 0 frames, and tails in the Winograd form
STAT_CASES = (
    Case('b1_t257', 1, 257, (), ('winograd', '64-row'), model='replaced'),
    Case('b3_t300_ragged', 3, 300, (), ('winograd', '256-row'), lengths=(300, 257, 0), model='replaced'),
    Case('b9_t16_ragged', 9, 16, (), ('winograd', '64-row'), lengths=(16, 0, 1, 16, 16, 16, 16, 9, 7), model='replaced'),
)


def test_case_table_reaches_what_it_names():
    """(no GPU work) The dispatch rules agree with the table, which reaches the Winograd form, every fp32 tile family and both
    selections of the ragged Winograd cases."""
    for c in CASES + STAT_CASES:
        form = c.forms[0] if c.model != 'c256' else 'direct'           # the Winograd form is a 512-channel form
        v = wc.pick_variant(c.B, c.T, 'f32', form)
        assert ('winograd' if v.wino else 'direct', v.tiles) == c.ran, c.name
    assert {c.ran[1] for c in CASES} == {'64-row', '128x64', '128-row', '256-row'}
    assert {c.ran for c in CASES if c.model != 'c256'} >= {('winograd', '64-row'), ('winograd', '128-row'), ('winograd', '256-row')}
    a, b = CASE_BY_NAME['b9_t16_ragged'], CASE_BY_NAME['b12_t16_ragged']
    assert sum(a.lengths) < wc.WINO_MIN_FRAMES <= a.B * a.T and wc.WINO_MIN_FRAMES <= sum(b.lengths)
    for c in (a, b):
        assert {0, 1, c.T} <= set(c.lengths) and any(1 < n < c.T for n in c.lengths)
    # encode_stats_partial_kernel gives each of its 32 blocks per row ceil(frames * 32 / 32) positions: above 256 frames a
    # block's 256 threads take a second pass
    assert sum(max(c.lengths or (c.T,)) > 256 for c in STAT_CASES) == 2
    assert wc.pick_variant(1, 257, 'f32').PR == 320 and wc.pick_variant(1, 383, 'f32').PR == 384
    assert wc.pick_variant(5, 13, 'f32').PR == 128 and wc.pick_variant(2, 128, 'f32').PR == 256


# ---- models, inputs and the oracle's conditioning, once per module
@pytest.fixture(scope='module')
def models(gpu_engine, wg_weights, wg_cfg):
    """name -> (engine, weights, config); the 'replaced' and 'c256' engines are made on first use."""
    from text_to_speech_amd import weights
    from text_to_speech_amd.config import WaveGlowConfig
    from text_to_speech_amd.engine import HipEngine
    made, own = {'session': (gpu_engine, wg_weights, wg_cfg)}, []

    def get(name):
        if name not in made:
            cfg = wg_cfg if name == 'replaced' else WaveGlowConfig(n_channels=256)
            w = ref.replace_invertible_kernels(wg_weights, wg_cfg) if name == 'replaced' else weights.synth_waveglow(cfg, seed=1234)
            eng = HipEngine(0)
            eng.load_state(w)
            eng.finalize()
            own.append(eng)
            made[name] = (eng, w, cfg)
        return made[name]
    yield get
    for eng in own:
        eng.close()


@functools.lru_cache(maxsize=None)
def _inputs(B, T, lengths):
    """(audio, mel, the same with NaN behind every row's length)."""
    rng = np.random.default_rng(4100 + 100 * B + T)
    mel = rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    audio = rng.uniform(-0.9, 0.9, (B, T * 256)).astype(np.float32)
    nan_audio, nan_mel = audio.copy(), mel.copy()
    for b, n in enumerate(lengths or ()):
        nan_audio[b, n * 256:] = np.nan
        nan_mel[b, n:] = np.nan
    for a in (audio, mel, nan_audio, nan_mel):
        a.setflags(write=False)
    return audio, mel, nan_audio, nan_mel


_spect, _probes = {}, {}


def _spect_groups(case, w, cfg):
    """The oracle's conditioning of each row group in float64 and float32, cached (it does not depend on the kernels)."""
    key = (case.B, case.T, case.lengths, cfg.n_channels)
    if key not in _spect:
        mel = _inputs(case.B, case.T, case.lengths)[1]
        _spect[key] = [{dt: ref.spect_of(mel[rows, :n], w, cfg, dt) for dt in (np.float64, np.float32)}
                       for rows, n in ref.row_groups(case.B, case.T, case.lengths)]
    return _spect[key]


def _last_error(eng):
    msg = eng._lib.tts_hip_last_error(eng._h)
    return msg.decode('utf-8', 'replace') if msg else ''


def _run(eng, case, form, call):
    """call(audio, mel, lengths) under the handle's form `form`, with NaN behind the lengths; asserts what ran."""
    _, _, audio, mel = _inputs(case.B, case.T, case.lengths)
    eng.set_waveglow_form(form)
    try:
        out = call(audio, mel, None if case.lengths is None else list(case.lengths))
        ran = (eng.last_waveglow_form, eng.last_waveglow_tiles)
    finally:
        eng.set_waveglow_form('winograd')
    assert ran == case.ran, f'{case.name} {form}: expected {case.ran}, ran {ran}; last error: {_last_error(eng)!r}'
    return out


def _probe(eng, case, form, flow, what):
    """The probe's answer, kept per module: flow k's output is flow k + 1's input (the repeat test shows repeats are bit-equal)."""
    key = (case.name, form, flow, what)
    if key not in _probes:
        out = _run(eng, case, form, lambda a, m, l: eng.waveglow_encode_probe(a, m, lengths=l, flow=flow, what=what))
        out.setflags(write=False)
        _probes[key] = out
    return _probes[key]


def _z(eng, case, form):
    key = (case.name, form, 'z')
    if key not in _probes:
        _probes[key] = _run(eng, case, form, lambda a, m, l: eng.waveglow_encode(a, m, lengths=l))
    return _probes[key]


def _assert_zero_behind(case, x, what):
    for b, n in enumerate(case.lengths or ()):
        assert not x[b, n * 32:].any(), f'{case.name}: {what} of row {b} is not 0 behind its {n} frames'


STEP_PARAMS = [pytest.param(c.name, form, k, id=f'{c.name}-{form}-flow{k}') for c in CASES for form in c.forms for k in c.steps]


@pytest.mark.parametrize('name,form,k', STEP_PARAMS)
def test_one_flow_matches_float64(models, name, form, k):
    case = CASE_BY_NAME[name]
    eng, w, cfg = models(case.model)
    audio = _inputs(case.B, case.T, case.lengths)[0]
    n_out = 8 if k <= 2 else 6 if k <= 6 else 4
    state_in = audio.reshape(case.B, -1, 8) if k < 0 else _probe(eng, case, form, k - 1, 'state')
    state_out = _probe(eng, case, form, k, 'state')
    assert state_out.shape == (case.B, case.T * 32, n_out) and state_out.dtype == np.float32
    inc = z = None
    if k >= 0:
        slog = _probe(eng, case, form, k, 'slog')
        assert slog.shape == (case.B, case.T * 32)
        inc = slog.astype(np.float64) - (_probe(eng, case, form, k - 1, 'slog') if k > 0 else 0.0)
        _assert_zero_behind(case, slog, f'slog after flow {k}')
    if ref.z_slot(k, cfg) is not None and k >= 0:
        z, _ = _z(eng, case, form)
        _assert_zero_behind(case, z, 'z')
    _assert_zero_behind(case, state_out, f'state after flow {k}')
    groups = ref.row_groups(case.B, case.T, case.lengths)
    check = ref.StepCheck(state_in, _spect_groups(case, w, cfg), w, cfg, k, groups)
    f = check.floors(state_out, inc, z)
    print(f'{name} {form} flow {k} ({case.ran[0]}, {case.ran[1]}): ' +
          ', '.join(f'{q} {v:.2f} floors (floor {check.floor_of(q):.2e})' for q, v in f.items()))
    for q in (state_out, inc, z):
        assert q is None or np.isfinite(check.gather(q)).all()
    for q, v in f.items():
        assert v <= ref.StepCheck.MARGIN, f'{name} {form} flow {k}: {q} at {v:.2f} floors'


def test_flow_11_probe_is_the_plain_calls_z(models):
    """What the probe returns after flow 11 is the plain call's z, bit for bit, in a ragged and a Winograd case."""
    for name in ('b5_t13_ragged', 'b16_t9'):
        case = CASE_BY_NAME[name]
        eng, _, _ = models(case.model)
        z, _ = _z(eng, case, 'winograd')
        assert np.array_equal(_probe(eng, case, 'winograd', 11, 'state'), z[:, :, :4])


# ---- the row statistics, recomputed from the GPU's own z and sums
@pytest.mark.parametrize('name', [c.name for c in STAT_CASES])
def test_row_statistics_are_the_float64_sums_of_their_terms(models, name):
    case = {c.name: c for c in STAT_CASES}[name]
    eng, w, cfg = models('replaced')
    z, stats = _run(eng, case, 'winograd', lambda a, m, l: eng.waveglow_encode(a, m, lengths=l))
    slog = _run(eng, case, 'winograd', lambda a, m, l: eng.waveglow_encode_probe(a, m, lengths=l, flow=11, what='slog'))
    assert stats.shape == (3, case.B) and stats.dtype == np.float32
    log_det = float(ref.log_abs_dets(w, cfg).sum())
    assert abs(log_det) > 1.0
    lengths = case.lengths or (case.T,) * case.B
    for b, n in enumerate(lengths):
        if n == 0:
            assert not stats[:, b].any() and not np.signbit(stats[:, b]).any(), f'empty row {b}: {stats[:, b]}'
            continue
        for i, terms in enumerate((np.square(z[b, :n * 32].astype(np.float64)), slog[b, :n * 32].astype(np.float64))):
            want, bound = terms.sum(), 2.0 ** -23 * abs(terms.sum()) + 1e-12 * np.abs(terms).sum()
            err = abs(float(stats[i, b]) - want)
            print(f'{name} row {b} ({n} frames) stats[{i}] = {stats[i, b]!r}: float64 {want!r}, error {err:.3e}, bound {bound:.3e}')
            assert np.isfinite(stats[i, b]) and err <= bound
        want = float(np.float32(n * 32 * log_det))
        print(f'{name} row {b} stats[2] = {stats[2, b]!r}: float64 {n * 32 * log_det!r}')
        assert abs(float(stats[2, b]) - want) <= 2.0 ** -23 * abs(want)


# ---- the hook itself
def test_refusals_through_the_real_symbol(gpu_engine):
    audio, mel = _inputs(2, 5, None)[:2]
    lib, h, ptr = gpu_engine._lib, gpu_engine._h, gpu_engine._ptr
    name = 'tts_hip_waveglow_encode_probe'
    out = np.full((2, 160, 8), 7, np.float32)
    lens = lambda *v: np.array(v, dtype=np.int32)

    def refused(*args):
        rc = getattr(lib, name)(h, *args)
        msg = lib.tts_hip_last_error(h).decode()
        assert rc == -1 and msg.startswith(name + ': '), (rc, msg)
        return msg

    a, m, o = ptr(audio), ptr(mel), ptr(out)
    # everything tts_hip_waveglow_encode refuses, in its order
    assert 'bad mem kind 7' in refused(a, m, 0, 5, None, 0, 0, o, 7)
    assert 'B = 0' in refused(a, m, 0, 0, None, 0, 0, o, 0)
    assert 'T = 0' in refused(a, m, 2, 0, None, 0, 0, o, 0)
    assert 'audio or mel is NULL' in refused(None, m, 2, 5, None, 0, 0, o, 0)
    assert 'audio or mel is NULL' in refused(a, None, 2, 5, None, 0, 0, o, 0)
    assert 'lengths[1] = 9' in refused(a, m, 2, 5, ptr(lens(5, 9)), 0, 0, o, 0)
    assert 'lengths[0] = -1' in refused(a, m, 2, 31744, ptr(lens(-1, 0)), 0, 0, o, 0)
    assert 'exceeds one run' in refused(a, m, 2, 15873, None, 0, 0, o, 0)
    # and its own
    assert 'flow = 12' in refused(a, m, 2, 5, None, 12, 0, o, 0)
    assert 'flow = -2' in refused(a, m, 2, 5, None, -2, 0, o, 0)
    assert 'what = 2' in refused(a, m, 2, 5, None, 3, 2, o, 0)
    assert 'what = -1' in refused(a, m, 2, 5, None, 3, -1, o, 0)
    assert 'needs flow >= 0' in refused(a, m, 2, 5, None, -1, 1, o, 0)
    assert 'out is NULL' in refused(a, m, 2, 5, None, 3, 0, None, 0)
    assert np.all(out == 7)                                                  # nothing was written
    with pytest.raises(ValueError, match='what must be one of'):
        gpu_engine.waveglow_encode_probe(audio, mel, flow=3, what='acts')
    # the edges that are accepted
    assert gpu_engine.waveglow_encode_probe(audio, mel, flow=-1).shape == (2, 160, 8)
    assert gpu_engine.waveglow_encode_probe(audio, mel, flow=11, what='slog').shape == (2, 160)


@pytest.mark.parametrize('name', ['b5_t13_ragged', 'b16_t9'])
def test_probe_leaves_later_calls_their_bits(gpu_engine, name):
    """A plain encode and an infer call right after probe calls return the bits they returned before them; device memory for
    `out` gives the host call's bits; a repeated probe is bit-equal."""
    import torch
    case = CASE_BY_NAME[name]
    audio, mel = _inputs(case.B, case.T, case.lengths)[:2]
    lengths = None if case.lengths is None else list(case.lengths)
    z, stats = gpu_engine.waveglow_encode(audio, mel, lengths=lengths)
    wave = gpu_engine.waveglow_infer(mel, z=None)
    first = {}
    for flow, what in ((5, 'state'), (-1, 'state'), (11, 'slog'), (3, 'slog')):
        first[flow, what] = gpu_engine.waveglow_encode_probe(audio, mel, lengths=lengths, flow=flow, what=what)
        z2, stats2 = gpu_engine.waveglow_encode(audio, mel, lengths=lengths)
        assert np.array_equal(z2, z) and np.array_equal(stats2, stats), (flow, what)
        assert np.array_equal(gpu_engine.waveglow_infer(mel, z=None), wave), (flow, what)
    for (flow, what), out in first.items():
        assert np.array_equal(gpu_engine.waveglow_encode_probe(audio, mel, lengths=lengths, flow=flow, what=what), out)
    # `out` in device memory (mem = 1), through the symbol
    lib, h, ptr = gpu_engine._lib, gpu_engine._h, gpu_engine._ptr
    da, dm = torch.tensor(audio).cuda(), torch.tensor(mel).cuda()          # (copies: the cached inputs are read-only)
    dout = torch.full((case.B, case.T * 32, 6), 7.0, device='cuda')
    lens = None if lengths is None else np.array(lengths, dtype=np.int32)
    assert lib.tts_hip_waveglow_encode_probe(h, ptr(da), ptr(dm), case.B, case.T, ptr(lens), 5, 0, ptr(dout), 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), first[5, 'state'])
