"""GPU: ragged (`lengths=`) and packed (`packed=True`) WaveGlow runs layer by layer in every variant (tests/waveglow_cases.py,
RAGGED_CASES and PACKED_CASES), through the probe that takes lengths (tts_hip_waveglow_probe_rows).

Whether a short row computes what it computes alone rests on one invariant: the residual stream is zero on every frame that
is not real, after every layer, in every precision and tile family.  Here every row's real positions go against the float64
oracle run on THAT ROW'S OWN frames -- the gated activations of all 8 WN layers of flow 11, layers 0, 1 and 7 of flows 7 and
3 from the GPU's own state, the flow state after flows 11, 8, 4 and 0, the Winograd form's conditioning plane -- with the
bounds of the unmasked matrix (waveglow_cases), per row, the row's own ends as edge windows.  mel and z hold NaN behind every
length.  The state must be exactly 0 behind a length and on a gap frame: a tail left unmasked in the init step or in a flow's
end kernel reaches no activation (oracle-only controls, tests/test_waveglow_variants.py).

Each call first asserts which form and tile family ran (`pick_variant` on B x T, or on 1 x F for a packed row)."""
import numpy as np
import pytest

import waveglow_cases as wc
from test_waveglow_variants_gpu import _last_error, _line

pytestmark = pytest.mark.gpu


def _probe(eng, case, precision, form, **kw):
    mel, z = wc.rows_inputs(case)
    eng.set_waveglow_form(form)
    try:
        out = eng.waveglow_probe(mel, z=z, precision=precision, lengths=case.lengths, packed=case.packed, **kw)
        ran = (eng.last_waveglow_form, eng.last_waveglow_tiles)
    finally:
        eng.set_waveglow_form('winograd')
    v = wc.rows_variant(case, precision, form)
    want = ('winograd' if v.wino and eng.waveglow_channels == 512 else 'direct', v.tiles)
    assert ran == want, f'{case.name} {precision} {form}: expected {want}, ran {ran}; last error: {_last_error(eng)!r}'
    assert out.shape[:-1] == ((case.frames * wc.NPH,) if case.packed else (case.B, case.T * wc.NPH)), out.shape
    return out


def _rows(case):
    return [(b, n) for b, n in enumerate(case.lengths) if n > 0]


@pytest.mark.parametrize('name', [c.name for c in wc.ROWS_CASES])
def test_rows_layers_match_each_rows_solo_oracle(gpu_engine, name):
    case = wc.ROWS_CASE_BY_NAME[name]
    failures = []
    for precision, form in wc.runs(case):
        v = wc.rows_variant(case, precision, form)
        worst = {'rel': 0.0, 'edge': 0.0, 'abs': 0.0}
        for layer in range(wc.N_LAYERS):
            acts = _probe(gpu_engine, case, precision, form, flow=11, what='acts', layer=layer)
            for b, n in _rows(case):
                got, ref = wc.row_of(case, acts, b), wc.row_flow11_acts(case, b)[layer]
                assert got.shape == ref.shape and np.isfinite(got).all(), (name, precision, form, layer, b)
                e = wc.act_errors(got, ref, n, 1 << layer)
                worst = {k: max(worst[k], e[k]) for k in worst}
                failures += wc.act_failures(e, precision, f'{name} {precision} {form} layer {layer} row {b} (n={n})')
        print(_line(f'{name:7s} {"packed" if case.packed else "ragged"} frames={case.frames:3d} {precision:5s} {form:16s} '
                    f'{v.tiles:7s} {"wino" if v.wino else "dir "} PR={v.PR:3d} worst of 8 layers x rows', worst))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('name', wc.ROWS_LATER_FLOW_CASES)
def test_rows_later_flows_match_each_rows_solo_oracle(gpu_engine, name):
    """Layers 0, 1 and 7 of flows 7 and 3: the a0p rows of 3 and 4 coupling channels and their constant-1 column, which
    zero_tail(.., with_a0p) must clear -- against the oracle run on each row's own state after flows 8 and 4 (the GPU's)."""
    case = wc.ROWS_CASE_BY_NAME[name]
    spect = {b: wc.spect_of(wc.row_inputs(case, b)[0], wc.weights64()) for b, _ in _rows(case)}
    failures = []
    for precision in wc.PRECISIONS:
        worst = {'rel': 0.0, 'edge': 0.0, 'abs': 0.0}
        for flow in (7, 3):
            state = _probe(gpu_engine, case, precision, 'winograd', flow=flow + 1, what='state')
            assert not wc.not_real(case, state).any()
            acts = {layer: _probe(gpu_engine, case, precision, 'winograd', flow=flow, what='acts', layer=layer) for layer in (0, 1, 7)}
            for b, n in _rows(case):
                ref = wc.flow_acts(wc.row_of(case, state, b)[:, :, :wc.n_half_of(flow)], spect[b], flow)
                for layer in (0, 1, 7):
                    e = wc.act_errors(wc.row_of(case, acts[layer], b), ref[layer], n, 1 << layer)
                    worst = {k: max(worst[k], e[k]) for k in worst}
                    failures += wc.act_failures(e, precision, f'{name} {precision} flow {flow} layer {layer} row {b} (n={n})')
        print(_line(f'{name} {precision} flows 7 and 3, layers 0, 1, 7, worst over rows', worst))
    assert not failures, '\n'.join(failures)


@pytest.fixture(scope='module')
def state_engine():
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.load_state(wc.weights(wc.STATE_END_SCALE))
    eng.finalize()
    yield eng
    eng.close()


def _scattered(case, out):
    """A packed probe's [F*32, W] rows in the batch layout [B, T*32, W], zeros behind the lengths: the scatter's mapping."""
    full = np.zeros((case.B, case.T * wc.NPH, out.shape[-1]), out.dtype)
    for b, n in _rows(case):
        full[b, :n * wc.NPH] = wc.row_of(case, out, b)[0]
    return full


@pytest.mark.parametrize('name', wc.ROWS_STATE_CASES)
def test_rows_post_flow_state_matches_each_rows_solo_oracle_and_is_zero_elsewhere(state_engine, name):
    """The flow state after flows 11, 8 (with the appended early output), 4 and 0 on weights with end_scale 0.2: real
    positions per row against the oracle on the row alone; exactly 0 behind every length and on every gap frame, at every
    probed flow; and the state after flow 0 is the waveform the call itself returns, bit for bit."""
    case = wc.ROWS_CASE_BY_NAME[name]
    mel, z = wc.rows_inputs(case)
    failures = []
    for precision in wc.PRECISIONS:
        worst = {'rel': 0.0, 'max_rel': 0.0}
        for k in (11, 8, 4, 0):
            out = _probe(state_engine, case, precision, 'winograd', flow=k, what='state')
            stray = wc.not_real(case, out)
            assert not stray.any(), f'{name} {precision} flow {k}: {np.count_nonzero(stray)} non-zero values on frames that are not real'
            for b, n in _rows(case):
                got, ref = wc.row_of(case, out, b), wc.row_states(case, b)[k]
                assert got.shape == ref.shape and np.isfinite(got).all()
                e = wc.state_errors(got, ref)
                worst = {m: max(worst[m], e[m]) for m in worst}
                for m, bound in (('rel', wc.STATE_REL), ('max_rel', wc.STATE_MAX_REL)):
                    if not e[m] <= bound[precision]:
                        failures.append(f'{name} {precision} flow {k} row {b} (n={n}): {m} {e[m]:.3e} > {bound[precision]:.1e}')
        print(f'{name} {precision} state after flows 11, 8, 4, 0, worst over rows: rel {worst["rel"]:.2e} max_rel {worst["max_rel"]:.2e}')
        audio = state_engine.waveglow_infer(mel, z=z, precision=precision, lengths=case.lengths, packed=case.packed)
        final = _scattered(case, out) if case.packed else out
        assert np.array_equal(final.reshape(case.B, -1), audio), f'{name} {precision}: flow-0 state is not the call\'s waveform'
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('name', wc.ROWS_COND_CASES)
def test_rows_conditioning_plane_matches_each_rows_own(gpu_engine, wg_cfg, name):
    """The Winograd form's conditioning plane of layers 1 - 7 of flow 11 and of (3, 2): a row's real frames against the float64
    conditioning of the row alone (frames behind a length share a group of four with its last real frames; a packed row's
    first frames look back into a gap)."""
    from test_wino_cond_plane_gpu import REL_BOUND, _reference
    from conftest import rms
    case = wc.ROWS_CASE_BY_NAME[name]
    worst = 0.0
    for flow, layer in [(11, i) for i in range(1, 8)] + [(3, 2)]:
        got = _probe(gpu_engine, case, 'f32', 'winograd', flow=flow, what='cond', layer=layer)
        assert got.shape[-1] == 1024
        for b, n in _rows(case):
            ref = _reference(wc.row_inputs(case, b)[0], wc.weights64(), wg_cfg, flow, layer)      # (the session's weights)
            row = wc.row_of(case, got, b)
            assert row.shape == ref.shape and np.isfinite(row).all()
            rel = rms(row - ref) / rms(ref)
            worst = max(worst, rel)
            assert rel <= REL_BOUND, f'{name} flow {flow} layer {layer} row {b} (n={n}): relative RMS {rel:.3e} > {REL_BOUND:.2e}'
    print(f'{name} conditioning plane, worst relative RMS over layers and rows: {worst:.3e}')


# ---- 256 channels: the fp32 end_fold<false, false, MASK_*> pair -------------------------------------------------------------
@pytest.fixture(scope='module')
def cfg256():
    from text_to_speech_amd.config import WaveGlowConfig
    return WaveGlowConfig(n_channels=256)


@pytest.fixture(scope='module')
def w256(cfg256):
    from text_to_speech_amd import weights
    return weights.synth_waveglow(cfg256, seed=1234)


@pytest.fixture(scope='module')
def eng256(w256):
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.load_state(w256)
    eng.finalize()
    yield eng
    eng.close()


@pytest.mark.parametrize('name', wc.ROWS_256_CASES)
def test_rows_state_on_a_256_channel_handle(eng256, w256, cfg256, name):
    """fp32 at 256 channels has no end partial sums: the flow ends in wn_end_fold_kernel<false, false, MASK_*>.  State after
    flows 11 and 0: exactly 0 on frames that are not real, real positions within tests/test_waveglow_channels_gpu.py's bound
    (RMS_TOL, absolute RMS) of the oracle on the row alone."""
    from conftest import rms
    from oracle import waveglow_ref
    from test_waveglow_gpu import RMS_TOL
    case = wc.ROWS_CASE_BY_NAME[name]
    assert eng256.waveglow_channels == 256
    refs = {}
    for b, _ in _rows(case):
        mel, z = wc.row_inputs(case, b)
        refs[b] = waveglow_ref.infer(mel, w256, cfg256, z=z, sigma=1.0, return_intermediates=True)[1]
    for k in (11, 0):
        out = _probe(eng256, case, 'f32', 'winograd', flow=k, what='state')
        assert not wc.not_real(case, out).any(), (name, k)
        for b, n in _rows(case):
            got, ref = wc.row_of(case, out, b), refs[b][f'audio_after_flow_{k}']
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = rms(got - ref)
            print(f'C=256 {name} state after flow {k} row {b} (n={n}): rms_err={err:.3e} (state RMS {rms(ref):.3f})')
            assert rms(ref) > 0.1 and err <= RMS_TOL


# ---- the probe without lengths is the old probe -----------------------------------------------------------------------------
@pytest.mark.parametrize('precision,what,kw', [('f32', 'acts', dict(flow=11, layer=3)), ('f16', 'state', dict(flow=8)),
                                               ('f16x3', 'acts', dict(flow=7, layer=0))])
def test_probe_rows_without_lengths_is_the_probe_bit_for_bit(gpu_engine, precision, what, kw):
    """tts_hip_waveglow_probe_rows(lengths = NULL, packed = 0) against tts_hip_waveglow_probe on the same arguments."""
    case = wc.CASE_BY_NAME['t2_b7']
    mel, z = wc.inputs(case)
    eng = gpu_engine
    old = eng.waveglow_probe(mel, z=z, precision=precision, what=what, **kw)
    code = {'acts': 0, 'state': 1}[what]
    new = eng._call('waveglow_probe_rows', [(mel, None, 'float32'), (z, None, 'float32')], lambda make: (make(old.shape),),
                    lambda ins, outs, where: (ins[0], case.B, case.T, None, 0, ins[1], 1.0, eng._WG_PRECISIONS[precision],
                                              kw['flow'], code, kw.get('layer', 0), outs[0]))[0]
    assert np.array_equal(old, new) and np.isfinite(new).all() and new.any()


def test_probe_rows_refusals_name_the_symbol(gpu_engine):
    from text_to_speech_amd._lib import HipLibraryError
    mel = np.zeros((2, 3, 80), np.float32)
    with pytest.raises(HipLibraryError, match=r'tts_hip_waveglow_probe_rows: flow = 12 is outside'):
        gpu_engine.waveglow_probe(mel, lengths=[3, 1], flow=12)
    with pytest.raises(HipLibraryError, match=r'tts_hip_waveglow_probe: layer = 8 is outside'):
        gpu_engine.waveglow_probe(mel, layer=8)
    with pytest.raises(HipLibraryError, match=r'tts_hip_waveglow_probe_rows: what = 2 \(cond\) needs precision 0'):
        gpu_engine.waveglow_probe(mel, lengths=[3, 1], packed=True, what='cond', layer=1, precision='f16')
