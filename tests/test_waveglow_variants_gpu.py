"""GPU half of the WaveGlow-variant matrix (tests/waveglow_cases.py): every case in every precision and fp32 form, layer by
layer against the float64 oracle -- the gated activations of all 8 WN layers of flow 11, layers 0, 1 and 7 of flows 7 and
3 (n_half 3 and 4) from the GPU's own flow input, and the flow state after flows 11, 8, 4 and 0.

Each call first asserts which form and tile family ran (`pick_variant`); the engine's last error goes into the message."""
import numpy as np
import pytest

import waveglow_cases as wc

pytestmark = pytest.mark.gpu


def _last_error(eng):
    msg = eng._lib.tts_hip_last_error(eng._h)
    return msg.decode('utf-8', 'replace') if msg else ''


def _probe(eng, case, precision, form, **kw):
    mel, z = wc.inputs(case)
    eng.set_waveglow_form(form)
    try:
        out = eng.waveglow_probe(mel, z=z, precision=precision, **kw)
        ran = (eng.last_waveglow_form, eng.last_waveglow_tiles)
    finally:
        eng.set_waveglow_form('winograd')
    v = wc.pick_variant(case.B, case.T, precision, form)
    want = ('winograd' if v.wino else 'direct', v.tiles)
    assert ran == want, f'{case.name} {precision} {form}: expected {want}, ran {ran}; last error: {_last_error(eng)!r}'
    return out


def _line(tag, e):
    return f'{tag}: rel {e["rel"]:.2e} edge {e["edge"]:.2e} abs {e["abs"]:.2e}'


@pytest.mark.parametrize('name', [c.name for c in wc.CASES])
def test_waveglow_variant_layers_match_oracle(gpu_engine, name):
    case = wc.CASE_BY_NAME[name]
    ref = wc.flow11_acts(case)
    failures = []
    for precision, form in wc.runs(case):
        v = wc.pick_variant(case.B, case.T, precision, form)
        worst = {'rel': 0.0, 'edge': 0.0, 'abs': 0.0}
        for layer in range(wc.N_LAYERS):
            acts = _probe(gpu_engine, case, precision, form, flow=11, what='acts', layer=layer)
            assert acts.shape == ref[layer].shape and np.isfinite(acts).all()
            e = wc.act_errors(acts, ref[layer], case.T, 1 << layer)
            worst = {k: max(worst[k], e[k]) for k in worst}
            failures += wc.act_failures(e, precision, f'{name} {precision} {form} layer {layer}')
        print(_line(f'{name:8s} BT={case.BT:3d} {precision:5s} {form:16s} {v.tiles:7s} '
                    f'{"wino" if v.wino else "dir "} PR={v.PR:3d} worst of 8 layers', worst))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('name', wc.LATER_FLOW_CASES)
def test_waveglow_variant_later_flows_match_oracle(gpu_engine, name):
    """Layers 0, 1 and 7 of flows 7 and 3 (first-layer taps on 3 and 4 coupling channels), against the oracle run on the
    GPU's own input to that flow: the state after flows 8 and 4, early outputs included."""
    case = wc.CASE_BY_NAME[name]
    mel, _ = wc.inputs(case)
    spect = wc.spect_of(mel, wc.weights64())
    failures = []
    for precision in wc.PRECISIONS:
        for flow in (7, 3):
            state = _probe(gpu_engine, case, precision, 'winograd', flow=flow + 1, what='state')
            ref = wc.flow_acts(state[:, :, :wc.n_half_of(flow)], spect, flow)
            for layer in (0, 1, 7):
                acts = _probe(gpu_engine, case, precision, 'winograd', flow=flow, what='acts', layer=layer)
                e = wc.act_errors(acts, ref[layer], case.T, 1 << layer)
                tag = f'{name} {precision} flow {flow} layer {layer}'
                print(_line(tag, e))
                failures += wc.act_failures(e, precision, tag)
    assert not failures, '\n'.join(failures)


@pytest.fixture(scope='module')
def state_engine():
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.load_state(wc.weights(wc.STATE_END_SCALE))
    eng.finalize()
    yield eng
    eng.close()


@pytest.mark.parametrize('name', wc.STATE_CASES)
def test_waveglow_variant_post_flow_state_matches_oracle(state_engine, name):
    """The flow state after flows 11, 8 (with the appended early output), 4 and 0: the folded skip / `end` conv, affine
    coupling and inverse 1x1 conv of wn_end_fold_kernel in each precision, on weights with end_scale 0.2."""
    case = wc.CASE_BY_NAME[name]
    ref = wc.states(case)
    failures = []
    for precision in wc.PRECISIONS:
        for k in (11, 8, 4, 0):
            out = _probe(state_engine, case, precision, 'winograd', flow=k, what='state')
            assert out.shape == ref[k].shape and np.isfinite(out).all()
            e = wc.state_errors(out, ref[k])
            print(f'{name} {precision} state after flow {k}: rel {e["rel"]:.2e} max_rel {e["max_rel"]:.2e}')
            for m, bound in (('rel', wc.STATE_REL), ('max_rel', wc.STATE_MAX_REL)):
                if not e[m] <= bound[precision]:
                    failures.append(f'{name} {precision} flow {k}: {m} {e[m]:.3e} > {bound[precision]:.1e}')
    assert not failures, '\n'.join(failures)


def test_waveglow_probe_acts_is_the_f32_probe(gpu_engine):
    case = wc.CASE_BY_NAME['t2_b7']
    mel, z = wc.inputs(case)
    a = gpu_engine.waveglow_probe_acts(mel, z=z, flow=11, layer=3)
    b = gpu_engine.waveglow_probe(mel, z=z, precision='f32', flow=11, what='acts', layer=3)
    assert np.array_equal(a, b)
    # and the flow-0 state is the waveform waveglow_infer returns
    s = gpu_engine.waveglow_probe(mel, z=z, precision='f32', flow=0, what='state')
    assert np.array_equal(s.reshape(case.B, -1), gpu_engine.waveglow_infer(mel, z=z))
