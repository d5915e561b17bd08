"""GPU: the fp32 flow end on partial sums (tests/wn_end_cases.py) -- the residual GEMMs of layers 0 .. 6 form the folded skip /
`end` conv's sums while they stream the activations, wn_end_last_kernel adds layer 7 -- in every residual tile family and
both forms, against the float64 oracle; run to run equal to the bit; masked rows of ragged and packed calls inert."""
import numpy as np
import pytest

import waveglow_cases as wc
import wn_end_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def state_engine():
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.load_state(wc.weights(wc.STATE_END_SCALE))
    eng.finalize()
    yield eng
    eng.close()


def _probe(eng, case, form, want_tiles, **kw):
    mel, z = wc.inputs(case)
    eng.set_waveglow_form(form)
    try:
        out = eng.waveglow_probe(mel, z=z, precision='f32', **kw)
        again = eng.waveglow_probe(mel, z=z, precision='f32', **kw)
        ran = (eng.last_waveglow_form, eng.last_waveglow_tiles)
    finally:
        eng.set_waveglow_form('winograd')
    assert ran == ('winograd' if form == 'winograd' else 'direct', want_tiles), f'{case.name} {form}: ran {ran}'
    assert np.array_equal(out, again), f'{case.name} {form} {kw}: two runs differ'
    return out


@pytest.mark.parametrize('name,form,tiles,flows', ec.STATE_RUNS, ids=[f'{r[0]}-{r[1]}' for r in ec.STATE_RUNS])
def test_flow_state_on_partial_sums_matches_oracle(state_engine, name, form, tiles, flows):
    """State after the flows named in STATE_RUNS, end_scale 0.2 weights, bounds STATE_REL / STATE_MAX_REL['f32']; every
    probe runs twice and the two results are equal to the bit."""
    case = wc.CASE_BY_NAME[name]
    ref = wc.states(case) if len(flows) > 1 else {11: ec.state11(case)}
    failures = []
    for k in flows:
        out = _probe(state_engine, case, form, tiles, flow=k, what='state')
        assert out.shape == ref[k].shape and np.isfinite(out).all()
        e = wc.state_errors(out, ref[k])
        print(f'{name} {form} {tiles} state after flow {k}: rel {e["rel"]:.2e} max_rel {e["max_rel"]:.2e}')
        for m, bound in (('rel', wc.STATE_REL), ('max_rel', wc.STATE_MAX_REL)):
            if not e[m] <= bound['f32']:
                failures.append(f'{name} {form} flow {k}: {m} {e[m]:.3e} > {bound["f32"]:.1e}')
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('name,form', ec.ACTS_RUNS, ids=[f'{r[0]}-{r[1]}' for r in ec.ACTS_RUNS])
def test_second_layer_of_flow_11_matches_oracle(gpu_engine, name, form):
    """Layer 1 reads the residual stream that the start conv and layer 0's residual GEMM leave: a wrong start column or
    bias shows here first."""
    case = wc.CASE_BY_NAME[name]
    mel, z = wc.inputs(case)
    gpu_engine.set_waveglow_form(form)
    try:
        acts = gpu_engine.waveglow_probe_acts(mel, z=z, flow=11, layer=1)
        again = gpu_engine.waveglow_probe_acts(mel, z=z, flow=11, layer=1)
    finally:
        gpu_engine.set_waveglow_form('winograd')
    assert np.array_equal(acts, again)
    e = wc.act_errors(acts, wc.flow11_acts(case)[1], case.T, 2)
    print(f'{name} {form} flow 11 layer 1: rel {e["rel"]:.2e} edge {e["edge"]:.2e} abs {e["abs"]:.2e}')
    assert e['rel'] <= wc.ACTS_REL['f32'] and e['edge'] <= wc.ACTS_EDGE_REL['f32']


@pytest.mark.parametrize('packed', (False, True), ids=('ragged', 'packed'))
def test_masked_rows_never_reach_an_output(state_engine, packed):
    """16 rows of up to 9 frames: NaN in the mel and z tails changes no bit of the result, tails are 0, and two runs are
    equal.  (The probe takes no lengths; the state after flow 0 is the waveform, tests/test_waveglow_variants_gpu.py.)"""
    case = wc.CASE_BY_NAME['b16_t9']
    mel, z = wc.inputs(case)
    lengths = [9, 1, 5, 9, 3, 8, 2, 9, 4, 7, 6, 9, 1, 5, 9, 8]
    nan_mel, nan_z = mel.copy(), z.copy()
    for b, n in enumerate(lengths):
        nan_mel[b, n:] = np.nan
        nan_z[b, n * wc.NPH:] = np.nan
    out = state_engine.waveglow_infer(mel, z=z, lengths=lengths, packed=packed)
    assert np.isfinite(out).all()
    assert np.array_equal(state_engine.waveglow_infer(mel, z=z, lengths=lengths, packed=packed), out)
    assert np.array_equal(state_engine.waveglow_infer(nan_mel, z=nan_z, lengths=lengths, packed=packed), out)
    for b, n in enumerate(lengths):
        assert not out[b, n * 256:].any() and out[b, :n * 256].any()
