"""GPU: the first WN layer of a flow in the Winograd form (csrc/wn_wino.hip, wino_layer0_kernel): the conditioning as the
frame-axis F(4, 4) products of the plane kernel on the layer's own weight planes, the three composed taps as one K = 16 MFMA
chunk per output frame in the epilogue, bias, gate (tanh and sigmoid halves exchanged between two waves through LDS) and store
-- in place of the direct K = 320 + 48 GEMM, in every Winograd-form call whatever its form or tile family.

Measured on one MI355X (worst over the flows 11, 5, 0 -- taps on 2, 3, 4 coupling channels -- of each shape; `edge`: the
positions within d = 1 of an utterance's ends, where a tap leaking across an utterance boundary or a missing bias indicator
shows):
                 this kernel                              the direct GEMM it replaces (parent commit)
    3 x 131      rel 1.30e-06  edge 1.74e-06  abs 2.70e-05    rel 1.07e-06  edge 1.02e-06  abs 1.47e-05
    48 x 3       rel 1.71e-06  edge 1.93e-06  abs 3.44e-05    rel 8.80e-07  edge 9.14e-07  abs 1.15e-05
    1 x 256      rel 1.30e-06  edge 1.59e-06  abs 3.36e-05    rel 1.07e-06  edge 1.21e-06  abs 1.68e-05
(the conditioning's F(4, 4) rounding, 4.4e-7 against 1.7e-7 relative, is what the difference is made of).
The bounds below are 10 x the worst of the new kernel's column (this file's convention, as tests/test_wino_cond_plane_gpu.py);
all of them lie inside waveglow_cases' fp32 bounds, which tests/test_waveglow_variants_gpu.py applies to the same layer.
"""
import numpy as np
import pytest

import waveglow_cases as wc

pytestmark = pytest.mark.gpu

L0_REL, L0_EDGE, L0_ABS = 1.71e-5, 1.93e-5, 3.44e-4

SHAPES = [(3, 131), (48, 3), (1, 256)]            # a partial last group; utterances shorter than a group; whole groups
FLOWS = (11, 5, 0)                                # n_half 2, 3, 4


def _inputs(B, T, seed):
    mel = np.random.default_rng(seed).uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    z = np.random.default_rng(seed + 4).standard_normal((B, T * 32, 8)).astype(np.float32)
    return mel, z


@pytest.mark.parametrize('B,T', SHAPES)
def test_layer0_activations_match_the_float64_oracle(gpu_engine, B, T):
    mel, z = _inputs(B, T, seed=7 * B + T)
    spect = wc.spect_of(mel, wc.weights64())
    worst = {'rel': 0.0, 'edge': 0.0, 'abs': 0.0}
    for flow in FLOWS:
        h = wc.n_half_of(flow)
        if flow == 11:
            a0 = z[:, :, :h]
        else:                                     # the oracle runs on the GPU's own input to the flow
            a0 = gpu_engine.waveglow_probe(mel, z=z, precision='f32', flow=flow + 1, what='state')[:, :, :h]
        ref = wc.flow_acts(a0, spect, flow, stop_after=0)[0]
        acts = gpu_engine.waveglow_probe_acts(mel, z=z, flow=flow, layer=0)
        assert gpu_engine.last_waveglow_form == 'winograd'
        assert acts.shape == (B, T * 32, 512) and np.isfinite(acts).all()
        e = wc.act_errors(acts, ref, T, 1)
        print(f'{B} x {T} flow {flow} (h = {h}) layer 0: rel {e["rel"]:.2e} edge {e["edge"]:.2e} abs {e["abs"]:.2e}')
        worst = {k: max(worst[k], e[k]) for k in worst}
    print(f'{B} x {T} worst of flows {FLOWS}: rel {worst["rel"]:.2e} edge {worst["edge"]:.2e} abs {worst["abs"]:.2e}')
    assert worst['rel'] <= L0_REL and worst['edge'] <= L0_EDGE and worst['abs'] <= L0_ABS
    assert not wc.act_failures(worst, 'f32', f'{B} x {T}')


def test_layer0_bits_do_not_depend_on_the_form(gpu_engine):
    try:
        for (B, T), forms in (((3, 195), ('winograd', 'winograd-3pass', 'winograd-prepass')), ((48, 3), ('winograd', 'winograd-prepass'))):
            mel, z = _inputs(B, T, seed=100 * B + T)
            runs = []
            for form in forms + forms:                                        # two runs each
                gpu_engine.set_waveglow_form(form)
                acts = gpu_engine.waveglow_probe_acts(mel, z=z, flow=5, layer=0)
                assert gpu_engine.last_waveglow_form == 'winograd', f'{form} did not run {B} x {T} in the Winograd form'
                assert np.isfinite(acts).all() and acts.any()
                runs.append(acts)
            for form, acts in zip(forms + forms, runs[1:]):
                assert np.array_equal(acts, runs[0]), f'{B} x {T}: layer 0 of {form} differs from the first run'
    finally:
        gpu_engine.set_waveglow_form('winograd')


def test_layer0_bits_do_not_depend_on_the_tile_family(gpu_engine):
    """1 x 150 frames (64-row tiles) and 1 x 600 frames (128-row tiles) whose first 150 frames coincide: the upsampling is
    causal and layer 0's taps reach one position, so the first 100 frames depend on the common prefix only -- for the oracle
    (checked here, to the last bit) and, group for group, for the kernel."""
    mel, z = _inputs(1, 600, seed=31)
    short = (np.ascontiguousarray(mel[:, :150]), np.ascontiguousarray(z[:, :150 * 32]))
    n = 100 * 32
    w = wc.weights64()
    ref = [wc.flow_acts(zz[:, :, :2], wc.spect_of(mm, w), 11, stop_after=0)[0][:, :n] for mm, zz in (short, (mel, z))]
    assert np.array_equal(ref[0], ref[1]), 'the oracle itself differs on the common prefix'
    acts, tiles = [], []
    for mm, zz in (short, (mel, z)):
        acts.append(gpu_engine.waveglow_probe_acts(mm, z=zz, flow=11, layer=0)[:, :n])
        assert gpu_engine.last_waveglow_form == 'winograd'
        tiles.append(gpu_engine.last_waveglow_tiles)
    assert tiles == ['64-row', '128-row'], tiles
    e = wc.act_errors(acts[0], ref[0], 100, 1)
    assert e['rel'] <= L0_REL and e['abs'] <= L0_ABS
    diff = acts[0] != acts[1]
    assert not diff.any(), f'{int(diff.sum())} elements differ, first at {np.argwhere(diff)[0]}'


def test_ragged_row_equals_its_own_call(gpu_engine):
    """(150, 147, 3) frames: row 1 against a one-row call of its 147 frames, both in the Winograd form.  The probe takes no
    lengths, so the comparison is at the audio, with the re-association tolerance of tests/test_waveglow_ragged_gpu.py."""
    lengths = (150, 147, 3)
    mel, z = _inputs(3, 150, seed=53)
    full = gpu_engine.waveglow_infer(mel, z=z, lengths=lengths)
    assert gpu_engine.last_waveglow_form == 'winograd' and np.isfinite(full).all()
    single = gpu_engine.waveglow_infer(np.ascontiguousarray(mel[1:2, :147]), z=np.ascontiguousarray(z[1:2, :147 * 32]))
    assert gpu_engine.last_waveglow_form == 'winograd'
    err = float(np.sqrt(np.mean((single[0].astype(np.float64) - full[1, :147 * 256]) ** 2)))
    print(f'row 1 (147 frames) against its own call: rms diff {err:.3e}')
    assert err <= 5e-6
    for b, n in enumerate(lengths):
        assert full[b, :n * 256].any() and not full[b, n * 256:].any()


@pytest.mark.parametrize('packed', [False, True])
def test_nan_tails_reach_no_sample(gpu_engine, packed):
    """(4, 151, 1) frames: a row that ends on a group boundary and a single frame.  NaN past the lengths (mel and noise)
    against -11 / 0 there: the same audio bit for bit, twice each."""
    lengths = (4, 151, 1)
    B, T = len(lengths), max(lengths) + 2
    mel, z = _inputs(B, T, seed=19)
    clean, dirty = (mel.copy(), z.copy()), (mel.copy(), z.copy())
    for r, n in enumerate(lengths):
        clean[0][r, n:], clean[1][r, n * 32:] = -11.0, 0.0
        dirty[0][r, n:], dirty[1][r, n * 32:] = np.nan, np.nan
    outs = []
    for m2, z2 in (clean, dirty, clean, dirty):
        outs.append(gpu_engine.waveglow_infer(m2, z=z2, lengths=lengths, packed=packed))
        assert gpu_engine.last_waveglow_form == 'winograd'
    assert np.isfinite(outs[0]).all()
    for out in outs[1:]:
        assert np.array_equal(out, outs[0])
    for r, n in enumerate(lengths):
        assert outs[0][r, :n * 256].any() and not outs[0][r, n * 256:].any()
