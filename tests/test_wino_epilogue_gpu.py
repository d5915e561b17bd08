"""GPU: the epilogue of the default Winograd WN kernel (csrc/wn_wino.hip, wino4_fused2_kernel) stages the conditioning plane
through LDS by DMA, two tiles per wave, ordered by request counts alone.  The three-pass form's combine kernel reads the same
plane with plain vector loads and writes the output transform identically, so the gated activations of the two forms are EQUAL
bit for bit: a tile read before it landed, a wrong row or a wrong 16-byte piece shows up as a difference -- or as a difference
between two runs of the same call.

Shapes: utterances that end inside a group of four (131, 195, 513 frames; 48 x 3 and 176 x 3 frames, shorter than one group),
calls whose B T is no multiple of 64 (655, 585, 513, 528 frames: padded group rows), all seven Winograd layers of one flow, i.e. all three group
kinds (phase groups d <= 8, mixed groups d = 16, frame groups d >= 32).  The ragged and the packed call are checked at their
outputs: NaN in the caller's tails changes no bit of the audio.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOW = 11


def _inputs(B, T, seed):
    mel = np.random.default_rng(seed).uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    z = np.random.default_rng(seed + 4).standard_normal((B, T * 32, 8)).astype(np.float32)
    return mel, z


# The reference is the three-pass form wherever it exists.  It needs 128-row phase blocks and therefore does not run calls of
# fewer than ~400 frames in the Winograd form at all (csrc/waveglow.hip: such a call takes the direct form, which is not
# bit-identical): 48 x 3 = 144 frames is compared with the OTHER form that reads the plane with plain loads into registers,
# the fused GEMM behind the pre-pass ('winograd-prepass', wino_gate_store), and 176 x 3 = 528 frames -- the same utterances
# shorter than one group, enough of them -- with the three-pass form.
@pytest.mark.parametrize('B,T,reference', [(5, 131, 'winograd-3pass'), (3, 195, 'winograd-3pass'), (1, 513, 'winograd-3pass'),
                                           (176, 3, 'winograd-3pass'), (48, 3, 'winograd-prepass')])
def test_gated_activations_equal_the_three_pass_form_bit_for_bit(gpu_engine, B, T, reference):
    mel, z = _inputs(B, T, seed=100 * B + T)
    try:
        for layer in range(1, 8):
            runs = {}
            for form in (reference, 'winograd', reference, 'winograd'):                         # each comparison twice
                gpu_engine.set_waveglow_form(form)
                acts = gpu_engine.waveglow_probe_acts(mel, z=z, flow=FLOW, layer=layer)
                assert gpu_engine.last_waveglow_form == 'winograd', f'{form} did not run {B} x {T} in the Winograd form'
                assert acts.shape == (B, T * 32, 512) and np.isfinite(acts).all() and acts.any()
                if form in runs:
                    assert np.array_equal(acts, runs[form]), f'{B} x {T} layer {layer}: two runs of {form} differ'
                runs[form] = acts
            diff = runs['winograd'] != runs[reference]
            print(f'{B} x {T} flow {FLOW} layer {layer} (dilation {1 << layer}): {int(diff.sum())} of {diff.size} elements differ')
            assert not diff.any(), f'{B} x {T} layer {layer}: first difference at {np.argwhere(diff)[0]}'
    finally:
        gpu_engine.set_waveglow_form('winograd')


@pytest.mark.parametrize('lengths', [(101, 37, 70), (2, 150, 3), (300, 150, 211)])
@pytest.mark.parametrize('packed', [False, True])
def test_ragged_and_packed_calls_ignore_their_tails(gpu_engine, lengths, packed):
    """Frames past a row's length share a group of four (and a staged tile) with its last real frames: NaN there (mel and
    noise) against -11 / 0 there gives the same audio bit for bit, in two runs each, and zeros past the lengths."""
    B, T = len(lengths), max(lengths) + 2
    mel, z = _inputs(B, T, seed=17)
    clean, dirty = (mel.copy(), z.copy()), (mel.copy(), z.copy())
    for r, n in enumerate(lengths):
        clean[0][r, n:], clean[1][r, n * 32:] = -11.0, 0.0
        dirty[0][r, n:], dirty[1][r, n * 32:] = np.nan, np.nan
    outs = []
    for m2, z2 in (clean, dirty, clean, dirty):
        outs.append(gpu_engine.waveglow_infer(m2, z=z2, lengths=lengths, packed=packed))
        if not packed:
            assert gpu_engine.last_waveglow_form == 'winograd'
    assert np.isfinite(outs[0]).all()
    for out in outs[1:]:
        assert np.array_equal(out, outs[0])
    for r, n in enumerate(lengths):
        assert outs[0][r, :n * 256].any() and not outs[0][r, n * 256:].any()


@pytest.mark.parametrize('packed', [False, True])
def test_ragged_and_packed_calls_equal_the_three_pass_form(gpu_engine, packed):
    """(more than 512 frames per call, where all forms run the same first-layer and residual kernels)"""
    lengths = (300, 150, 211)
    mel, z = _inputs(3, 302, seed=23)
    try:
        outs = {}
        for form in ('winograd-3pass', 'winograd'):
            gpu_engine.set_waveglow_form(form)
            outs[form] = gpu_engine.waveglow_infer(mel, z=z, lengths=lengths, packed=packed)
    finally:
        gpu_engine.set_waveglow_form('winograd')
    assert np.array_equal(outs['winograd'], outs['winograd-3pass'])
