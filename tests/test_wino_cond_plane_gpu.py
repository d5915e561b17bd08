"""GPU: the conditioning plane of the fp32 Winograd WN layers (csrc/wn_wino.hip, wino_cond_kernel: seven K = 80 products per
four frames, F(4,4) along frames) against a float64 evaluation of the reference's conditioning,
cond_layer(regroup(upsample(mel))) + in-layer bias, reached through the probe hook (`waveglow_probe(what='cond')`).

Shapes: partial last groups (3 x 131 frames), utterances shorter than one group of four frames in a call that takes the
Winograd form (48 x 3), and the three group kinds' tile families (256 frames).  The plane of a run with row lengths (ragged
or packed, through `waveglow_probe(.., lengths=)`) is compared row by row in tests/test_waveglow_rows_gpu.py; here the ragged
property is checked once more at the call's output: frames past a row's length share a group with its last real frames, and
NaN there changes no bit of the audio.
"""
import numpy as np
import pytest

from conftest import rms

pytestmark = pytest.mark.gpu

# Worst relative RMS measured on MI355X over the cases below: 8.84e-7 (48 x 3 frames, where every output sums fewer than four
# taps while the transformed operands keep their size; 3 x 131 and 1 x 256 frames: 6.1e-7; the CPU model of the roundings
# predicts 4.4e-7 for full windows).  The bound is 10 x that, the convention of tests/waveglow_cases.py.
REL_MEASURED = 8.84e-7
REL_BOUND = 10 * REL_MEASURED


def _reference(mel, w, cfg, flow, layer):
    """[B, T*32, 1024] float64, columns in the engine's gate-interleaved order: 64 j + c <- tanh channel 32 j + c,
    64 j + 32 + c <- sigmoid channel 32 j + c."""
    from oracle import waveglow_ref
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    spect = waveglow_ref.regroup(waveglow_ref.upsample(np.asarray(mel, dtype=np.float64), w64['waveglow/upsample/kernel'],
                                                       w64['waveglow/upsample/bias'], cfg.upsample_stride), cfg.n_group)
    p = f'waveglow/block-{flow}'
    cond = spect @ w64[f'{p}/cond_layer-{layer}/kernel'][0] + w64[f'{p}/cond_layer-{layer}/bias'] + w64[f'{p}/in_conv-{layer}/bias']
    n = cfg.n_channels
    ch = np.arange(n)
    out = np.empty_like(cond)
    out[..., 64 * (ch // 32) + ch % 32] = cond[..., :n]
    out[..., 64 * (ch // 32) + 32 + ch % 32] = cond[..., n:]
    return out


@pytest.mark.parametrize('B,T', [(3, 131), (48, 3), (1, 256)])
def test_conditioning_plane_against_float64(gpu_engine, wg_weights, wg_cfg, B, T):
    mel = np.random.default_rng(B * 1000 + T).uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    worst = 0.0
    for flow, layer in [(11, i) for i in range(1, 8)] + [(3, 2)]:
        got = gpu_engine.waveglow_probe(mel, flow=flow, what='cond', layer=layer)
        assert gpu_engine.last_waveglow_form == 'winograd'
        ref = _reference(mel, wg_weights, wg_cfg, flow, layer)
        assert got.shape == ref.shape == (B, T * 32, 1024) and np.isfinite(got).all()
        rel = rms(got - ref) / rms(ref)
        worst = max(worst, rel)
        print(f'B={B} T={T} flow {flow} layer {layer}: conditioning plane relative RMS {rel:.3e} (rms {rms(ref):.3f})')
    print(f'B={B} T={T}: worst {worst:.3e}')
    assert worst <= REL_BOUND


def test_conditioning_plane_is_the_same_in_every_form(gpu_engine):
    mel = np.random.default_rng(5).uniform(-11.5, 1.2, (2, 150, 80)).astype(np.float32)
    try:
        planes = []
        for form in ('winograd', 'winograd-3pass', 'winograd-prepass'):
            gpu_engine.set_waveglow_form(form)
            planes.append(gpu_engine.waveglow_probe(mel, flow=11, what='cond', layer=4))
    finally:
        gpu_engine.set_waveglow_form('winograd')
    assert np.array_equal(planes[0], planes[1]) and np.array_equal(planes[0], planes[2])


def test_plane_needs_the_winograd_form(gpu_engine):
    mel = np.zeros((1, 16, 80), np.float32)                  # 16 frames: the direct form, no plane
    with pytest.raises(Exception):
        gpu_engine.waveglow_probe(mel, flow=11, what='cond', layer=1)
    with pytest.raises(Exception):
        gpu_engine.waveglow_probe(np.zeros((1, 200, 80), np.float32), flow=11, what='cond', layer=0)     # layer 0: direct
    with pytest.raises(Exception):
        gpu_engine.waveglow_probe(np.zeros((1, 200, 80), np.float32), flow=11, what='cond', layer=1, precision='f16')


@pytest.mark.parametrize('lengths', [(101, 37, 70), (2, 150, 3)])
def test_ragged_tails_inside_a_frame_group_change_no_bit(gpu_engine, lengths):
    """Row lengths that are no multiples of four: the last real frames of a row share their group of four with frames past its
    length.  NaN there (mel and noise) against -11 / 0 there: the same audio bit for bit, zeros past the lengths."""
    B, T = len(lengths), max(lengths) + 2
    mel = np.random.default_rng(17).uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    z = np.random.default_rng(18).standard_normal((B, T * 32, 8)).astype(np.float32)
    a, b = (mel.copy(), z.copy()), (mel.copy(), z.copy())
    for r, n in enumerate(lengths):
        a[0][r, n:], a[1][r, n * 32:] = -11.0, 0.0
        b[0][r, n:], b[1][r, n * 32:] = np.nan, np.nan
    out_a = gpu_engine.waveglow_infer(a[0], z=a[1], lengths=lengths)
    assert gpu_engine.last_waveglow_form == 'winograd'
    out_b = gpu_engine.waveglow_infer(b[0], z=b[1], lengths=lengths)
    assert np.isfinite(out_a).all() and np.array_equal(out_a, out_b)
    for r, n in enumerate(lengths):
        assert not out_a[r, n * 256:].any()
