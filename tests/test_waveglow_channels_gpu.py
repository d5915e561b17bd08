"""GPU: a 256-channel WaveGlow (n_channels = 256, the width of NVIDIA's "universal" checkpoints) in every precision, every
WN GEMM tile family and every call kind, against the oracle -- beside the session's 512-channel engine in the same process.

Weights: `synth_waveglow(WaveGlowConfig(n_channels=256), seed=1234)` in an engine of this module; inputs as in
tests/test_waveglow_gpu.py.  Tolerances are the project's own: 1e-4 waveform RMS for fp32 and f16x3, F16_RMS_TOL for f16,
ACTS_REL_TOL for one layer's activations (tests/test_waveglow_gpu.py); 5e-6 / 5e-5 for a batch row against its own HIP run
(tests/test_waveglow_packed_gpu.py HIP_TOL).  The tile family of a call follows from the frame count alone (csrc/wg_plan.h).
One reference per shape, shared by the precisions (numpy oracle; the 384-frame one from oracle/torch_ref.py).
"""
import json

import numpy as np
import pytest

from conftest import rms
from test_waveglow_gpu import ACTS_REL_TOL, F16_RMS_TOL, RMS_TOL, _inputs
from test_waveglow_packed_gpu import HIP_TOL

pytestmark = pytest.mark.gpu

TOL = {'f32': RMS_TOL, 'f16': F16_RMS_TOL, 'f16x3': RMS_TOL}
# frames -> tile family (tts_hip_last_waveglow_tiles): 64-row (3), 128 x 64 (2), 128-row (1), 256-row (0)
SHAPES = {(2, 13): '64-row', (1, 100): '128x64', (1, 384): '128-row', (2, 128): '256-row'}


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


@pytest.fixture(scope='module')
def oracle256(w256, cfg256):
    """(B, T) -> (mel, z, reference waveform, intermediates or None), computed once per shape."""
    from oracle import torch_ref, waveglow_ref
    cache = {}

    def get(B, T):
        if (B, T) not in cache:
            mel, z = _inputs(B, T)
            if B * T >= 384:
                ref, inter = torch_ref.torch_waveglow(mel, w256, cfg256, z, sigma=1.0), None
            else:
                ref, inter = waveglow_ref.infer(mel, w256, cfg256, z=z, sigma=1.0, return_intermediates=True)
            ref.setflags(write=False)
            cache[B, T] = (mel, z, ref, inter)
        return cache[B, T]
    return get


def test_finalize_reports_the_width(eng256, gpu_engine):
    assert eng256.has_model('waveglow') and eng256.waveglow_channels == 256
    assert gpu_engine.waveglow_channels == 512
    from text_to_speech_amd.engine import HipEngine
    empty = HipEngine(0)
    try:
        assert empty.waveglow_channels == 0                      # no WaveGlow finalized
    finally:
        empty.close()


@pytest.mark.parametrize('prec', ['f32', 'f16'])
@pytest.mark.parametrize('B,T', list(SHAPES))
def test_256_channels_match_the_oracle_in_every_tile_family(eng256, oracle256, B, T, prec):
    mel, z, ref, _ = oracle256(B, T)
    out = eng256.waveglow_infer(mel, z=z, sigma=1.0, precision=prec)
    assert eng256.last_waveglow_tiles == SHAPES[B, T] and eng256.last_waveglow_form == 'direct'
    assert out.shape == ref.shape == (B, T * 256) and np.isfinite(out).all()
    err = rms(out - ref)
    print(f'C=256 {prec} {B} x {T} ({SHAPES[B, T]}): rms_err={err:.3e} max_err={np.abs(out - ref).max():.3e} ref_rms={rms(ref):.3f}')
    assert rms(ref) > 0.5 and err <= TOL[prec]
    if prec == 'f16':                                            # a different arithmetic, not the flag ignored
        exact = eng256.waveglow_infer(mel, z=z, sigma=1.0)
        assert rms(exact - ref) <= RMS_TOL < 1e3 * rms(out - exact)


@pytest.mark.parametrize('B,T', [(2, 13), (2, 128)])
def test_256_channels_f16x3_matches_the_oracle(eng256, oracle256, B, T):
    mel, z, ref, _ = oracle256(B, T)
    out = eng256.waveglow_infer(mel, z=z, sigma=1.0, precision='f16x3')
    assert eng256.last_waveglow_tiles == SHAPES[B, T]
    exact = eng256.waveglow_infer(mel, z=z, sigma=1.0)
    err = rms(out - ref)
    print(f'C=256 f16x3 {B} x {T}: rms_err={err:.3e} (exact fp32 path {rms(exact - ref):.3e}; x3 vs exact {rms(out - exact):.3e})')
    assert np.isfinite(out).all() and err <= RMS_TOL
    assert not np.array_equal(out, exact)


def test_one_flow_layer_by_layer(eng256, oracle256, w256, cfg256):
    """1 x 100 frames, fp32: the gated activations of flow 11's layers 0 (the composed start conv), 1 and 7 (the last one:
    no residual GEMM behind it) against the oracle's `wn_block(collect=...)`, and the flow state after flows 11, 8 and 4
    (the two early-z prepends) against `return_intermediates`."""
    from oracle import waveglow_ref
    mel, z, _, inter = oracle256(1, 100)
    acts = []
    waveglow_ref.wn_block(z[:, :, :cfg256.n_remaining_channels // 2], inter['spect'], w256, 'waveglow/block-11', cfg256.n_layers, cfg256.n_channels, collect=acts)
    for layer in (0, 1, 7):
        got = eng256.waveglow_probe(mel, z=z, flow=11, what='acts', layer=layer)
        assert got.shape == acts[layer].shape == (1, 3200, 256)
        err = rms(got - acts[layer]) / rms(acts[layer])
        print(f'C=256 flow 11 layer {layer}: acts rel. RMS error {err:.3e} (acts RMS {rms(acts[layer]):.3f})')
        assert err <= ACTS_REL_TOL
        assert np.array_equal(got, eng256.waveglow_probe_acts(mel, z=z, flow=11, layer=layer))
    for flow, width in ((11, 4), (8, 6), (4, 8)):
        want = inter[f'audio_after_flow_{flow}']
        got = eng256.waveglow_probe(mel, z=z, flow=flow, what='state')
        assert got.shape == want.shape == (1, 3200, width)
        err = rms(got - want)
        print(f'C=256 state after flow {flow}: rms_err={err:.3e} (state RMS {rms(want):.3f})')
        assert err <= RMS_TOL


def test_winograd_form_is_not_taken_at_256_channels(eng256):
    """1 x 160 frames is above the 144-frame threshold of the Winograd form, which exists for 512 channels only."""
    from text_to_speech_amd._lib import HipLibraryError
    mel, z = _inputs(1, 160, seed=15)
    try:
        eng256.set_waveglow_form('winograd')
        a = eng256.waveglow_infer(mel, z=z)
        assert eng256.last_waveglow_form == 'direct'
        with pytest.raises(HipLibraryError, match='no conditioning plane'):
            eng256.waveglow_probe(mel, z=z, flow=11, what='cond', layer=2)
        eng256.set_waveglow_form('direct')
        b = eng256.waveglow_infer(mel, z=z)
        assert eng256.last_waveglow_form == 'direct'
    finally:
        eng256.set_waveglow_form('winograd')
    assert np.isfinite(a).all() and a.any() and np.array_equal(a, b)


@pytest.mark.parametrize('prec', ['f32', 'f16', 'f16x3'])
@pytest.mark.parametrize('T,lengths', [(6, (6, 1, 5)), (40, (40, 0, 25))])
def test_unequal_rows(eng256, T, lengths, prec):
    B = len(lengths)
    mel, z = _inputs(B, T, seed=13)
    nan_mel, nan_z = mel.copy(), z.copy()
    for b, n in enumerate(lengths):
        nan_mel[b, n:] = np.nan
        nan_z[b, n * 32:] = np.nan
    tol = HIP_TOL[prec]
    ragged = eng256.waveglow_infer(mel, z=z, precision=prec, lengths=lengths)
    assert ragged.shape == (B, T * 256) and np.isfinite(ragged).all()
    assert np.array_equal(eng256.waveglow_infer(nan_mel, z=nan_z, precision=prec, lengths=lengths), ragged)
    packed = eng256.waveglow_infer(mel, z=z, precision=prec, lengths=lengths, packed=True)
    assert np.array_equal(eng256.waveglow_infer(nan_mel, z=nan_z, precision=prec, lengths=lengths, packed=True), packed)
    seeds = ([11, 12, 13], [0, 5, 9])
    seeded = eng256.waveglow_infer(nan_mel, precision=prec, lengths=lengths, row_seeds=seeds)
    for b, n in enumerate(lengths):
        assert not ragged[b, n * 256:].any() and not packed[b, n * 256:].any() and not seeded[b, n * 256:].any()
        if n == 0:
            continue
        own_mel = np.ascontiguousarray(mel[b:b + 1, :n])
        solo = eng256.waveglow_infer(own_mel, z=np.ascontiguousarray(z[b:b + 1, :n * 32]), precision=prec)[0]
        e_r, e_p = rms(ragged[b, :n * 256] - solo), rms(packed[b, :n * 256] - solo)
        solo_seeded = eng256.waveglow_infer(own_mel, precision=prec, row_seeds=([seeds[0][b]], [seeds[1][b]]))[0]
        e_s = rms(seeded[b, :n * 256] - solo_seeded)
        print(f'C=256 {prec} T={T} row {b} n={n}: vs its own run ragged {e_r:.3e} packed {e_p:.3e} seeded {e_s:.3e} (rms {rms(solo):.3f})')
        assert solo.any() and e_r <= tol and e_p <= tol and e_s <= tol
    assert rms(packed - ragged) <= tol


def test_two_widths_in_one_process(eng256, gpu_engine, oracle256, wg_weights, wg_cfg):
    from oracle import waveglow_ref
    mel, z, ref256, _ = oracle256(2, 13)
    ref512 = waveglow_ref.infer(mel, wg_weights, wg_cfg, z=z, sigma=1.0)
    for prec in ('f32', 'f16', 'f16x3'):
        a512 = gpu_engine.waveglow_infer(mel, z=z, precision=prec)
        a256 = eng256.waveglow_infer(mel, z=z, precision=prec)
        b512 = gpu_engine.waveglow_infer(mel, z=z, precision=prec)
        b256 = eng256.waveglow_infer(mel, z=z, precision=prec)
        assert np.array_equal(a512, b512) and np.array_equal(a256, b256)
        e512, e256 = rms(a512 - ref512), rms(a256 - ref256)
        print(f'{prec}: 512 rms_err={e512:.3e}  256 rms_err={e256:.3e}  (512 vs 256 outputs differ by {rms(a512 - a256):.3f})')
        assert e512 <= TOL[prec] and e256 <= TOL[prec] and rms(a512 - a256) > 0.1
    assert gpu_engine.waveglow_channels == 512 and eng256.waveglow_channels == 256


def test_model_directory_with_a_256_channel_keras_checkpoint(tmp_path, monkeypatch, cfg256):
    """A full-size 256-channel model directory (Keras `.weights.h5` written by the real HDF5 library) through
    `pretrained.load_model`: the width comes from the directory's hyper-parameters, the audio is judged by the oracle on the
    original tensors, and the `WaveGlow` wrapper vocodes on that runtime."""
    import os
    import test_pretrained_gpu as tpg
    from oracle import waveglow_ref
    from text_to_speech_amd import pretrained
    monkeypatch.setattr(tpg, 'GEN', os.path.join(os.path.dirname(tpg.GEN), 'make_h5_waveglow_channels.py'))
    d, save, tensors = tpg._write_checkpoint(tmp_path, 'pretrained_waveglow_256', '--full-waveglow', '--channels', '256')
    assert tensors['waveglow/block-0/start_conv/kernel'].shape == (1, 4, 256)
    (d / 'config.json').write_text(json.dumps({'class_name': 'WaveGlow', 'config': {'name': d.name}}))
    (save / 'config_models.json').write_text(json.dumps({'model': {'class_name': 'WaveGlow', 'config': cfg256.to_dict()}}))
    model = pretrained.load_model(str(d), reload=True)
    eng = model.compiled_infer.engine
    assert eng.waveglow_channels == 256
    rng = np.random.default_rng(2)
    mel = rng.uniform(-11.5, 1.2, (1, 6, 80)).astype(np.float32)
    z = rng.standard_normal((1, 6 * 32, 8)).astype(np.float32)
    got = eng.waveglow_infer(mel, z=z)
    err = rms(got - waveglow_ref.infer(mel, tensors, cfg256, z=z))
    print(f'imported 256-channel Keras checkpoint vs oracle: waveform RMS err {err:.2e}')
    assert err <= tpg.WAVE_RMS_TOL == 1e-4
    assert np.array_equal(model(mel, z=z), got)
    # ... and a directory that does not state its width: the importer reads it off the start conv
    os.remove(save / 'config_models.json')
    os.remove(save / 'ckpt-0000.ttsw')
    path, _ = pretrained.convert_model_dir(str(d))
    from text_to_speech_amd.weights import load_ttsw
    assert load_ttsw(path)['waveglow/block-3/in_conv-2/kernel'].shape == (3, 256, 512)


def test_other_widths_fail_finalize_by_name(w256, taco_weights):
    from text_to_speech_amd._lib import HipLibraryError
    from text_to_speech_amd.engine import HipEngine
    tok = np.random.default_rng(0).integers(1, 148, (1, 12)).astype(np.int32)
    eng = HipEngine(0)
    try:
        eng.load_state(taco_weights)
        eng.finalize()
        before = eng.tacotron2_infer(tok, max_len=6, early_stopping=False)
        bad = dict(w256)
        bad['waveglow/block-0/start_conv/kernel'] = np.zeros((1, 4, 384), np.float32)
        eng.load_state(bad)
        with pytest.raises(HipLibraryError, match=r'\(-1\).*waveglow/block-0/start_conv/kernel.*256 or 512.*384'):
            eng.finalize()
        assert not eng.has_model('waveglow') and eng.waveglow_channels == 0
        # a tensor that disagrees with the start conv's width is the same error, by its own name
        eng.set_tensor('waveglow/block-0/start_conv/kernel', w256['waveglow/block-0/start_conv/kernel'])
        eng.set_tensor('waveglow/block-0/start_conv/bias', np.zeros((512,), np.float32))
        with pytest.raises(HipLibraryError, match=r'\(-1\).*waveglow/block-0/start_conv/bias.*\[512\]'):
            eng.finalize()
        assert not eng.has_model('waveglow') and eng.waveglow_channels == 0
        with pytest.raises(HipLibraryError):
            eng.waveglow_infer(np.zeros((1, 4, 80), np.float32))
        after = eng.tacotron2_infer(tok, max_len=6, early_stopping=False)
        assert np.array_equal(before.mel, after.mel)
    finally:
        eng.close()
