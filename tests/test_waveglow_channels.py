"""CPU: the WaveGlow WN width (n_channels) is 256 or 512 -- the model-directory gate, the importers that take the width from
the tensors, and the C ABI's `tts_hip_waveglow_channels` (the engine itself: tests/test_waveglow_channels_gpu.py)."""
import json
import os

import numpy as np
import pytest

from test_pretrained_dir import make_dir
from text_to_speech_amd import pretrained, weights, weights_import
from text_to_speech_amd.config import WaveGlowConfig


def test_hparams_gate_accepts_256_and_512_and_names_other_widths():
    pretrained.check_hparams('waveglow', {'n_channels': 256})
    pretrained.check_hparams('waveglow', {'n_channels': 512})
    pretrained.check_hparams('waveglow', WaveGlowConfig(n_channels=256).to_dict())
    with pytest.raises(ValueError, match=r'n_channels = 384 \(supported: 256 or 512\)'):
        pretrained.check_hparams('waveglow', {'n_channels': 384})
    # everything else of the architecture stays required
    with pytest.raises(ValueError, match='n_layers = 4'):
        pretrained.check_hparams('waveglow', {'n_channels': 256, 'n_layers': 4})
    with pytest.raises(ValueError, match='n_flows = 6'):
        pretrained.check_hparams('waveglow', {'n_flows': 6})


def test_model_directory_reports_its_width(tmp_path):
    d = make_dir(tmp_path, 'WaveGlow', 'keras_waveglow_attrs.weights.h5')
    hp = {'model': {'class_name': 'WaveGlow', 'config': WaveGlowConfig(n_channels=256).to_dict()}}
    (d / 'saving' / 'config_models.json').write_text(json.dumps(hp))
    info = pretrained.read_model_dir(str(d))
    assert info['model'] == 'waveglow' and info['hparams']['n_channels'] == 256
    hp['model']['config']['n_channels'] = 384
    (d / 'saving' / 'config_models.json').write_text(json.dumps(hp))
    with pytest.raises(ValueError, match='n_channels = 384'):
        pretrained.read_model_dir(str(d))


@pytest.fixture(scope='module')
def w256():
    return weights.synth_waveglow(WaveGlowConfig(n_channels=256), seed=1234)


def _assert_round_trip(back, w):
    # the importer's round-trip bound (tests/test_weights_import.py: weight norm g * v / ||v|| in float32)
    assert list(back) == list(w)
    for k in w:
        np.testing.assert_allclose(back[k], w[k], atol=2e-6, err_msg=k)


def test_nvidia_state_dict_imports_without_a_width(w256, wg_weights, wg_cfg):
    cfg256 = WaveGlowConfig(n_channels=256)
    sd = weights_import.to_nvidia_waveglow(w256, cfg256, fused_cond=True, weight_norm=True)
    assert sd['WN.0.start.weight_v'].shape == (256, 4, 1) and sd['WN.0.cond_layer.bias'].shape == (8 * 512,)
    back = weights_import.from_nvidia_waveglow(sd)
    assert back['waveglow/block-0/start_conv/kernel'].shape == (1, 4, 256)
    _assert_round_trip(back, w256)
    # 512: unchanged, with and without the config
    sd = weights_import.to_nvidia_waveglow(wg_weights, wg_cfg, fused_cond=True, weight_norm=True)
    back = weights_import.from_nvidia_waveglow(sd)
    _assert_round_trip(back, wg_weights)
    with_cfg = weights_import.from_nvidia_waveglow(sd, wg_cfg)
    assert all(np.array_equal(back[k], with_cfg[k]) for k in back)


def test_a_384_wide_state_dict_is_refused_by_name():
    cfg = WaveGlowConfig(n_channels=384)
    w = weights.synth_waveglow(cfg, seed=5)
    with pytest.raises(ValueError, match='n_channels = 384'):
        weights_import.from_nvidia_waveglow(weights_import.to_nvidia_waveglow(w, cfg))
    named = {'wave_glow/' + k[len('waveglow/'):]: v for k, v in w.items()}
    with pytest.raises(ValueError, match='n_channels = 384'):
        weights_import.from_keras_variables(named, 'waveglow')


def test_keras_variables_import_without_a_width(w256):
    named = {'wave_glow/' + k[len('waveglow/'):]: v for k, v in w256.items()}
    back = weights_import.from_keras_variables(named, 'waveglow')
    assert list(back) == list(w256) and all(np.array_equal(back[k], w256[k]) for k in w256)


def test_keras_h5_without_a_width_refuses_the_tiny_fixture(tmp_path):
    """The H5 route reads the width off the start conv's dataset: the 8-channel fixture is named and refused, and still
    imports with its own config."""
    from test_hdf5_reader import H5
    from test_keras_h5 import TINY
    path = os.path.join(H5, 'keras_waveglow_attrs.weights.h5')
    with pytest.raises(ValueError, match=r'n_channels = 8 \(supported: 256 or 512\)'):
        weights_import.from_keras_h5(path, 'waveglow')
    assert list(weights_import.from_keras_h5(path, 'waveglow', TINY['waveglow'])) == list(weights.waveglow_manifest(TINY['waveglow']))


def test_library_exports_waveglow_channels():
    from text_to_speech_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load_library()
    assert hasattr(lib, 'tts_hip_waveglow_channels')
    assert lib.tts_hip_waveglow_channels(None) == 0
    assert lib.tts_hip_abi_version() == 13
