"""CPU: the mel plans' yardstick and their Python classes.  The float64 restatement of tests/mel_fn_cases.py is pinned to
the reference (its WhisperSTFT fixture, and the oracle's TacotronSTFT for the default configuration); the classes of
text_to_speech_amd.stft keep the reference's constructor arguments, defaults and get_config keys; and the bounds the GPU
tests hold the kernels to are shown to catch the errors a wrong kernel would make."""
import json
import os

import numpy as np
import pytest

import mel_fn_cases as M

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


# ---- 1. pinning ------------------------------------------------------------------------------------------------------------
def test_whisper_restatement_reproduces_the_reference_fixture():
    """audio_test_16k.wav -> normalize_audio(max_val=1.) -> config `whisper` in float64 against the reference's own
    stft-WhisperSTFT.npy, at the reference's tolerance (test_utils_audio.py:110)."""
    from text_to_speech_amd.audio import normalize_audio, read_wav
    rate, wav = read_wav(os.path.join(GOLDEN, 'audio_test_16k.wav'))
    assert rate == 16000
    want = np.load(os.path.join(GOLDEN, 'stft_whisper_fixture.npy'))
    got = M.stages('whisper', normalize_audio(wav, max_val=1.)[None])['mel'][0]
    assert got.shape == want.shape == (405, 80)
    err = float(np.abs(got - want).max())
    print('max abs difference to the reference fixture', err)
    assert err <= 2e-3


def test_default_restatement_is_the_oracle():
    from oracle import mel_stft_ref
    from text_to_speech_amd.config import MelSTFTConfig
    audio = np.load(os.path.join(GOLDEN, 'stft_tacotron_fixture.npz'))['audio'][None]
    want = mel_stft_ref.mel_spectrogram(audio, MelSTFTConfig(), dtype=np.float64)
    got = M.stages('default', audio)
    assert got['mel_log'].shape == want.shape
    assert np.abs(got['mel_log'] - want).max() <= 1e-12
    assert np.array_equal(got['mel'], got['mel_log'].astype(np.float32))


def test_case_table_covers_what_it_claims():
    for cfg in M.CONFIGS.values():
        lens = M.lengths_of(cfg)
        assert {1, cfg.win_length - 1, cfg.win_length, cfg.win_length + 1} <= set(lens)
        assert {n % 4 for n in lens} >= {1, 3}
        want = (63, 63, 64) if cfg.filter_length % 2 else (63, 64, 65)
        assert tuple(cfg.dft_frames(cfg.hop_length * k + d) for k, d in ((63, -1), (63, 0), (64, 0))) == want
        ragged = M.BY_NAME[f'{cfg.name}_ragged']
        assert ragged.B == 3 and ragged.lengths[1] == cfg.win_length - 1 and max(ragged.lengths) < ragged.N
        assert np.isnan(M.audio_of(ragged)[0, ragged.lengths[0]:]).all()
    assert M.CONFIGS['gather'].hop_length % 4 and M.CONFIGS['whisper'].filter_length % 32 and M.CONFIGS['odd'].filter_length % 2


# ---- 2. classes ------------------------------------------------------------------------------------------------------------
MEL_KEYS = {'class_name', 'n_mel_channels', 'sampling_rate', 'win_length', 'hop_length', 'filter_length', 'mel_fmin', 'mel_fmax',
            'pre_emph', 'normalize_mode'}
STFT_KEYS = {'filter_length', 'hop_length', 'win_length', 'window', 'to_magnitude', 'periodic'}


def test_get_config_keys_and_defaults():
    from text_to_speech_amd.stft import MelSTFT, TacotronSTFT, WhisperSTFT
    assert set(MelSTFT(22050).get_config()) == MEL_KEYS
    t, w = TacotronSTFT().get_config(), WhisperSTFT().get_config()
    assert set(t) == set(w) == MEL_KEYS | STFT_KEYS
    assert t == {'class_name': 'TacotronSTFT', 'n_mel_channels': 80, 'sampling_rate': 22050, 'win_length': 1024, 'hop_length': 256,
                 'filter_length': 1024, 'mel_fmin': 0.0, 'mel_fmax': 8000.0, 'pre_emph': 0., 'normalize_mode': None,
                 'window': 'hann', 'to_magnitude': True, 'periodic': True}
    assert (w['class_name'], w['sampling_rate'], w['win_length'], w['hop_length'], w['filter_length']) == \
        ('WhisperSTFT', 16000, 400, 160, 400)
    assert TacotronSTFT().rate == 22050 and WhisperSTFT().rate == 16000
    with pytest.raises(ValueError):
        TacotronSTFT(normalize_mode='per_batch')


def test_save_load_round_trip_and_create(tmp_path):
    from text_to_speech_amd.stft import MelSTFT, TacotronSTFT, WhisperSTFT
    obj = TacotronSTFT(16000, 40, win_length=400, hop_length=160, filter_length=512, pre_emph=0.97, normalize_mode='per_feature',
                       window='hamming', periodic=False)
    path = obj.save(str(tmp_path / 'mel_fn'))
    assert path.endswith('mel_fn.json') and set(json.load(open(path))) == MEL_KEYS | STFT_KEYS
    back = MelSTFT.load_from_file(path)
    assert type(back) is TacotronSTFT and back.get_config() == obj.get_config()
    assert type(MelSTFT.create('WhisperSTFT')) is WhisperSTFT
    assert MelSTFT.create('TacotronSTFT', 24000, 128, mel_fmax=12000.0).get_config()['n_mel_channels'] == 128
    # a mel_fn.json as the reference writes it (stft.py:150-166, 276-284, 316-319)
    ref = {'class_name': 'WhisperSTFT', 'n_mel_channels': 80, 'sampling_rate': 16000, 'win_length': 400, 'hop_length': 160,
           'filter_length': 400, 'mel_fmin': 0.0, 'mel_fmax': 8000.0, 'pre_emph': 0.0, 'normalize_mode': None, 'window': 'hann',
           'to_magnitude': True, 'periodic': True}
    p = tmp_path / 'ref_mel_fn.json'
    p.write_text(json.dumps(ref, indent=4))
    made = MelSTFT.create(str(p))
    assert type(made) is WhisperSTFT and made.get_config() == ref
    with pytest.raises(ValueError, match='Unknown Mel STFT class'):
        MelSTFT.create('JasperSTFT')


def test_lengths_in_seconds_and_frame_arithmetic():
    from text_to_speech_amd.stft import TacotronSTFT
    s = TacotronSTFT(16000, win_length=0.025, hop_length=0.01, filter_length=512)
    assert (s.win_length, s.hop_length, s.filter_length) == (400, 160, 512)
    assert TacotronSTFT(16000, win_length=1., hop_length=0.5, filter_length=1.).hop_length == 8000
    assert s.get_mel_length(16000) == 100 and s.get_mel_length(10) == 4 and s.get_audio_length(7) == 1120
    assert TacotronSTFT().get_mel_length(22050) == 87


def test_a_call_needs_an_engine():
    from text_to_speech_amd.stft import MelSTFT, WhisperSTFT
    with pytest.raises(RuntimeError, match='no engine'):
        WhisperSTFT()(np.zeros(1600, np.float32))
    with pytest.raises(NotImplementedError):
        MelSTFT(22050).bind(object())(np.zeros(1600, np.float32))


def test_fft_window():
    from scipy.signal import get_window
    from text_to_speech_amd.stft import TacotronSTFT
    assert TacotronSTFT().fft_window() is None                      # the engine's own periodic Hann
    w = TacotronSTFT(8000, 23, win_length=255, hop_length=64, filter_length=255, periodic=False).fft_window()
    assert np.array_equal(w, get_window('hann', 255, fftbins=False))
    assert np.abs(w - M.CONFIGS['odd'].window()).max() <= 1e-15


def test_load_mel_passes_a_mel_through():
    from text_to_speech_amd.audio import load_mel
    from text_to_speech_amd.stft import WhisperSTFT
    mel = np.zeros((7, 80), np.float32)
    assert load_mel(mel, engine=None, stft_fn=WhisperSTFT()) is mel
    assert load_mel({'mel': mel}, engine=None, stft_fn=WhisperSTFT()) is mel
    with pytest.raises(ValueError, match='22050'):                  # without stft_fn: as before
        load_mel(np.zeros(100, np.float32), 16000, engine=None)


# ---- 4. the bounds catch errors -------------------------------------------------------------------------------------------
def _planted(mutation, names):
    """The largest error a planted mutation makes at the stage it belongs to, over `names`, and the largest bound there."""
    stage, kw = M.MUTATIONS[mutation]
    worst, bound = 0.0, 0.0
    for name in names:
        case, ref = M.BY_NAME[name], M.reference(name)
        cfg = M.CONFIGS[case.config]
        bad = M.stages(case.config, M.audio_of(case, tail=0.0), case.lengths, **kw)
        if stage == 'mel':
            err, b = max(M.final_error(cfg, bad['mel'][r:r + 1, :f], ref['mel'][r:r + 1, :f]) if bad['mel'].shape == ref['mel'].shape
                         else float('inf') for r, f in enumerate(ref['frames'])), M.final_bound(cfg)
        else:
            dft = [f + (cfg.kind == 'whisper') for f in ref['frames']]
            err, b = M.stage_error(stage, bad[stage], ref, dft), M.BOUNDS[case.config][stage]
        worst, bound = max(worst, err), max(bound, b)
    return worst, bound


@pytest.mark.parametrize('mutation,names', [
    ('window_swapped', [f'{c}_noise_n{M.CONFIGS[c].hop_length * 63}' for c in M.CONFIGS]),
    ('lpad_off_by_one', ['centred_noise_n10080', 'wide_noise_n18900']),
    ('pre_emph_before_pad', ['centred_noise_n399', 'centred_noise_n1']),
    ('whisper_last_frame_kept', ['whisper_noise_n10080']),
    ('sample_std', ['centred_noise_n10080', 'gather_noise_n17325', 'centred_ragged', 'gather_ragged']),
    ('rowmax_over_batch', ['whisper_ragged']),
])
def test_bounds_catch_planted_errors(mutation, names):
    """Each planted error, computed in numpy, exceeds the bound of the stage it belongs to -- on every case listed, by 3x."""
    for name in names:
        assert name in M.BY_NAME, name
        err, bound = _planted(mutation, [name])
        print(mutation, name, f'planted {err:.3e}, bound {bound:.3e}')
        assert bound is not None and err > 3 * bound and err > 0, (mutation, name, err, bound)


def test_every_bound_lies_below_every_planted_spectrum_error():
    weakest = min(_planted(m, [n])[0] for m, names in (
        ('window_swapped', [f'{c}_noise_n{M.CONFIGS[c].hop_length * 63}' for c in M.CONFIGS]),
        ('lpad_off_by_one', ['centred_noise_n10080', 'wide_noise_n18900'])) for n in names)
    for config, bounds in M.BOUNDS.items():
        for stage, b in bounds.items():
            assert b is not None and b < weakest, (config, stage, b, weakest)
