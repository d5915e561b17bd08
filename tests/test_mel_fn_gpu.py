"""GPU: the mel plans (csrc/mel_stft.hip: any TacotronSTFT configuration and WhisperSTFT) stage by stage against the float64
restatement of tests/mel_fn_cases.py, the default plan against the fixed call, the reference's WhisperSTFT fixture through
load_mel, and the memory kinds / streams / several plans on one engine."""
import os

import numpy as np
import pytest

import mel_fn_cases as M
import mel_stft_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
GEMM_STAGES = ('spectrum', 'magnitude', 'mel_linear')
_RUNS = {}


def _plan(eng, config):
    cfg = M.CONFIGS[config]
    return eng.mel_fn(cfg.plan_config(), window=None if cfg.periodic else cfg.window())


def _all_of(eng, config, audio, lengths):
    plan = _plan(eng, config)
    out = {s: eng.mel_fn_probe(plan, audio, s, lengths=lengths) for s in M.STAGES}
    out['mel'] = eng.mel_fn_run(plan, audio, lengths=lengths)
    return out


def _run(eng, name):
    """Every probed stage and the result of a case (NaN behind the rows' lengths) on the session's engine, once."""
    if name not in _RUNS:
        case = M.BY_NAME[name]
        _RUNS[name] = _all_of(eng, case.config, M.audio_of(case), case.lengths)
    return _RUNS[name]


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 6. stage by stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', M.NAMES)
def test_stages(gpu_engine, name):
    case, ref, got = M.BY_NAME[name], M.reference(name), _run(gpu_engine, name)
    cfg = M.CONFIGS[case.config]
    audio, lens = M.audio_of(case), case.lengths or (case.N,)
    frames = ref['frames']
    dft = [f + (cfg.kind == 'whisper') for f in frames]
    for s in M.STAGES + ('mel',):
        assert got[s].dtype == np.float32 and got[s].shape == ref[s].shape, (s, got[s].shape, ref[s].shape)
        assert np.isfinite(got[s]).all(), (s, 'NaN or inf')
    assert frames == [gpu_engine.mel_fn_frames(_plan(gpu_engine, case.config), n) for n in lens]
    # steps 1 - 3 bit-equal to numpy in float32, zeros behind every row's extent
    assert _bits(got['padded'], M.padded_rows(case.config, audio, case.lengths, np.float32))
    # the GEMM stages against float64 on the audio
    errs = {s: M.stage_error(s, got[s], ref, dft) for s in GEMM_STAGES}
    print(name, 'stage_error', ' '.join(f'{s} {errs[s]:.3e}' for s in GEMM_STAGES))
    for s in GEMM_STAGES:
        bound = M.BOUNDS[case.config][s]
        assert bound is not None and errs[s] <= bound, (name, s, errs[s], bound)
    worst_log, worst_final = 0.0, 0.0
    for b, f in enumerate(frames):
        # the logarithm against float64 of the run's own linear mel; the final stage against numpy on the run's own mel_log
        worst_log = max(worst_log, M.log_ulp_error(cfg, got['mel_log'][b, :f], got['mel_linear'][b, :f]))
        worst_final = max(worst_final, M.final_error(cfg, got['mel'][b, :f], M.final_of(cfg, got['mel_log'][b, :f])))
        assert not got['mel_log'][b, f:].any() and not got['mel'][b, f:].any(), (name, b, 'frames beyond the row hold something')
    print(name, f'log {worst_log:.2f} ulps, final {worst_final:.3g} (bound {M.final_bound(cfg)})')
    assert worst_log <= M.LOG_ULPS
    assert worst_final <= M.final_bound(cfg)
    silent = [b for b in range(case.B) if (M.MIXED[b % 3] if case.signal == 'mixed' else case.signal) == 'zeros']
    if cfg.normalize_mode is not None:
        for b in silent:
            assert not got['mel'][b].any(), (name, b, 'a silent row is not all zeros')


@pytest.mark.parametrize('name', M.RAGGED)
def test_ragged_rows_equal_their_own_calls_and_ignore_the_tails(gpu_engine, name):
    case, got = M.BY_NAME[name], _run(gpu_engine, name)
    cfg = M.CONFIGS[case.config]
    audio = M.audio_of(case)
    for b, L in enumerate(case.lengths):
        alone = _all_of(gpu_engine, case.config, audio[b:b + 1, :L], None)
        f = alone['mel'].shape[1]
        w = alone['padded'].shape[1]
        assert _bits(got['padded'][b:b + 1, :w], alone['padded']) and not got['padded'][b, w:].any()
        for s in GEMM_STAGES:
            fd = alone[s].shape[1]
            assert _bits(got[s][b:b + 1, :fd], alone[s]), (name, b, s)
        for s in ('mel_log', 'mel'):
            assert _bits(got[s][b:b + 1, :f], alone[s]), (name, b, s)
    other = _all_of(gpu_engine, case.config, M.audio_of(case, tail=7.0), case.lengths)
    for s in M.STAGES + ('mel',):
        assert _bits(got[s], other[s]), (name, s, 'the result depends on what lies behind a row')


# ---- 7. the default plan against the fixed call -----------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1024, 1027, 16128])
def test_default_plan_is_the_fixed_call(gpu_engine, N):
    audio = C.audio_of(C.Case('x', 2, N, 'noise'))
    plan = _plan(gpu_engine, 'default')
    assert _bits(gpu_engine.mel_fn_run(plan, audio), gpu_engine.mel_stft(audio))
    for s in C.STAGES:
        assert _bits(gpu_engine.mel_fn_probe(plan, audio, s), gpu_engine.mel_stft_probe(audio, what=s)), s


def test_default_plan_pads_short_audio_as_python_did(gpu_engine):
    audio = C.audio_of(C.Case('x', 1, 1024, 'noise'))[:, :500]
    assert gpu_engine.mel_fn_frames(_plan(gpu_engine, 'default'), 500) == 5
    assert _bits(gpu_engine.mel_fn_run(_plan(gpu_engine, 'default'), audio), gpu_engine.mel_stft(audio))


# ---- 8. the reference's fixture on the device ----------------------------------------------------------------------------
def test_whisper_fixture_through_load_mel(gpu_engine):
    from text_to_speech_amd.audio import load_mel
    from text_to_speech_amd.stft import WhisperSTFT
    want = np.load(os.path.join(GOLDEN, 'stft_whisper_fixture.npy'))
    mel = load_mel(os.path.join(GOLDEN, 'audio_test_16k.wav'), stft_fn=WhisperSTFT(engine=gpu_engine), engine=gpu_engine)
    assert mel.shape == want.shape
    err = float(np.abs(mel - want).max())
    print('max abs difference to the reference fixture', err)
    assert err <= 2e-3


# ---- 9. memory kinds, streams, several plans -----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['whisper_ragged', 'gather_ragged', 'centred_noise_n10080'])
def test_host_device_and_stream_paths_agree(gpu_engine, name):
    import torch
    case, host = M.BY_NAME[name], _run(gpu_engine, name)['mel']
    plan = _plan(gpu_engine, case.config)
    dev_in = torch.from_numpy(M.audio_of(case)).cuda()
    dev = gpu_engine.mel_fn_run(plan, dev_in, lengths=case.lengths)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        streamed = gpu_engine.mel_fn_run(plan, dev_in, lengths=case.lengths, stream=s)
    s.synchronize()
    assert dev.is_cuda and _bits(dev.cpu().numpy(), host) and _bits(streamed.cpu().numpy(), host)


def test_two_plans_on_one_engine_do_not_disturb_each_other(gpu_engine):
    a, b = M.BY_NAME['wide_noise_n18900'], M.BY_NAME['whisper_noise_n401']
    pa, pb = _plan(gpu_engine, a.config), _plan(gpu_engine, b.config)
    assert pa is not pb and pa is _plan(gpu_engine, a.config)
    xa, xb = M.audio_of(a), M.audio_of(b)
    first = gpu_engine.mel_fn_run(pa, xa), gpu_engine.mel_fn_run(pb, xb)
    again = gpu_engine.mel_fn_run(pa, xa), gpu_engine.mel_stft(C.audio_of(C.BY_NAME['noise_b1_n1024'])), gpu_engine.mel_fn_run(pb, xb)
    assert _bits(first[0], again[0]) and _bits(first[1], again[2])
    assert _bits(first[0], _run(gpu_engine, a.name)['mel']) and _bits(first[1], _run(gpu_engine, b.name)['mel'])


def test_refusals_launch_nothing(gpu_engine):
    from text_to_speech_amd import HipLibraryError
    plan = _plan(gpu_engine, 'whisper')
    with pytest.raises(HipLibraryError, match='mel_fn_create: filter_length = 5000 outside'):
        gpu_engine.mel_fn(dict(M.CONFIGS['default'].plan_config(), filter_length=5000))
    with pytest.raises(ValueError):
        gpu_engine.mel_fn_run(plan, np.zeros((2, 100), np.float32), lengths=[100, 0])
    before = gpu_engine.mel_fn_run(plan, M.audio_of(M.BY_NAME['whisper_noise_n400']))
    assert _bits(before, _run(gpu_engine, 'whisper_noise_n400')['mel'])
