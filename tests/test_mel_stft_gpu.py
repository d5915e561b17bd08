"""GPU parity: HIP mel-STFT vs the reference's golden fixture and the numpy oracle, then stage by stage (padded rows,
spectrum, magnitudes, linear mel: `HipEngine.mel_stft_probe`) against the float64 restatement of tests/mel_stft_cases.py."""
import ctypes
import os

import numpy as np
import pytest

import mel_stft_cases as C

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'stft_tacotron_fixture.npz')


def test_mel_stft_reference_fixture(gpu_engine):
    f = np.load(GOLD)
    mel = gpu_engine.mel_stft(f['audio'])[0]
    err = np.abs(mel[:f['mel'].shape[0]] - f['mel']).max()
    print('max err vs reference fixture', err)
    assert err <= float(f['tolerance'])          # the reference's own tolerance (2e-3)


@pytest.mark.parametrize('B,N', [(1, 1024), (2, 5000), (3, 22050)])
def test_mel_stft_matches_oracle(gpu_engine, B, N):
    from oracle import mel_stft_ref
    from text_to_speech_amd.config import MelSTFTConfig
    audio = np.random.default_rng(N).uniform(-1, 1, (B, N)).astype(np.float32)
    ref = mel_stft_ref.mel_spectrogram(audio, MelSTFTConfig())
    out = gpu_engine.mel_stft(audio)
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() <= 1e-3


# ---- stage by stage against float64 (tests/mel_stft_cases.py) ------------------------------------------------------------
_RUNS = {}


def _run(eng, name):
    """{'padded', 'spectrum', 'magnitude', 'mel_linear', 'mel', 'mel_before'} of a case on the session's engine, once."""
    if name not in _RUNS:
        audio = C.audio_of(C.BY_NAME[name])
        out = {'mel_before': eng.mel_stft(audio)}
        out.update({s: eng.mel_stft_probe(audio, what=s) for s in C.STAGES})
        out['mel'] = eng.mel_stft(audio)
        _RUNS[name] = out
    return _RUNS[name]


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize('name', C.NAMES)
def test_stages_match_float64(gpu_engine, name):
    """Every probed stage of every case against the float64 restatement, as stage_error (per frame, relative to the frame's
    largest magnitude); the padded rows bit-equal to numpy's reflect pad; the probes leave the next call unchanged."""
    case, ref, got = C.BY_NAME[name], C.reference(name), _run(gpu_engine, name)
    pad = np.pad(C.audio_of(case), [(0, 0), (C.FL // 2, C.FL // 2)], mode='reflect')
    assert _bits(got['padded'], pad)
    errs = {s: C.stage_error(s, got[s], ref) for s in C.STAGES}
    print(name, 'stage_error', ' '.join(f'{s} {errs[s]:.3e}' for s in C.STAGES))
    for s in C.STAGES:
        assert got[s].shape == ref[s].shape and got[s].dtype == np.float32
        assert errs[s] <= C.BOUNDS[s], (name, s, errs[s])
    assert got['mel'].shape == (case.B, case.F, C.NMEL) and _bits(got['mel'], got['mel_before'])


@pytest.mark.parametrize('name', C.NAMES)
def test_log_and_clip(gpu_engine, name):
    """The last launch on its own: mel = log(max(mel_linear, 1e-5)) of the probed linear mel within 2 float32 ulps in every
    cell, log(1e-5) wherever the float64 reference lies below half the clip, silence included, and nothing non-finite.
    Cells between 0.5e-5 and 2e-5 may fall on either side of the clip; test_stages_match_float64 judges them, as every
    other cell, in the linear domain."""
    ref, got = C.reference(name), _run(gpu_engine, name)
    assert np.isfinite(got['mel']).all()
    ulps = C.log_ulp_error(got['mel'], got['mel_linear'])
    below = float((ref['mel_linear'] < 0.5 * C.CLIP).mean())
    print(name, f'log {ulps:.2f} ulps; {below:.0%} of the cells below half the clip')
    assert ulps <= C.LOG_ULPS
    assert C.clip_failures(got['mel'], ref) == []
    if C.BY_NAME[name].signal == 'zeros':
        floor = np.float32(np.log(np.float64(np.float32(C.CLIP))))
        assert (np.abs(got['mel'] - floor) <= C.LOG_ULPS * np.spacing(np.abs(floor))).all()
        assert not got['mel_linear'].any() and not got['spectrum'].any()


@pytest.mark.parametrize('name', C.BATCHED)
def test_rows_do_not_touch_each_other(gpu_engine, name):
    """A row of a batch is bit-equal to its own B = 1 call at every stage (the k order of a GEMM output does not depend on
    its row, and the padded rows only share a workspace), and stays so when every other row is NaN: nothing reads across
    the 1 - 3 floats between one padded row's tail and the next one's head, or across a tile that holds two rows' frames."""
    case, got = C.BY_NAME[name], _run(gpu_engine, name)
    audio = C.audio_of(case)
    for b in range(case.B):
        alone = {s: gpu_engine.mel_stft_probe(audio[b:b + 1], what=s) for s in C.STAGES}
        alone['mel'] = gpu_engine.mel_stft(audio[b:b + 1])
        poisoned = np.full_like(audio, np.nan)
        poisoned[b] = audio[b]
        among_nan = {s: gpu_engine.mel_stft_probe(poisoned, what=s) for s in C.STAGES}
        among_nan['mel'] = gpu_engine.mel_stft(poisoned)
        for s in C.STAGES + ('mel',):
            assert _bits(got[s][b:b + 1], alone[s]), (name, b, s, 'batched row differs from its own call')
            assert _bits(among_nan[s][b], got[s][b]), (name, b, s, 'row changed by NaN neighbours')
            if s != 'mel':                               # (fmaxf drops a NaN: the poisoned rows' mel is log(1e-5))
                assert np.isnan(np.delete(among_nan[s], b, axis=0)).all(), (name, b, s, 'the poison did not arrive')


def test_workspace_growth_and_reuse():
    """A fresh engine (small workspace): the smallest call, a large one (frames and mag grow), the smallest again in the
    grown workspace (padding of the large call behind its rows), the large one again -- equal bits every time."""
    from text_to_speech_amd.engine import HipEngine
    small, large = C.audio_of(C.BY_NAME['noise_b1_n1024']), C.audio_of(C.BY_NAME['impulse_b3_n16384'])
    eng = HipEngine(0)
    try:
        eng.finalize()                                   # no weights: only the mel-STFT becomes ready
        def all_of(a):
            out = {s: eng.mel_stft_probe(a, what=s) for s in C.STAGES}
            out['mel'] = eng.mel_stft(a)
            return out
        first_large = {'mel': eng.mel_stft(large)}       # grows everything from nothing
        runs = [all_of(small), all_of(large), all_of(small), all_of(large)]
    finally:
        eng.close()
    assert _bits(first_large['mel'], runs[1]['mel'])
    for s in C.STAGES + ('mel',):
        assert _bits(runs[0][s], runs[2][s]) and _bits(runs[1][s], runs[3][s]), s
    for s in C.STAGES[1:]:
        assert C.stage_error(s, runs[3][s], C.reference('impulse_b3_n16384')) <= C.BOUNDS[s]
        assert C.stage_error(s, runs[2][s], C.reference('noise_b1_n1024')) <= C.BOUNDS[s]


def test_workspace_large_small_large(gpu_engine):
    """On the session's engine: a large call, the smallest, the large one again -- the first and third bit-equal."""
    small, large = C.audio_of(C.BY_NAME['noise_b1_n1024']), C.audio_of(C.BY_NAME['noise_b5_n3333'])
    a = gpu_engine.mel_stft(large)
    a_lin = gpu_engine.mel_stft_probe(large, what='mel_linear')
    mid = gpu_engine.mel_stft(small)
    b = gpu_engine.mel_stft(large)
    b_lin = gpu_engine.mel_stft_probe(large, what='mel_linear')
    assert _bits(a, b) and _bits(a_lin, b_lin) and _bits(mid, _run(gpu_engine, 'noise_b1_n1024')['mel'])


@pytest.mark.parametrize('name', ['noise_b1_n1024', 'noise_b1_n16127', 'noise_b3_n1025'])
def test_host_device_and_stream_paths_agree(gpu_engine, name):
    import torch
    audio = C.audio_of(C.BY_NAME[name])
    host = _run(gpu_engine, name)['mel']
    dev_in = torch.from_numpy(audio).cuda()
    dev = gpu_engine.mel_stft(dev_in)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        streamed = gpu_engine.mel_stft(dev_in, stream=s)
    s.synchronize()
    assert _bits(dev.cpu().numpy(), host) and _bits(streamed.cpu().numpy(), host)
    # the probe on device memory (C ABI only): the same bits as through host memory
    B, N = audio.shape
    lin = torch.full((B, N // 256 + 1, 80), float('nan'), device='cuda')
    torch.cuda.synchronize()
    rc = gpu_engine._lib.tts_hip_mel_stft_probe(gpu_engine._h, ctypes.c_void_p(dev_in.data_ptr()), B, N, 3,
                                                ctypes.c_void_p(lin.data_ptr()), 1)
    assert rc == 0 and _bits(lin.cpu().numpy(), _run(gpu_engine, name)['mel_linear'])


@pytest.mark.parametrize('n', [1, 700, 1023])
def test_short_audio_is_zero_padded_on_both_paths(gpu_engine, n):
    """MelSTFT.__call__ pads audio shorter than one window with zeros to 1024 samples; host and device path alike."""
    import torch
    audio = np.random.default_rng(n).uniform(-1, 1, (2, n)).astype(np.float32)
    padded = np.pad(audio, [(0, 0), (0, 1024 - n)])
    want = gpu_engine.mel_stft(padded)
    assert want.shape == (2, 5, 80)
    assert _bits(gpu_engine.mel_stft(audio), want)
    dev_in = torch.from_numpy(audio).cuda()
    assert _bits(gpu_engine.mel_stft(dev_in).cpu().numpy(), want)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        streamed = gpu_engine.mel_stft(dev_in, stream=s)
    s.synchronize()
    assert _bits(streamed.cpu().numpy(), want)
    assert C.stage_error('mel_linear', gpu_engine.mel_stft_probe(padded, what='mel_linear'), C.stages(padded)) <= C.BOUNDS['mel_linear']


def test_refusals_write_nothing_and_leave_the_engine_usable(gpu_engine):
    """N = 1023, B = 0, NULL pointers, a bad `what` and a bad `mem` are TTS_HIP_EINVAL through the probe and both entry
    points, before anything is launched or copied: `out` keeps its bytes and the next call computes what it did before."""
    from text_to_speech_amd import HipLibraryError
    lib, h = gpu_engine._lib, gpu_engine._h
    EINVAL = -1
    audio = np.random.default_rng(5).uniform(-1, 1, (2, 2048)).astype(np.float32)
    before = gpu_engine.mel_stft(audio)
    out = np.full(2 * 3072, 12345.0, np.float32)                    # room for every stage's answer to a 1 x 1023 call, and more
    a, o = audio.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    probe, sync, asyn = lib.tts_hip_mel_stft_probe, lib.tts_hip_mel_stft, lib.tts_hip_mel_stft_async
    for what in range(4):
        assert probe(h, a, 1, 1023, what, o, 0) == EINVAL
        assert probe(h, a, 0, 2048, what, o, 0) == EINVAL
        assert probe(h, a, -1, 2048, what, o, 0) == EINVAL
        assert probe(h, None, 1, 2048, what, o, 0) == EINVAL
        assert probe(h, a, 1, 2048, what, None, 0) == EINVAL
        assert probe(h, a, 1, 2048, what, o, 2) == EINVAL and probe(h, a, 1, 2048, what, o, -1) == EINVAL
        assert b'mel_stft_probe' in lib.tts_hip_last_error(h)
    for what in (-1, 4, 1 << 20):
        assert probe(h, a, 1, 2048, what, o, 0) == EINVAL and probe(h, a, 1, 2048, what, o, 1) == EINVAL
    assert probe(None, a, 1, 2048, 0, o, 0) == EINVAL
    for bad in ((a, 1, 1023, o), (a, 0, 2048, o), (None, 1, 2048, o), (a, 1, 2048, None)):
        assert sync(h, *bad, 0) == EINVAL and sync(h, *bad, 1) == EINVAL
        assert asyn(h, *bad, None) == EINVAL
    assert sync(h, a, 1, 2048, o, 2) == EINVAL
    assert (out == 12345.0).all()
    with pytest.raises(ValueError):
        gpu_engine.mel_stft_probe(audio, what='phase')
    with pytest.raises(HipLibraryError, match='bad argument'):
        gpu_engine.mel_stft_probe(audio[:, :1000])
    assert _bits(gpu_engine.mel_stft(audio), before)
    lin = gpu_engine.mel_stft_probe(audio, what='mel_linear')
    assert C.stage_error('mel_linear', lin, C.stages(audio)) <= C.BOUNDS['mel_linear']
