"""GPU: reduce_noise stage by stage (`HipEngine.reduce_noise_probe`) against the float64 stage functions of
tests/reduce_noise_cases.py, each applied to the run's own previous stage; and the trim convolution
(`HipEngine.trim_silence_probe`) against np.convolve in float64 (tests/trim_conv_cases.py)."""
import ctypes

import numpy as np
import pytest

import audio_ref
import reduce_noise_cases as C
import trim_conv_cases as T

pytestmark = pytest.mark.gpu

_RUNS = {}
TIE_CASES = ('noise_1', 'noise_300', 'noise_511', 'noise_1_300_511_512_513', 'noise_1_511_4410_20000', 'zeros_2048',
             'zeros_300_2048_5000', 'zero_row1_3000_2500_700', 'burst_8000', 'burst_300_8000')


def _all_of(eng, inputs):
    """Every probed stage, then the ordinary call without and with renormalising."""
    audio, lens, noise, nl = inputs
    kw = dict(lengths=lens, noise=noise, noise_length=int(nl))
    out = {s: eng.reduce_noise_probe(audio, what=s, **kw) for s in C.STAGES}
    out['out'] = eng.reduce_noise(audio, **kw)
    out['out_norm'] = eng.reduce_noise(audio, renormalize=True, **kw)
    return out


def _run(eng, name):
    if name not in _RUNS:
        inputs = C.inputs_of(C.BY_NAME[name])
        audio, lens, noise, nl = inputs
        before = eng.reduce_noise(audio, lengths=lens, noise=noise, noise_length=int(nl))
        _RUNS[name] = dict(_all_of(eng, inputs), out_before=before)
    return _RUNS[name]


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('name', C.NAMES)
def test_stages_match_float64(gpu_engine, name):
    """Every stage of every case inside its bound (C.BOUNDS; `compare` says against what), the padded rows bit-equal with
    nothing of the NaN / 1e30 tails in them, every decidable mask cell equal to the float64 decision, tie cells and dead
    frames 0, at most 0.1 % of the cells undecidable, out[b, L_b:] exactly 0, silent rows exactly 0 before and after
    renormalising; and the probes leave the next ordinary call bit-equal to the one before them."""
    case, got = C.BY_NAME[name], _run(gpu_engine, name)
    inputs = C.inputs_of(case)
    for s in C.STAGES + ('out', 'out_norm'):
        assert got[s].dtype == np.float32 and np.isfinite(got[s]).all(), s
    e = C.compare(inputs, got)
    print(name, ' '.join(f'{k} {v:.3g}' for k, v in e.items()))
    assert C.failures(e) == []
    if name in TIE_CASES:
        assert e['ties'] > 0
    for b, L in enumerate(case.lengths):
        assert not got['out'][b, L:].any() and not got['out_norm'][b, L:].any()
    if case.signal == 'zeros':
        assert not got['out'].any() and not got['out_norm'].any() and not got['mask'].any() and not got['power_max'].any()
    assert _bits(got['out'], got['out_before'])


@pytest.mark.parametrize('name', C.BATCHED)
def test_rows_equal_their_own_calls(gpu_engine, name):
    """A row of a ragged batch is bit-equal to the one-row call on audio[b, :L_b] at every probed stage and in both outputs,
    over the row's own signal and noise frames (the slots past them read into the next row's samples); the padded clip over
    its whole extent."""
    case, got = C.BY_NAME[name], _run(gpu_engine, name)
    audio, lens, noise, nl = C.inputs_of(case)
    g = C.geometry(case.B, case.N, lens, noise, nl)
    for b, L in enumerate(case.lengths):
        alone = _all_of(gpu_engine, (audio[b:b + 1, :L], None, None if noise is None else noise[b:b + 1], nl))
        F, nF, w = int(g.F[b]), int(g.nF[b]), alone['padded'].shape[1]
        pairs = {
            'padded': (got['padded'][b, :w], alone['padded'][0]), 'noise_padded': (got['noise_padded'][b], alone['noise_padded'][0]),
            'spectrum': (got['spectrum'][b, :F], alone['spectrum'][0, :F]),
            'noise_spectrum': (got['noise_spectrum'][b, :nF], alone['noise_spectrum'][0, :nF]),
            'power_max': (got['power_max'][:, b], alone['power_max'][:, 0]), 'threshold': (got['threshold'][b], alone['threshold'][0]),
            'mask': (got['mask'][b, :F], alone['mask'][0, :F]), 'gated': (got['gated'][b, :F], alone['gated'][0, :F]),
            'frames': (got['frames'][b, :F], alone['frames'][0, :F]), 'out': (got['out'][b, :L], alone['out'][0]),
            'out_norm': (got['out_norm'][b, :L], alone['out_norm'][0]),
        }
        for s, (x, y) in pairs.items():
            assert _bits(x, y), (name, b, s)
        assert not got['padded'][b, w:].any()


def test_refusals_launch_nothing(gpu_engine):
    """What the real calls refuse, the probes refuse, and an unknown stage: TTS_HIP_EINVAL, `out` keeps its bytes, and the
    next call computes what it did before."""
    from text_to_speech_amd import HipLibraryError
    lib, h = gpu_engine._lib, gpu_engine._h
    inputs = C.inputs_of(C.BY_NAME['noise_1500_t500'])
    before = _all_of(gpu_engine, inputs)
    a = np.zeros((2, 4096), np.float32)
    out = np.full(2 * 14 * 2050 + 16, 12345.0, np.float32)
    conv = np.full(2 * 4097 + 16, 12345.0, np.float64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    bad_len, low_len = np.array([4097, 10], np.int32), np.array([0, 10], np.int32)
    rn, tr = lib.tts_hip_reduce_noise_probe, lib.tts_hip_trim_silence_probe
    for what in (-1, 9, 1 << 20):
        assert rn(h, p(a), 2, 4096, None, None, 100, what, p(out), 0) == -1
        assert b'reduce_noise_probe' in lib.tts_hip_last_error(h)
        assert rn(h, p(a), 2, 4096, None, None, 100, what, p(out), 1) == -1
    for what in range(9):
        assert rn(h, p(a), 2, 4096, p(bad_len), None, 100, what, p(out), 0) == -1
        assert b'lengths' in lib.tts_hip_last_error(h)
        assert rn(h, p(a), 2, 4096, p(low_len), None, 100, what, p(out), 0) == -1
        assert rn(h, p(a), 2, 4096, None, None, 0, what, p(out), 0) == -1
        assert rn(h, p(a), 2, 4096, None, None, 100, what, p(out), 7) == -1
        assert rn(h, p(a), 0, 4096, None, None, 100, what, p(out), 0) == -1
        assert rn(h, p(a), 2, 0, None, None, 100, what, p(out), 0) == -1
        assert rn(h, None, 2, 4096, None, None, 100, what, p(out), 0) == -1
        assert rn(h, p(a), 2, 4096, None, None, 100, what, None, 0) == -1
        assert rn(h, p(a), 1 << 14, 1 << 20, None, None, 100, what, p(out), 1) == -1
        assert b'31-bit' in lib.tts_hip_last_error(h)
        assert rn(None, p(a), 2, 4096, None, None, 100, what, p(out), 0) == -1
    assert tr(h, p(a), 2, 4096, None, 1, p(conv), 0) == -1
    assert b'trim_silence_probe' in lib.tts_hip_last_error(h)
    assert tr(h, p(a), 2, 4096, p(bad_len), 400, p(conv), 0) == -1
    assert tr(h, p(a), 2, 4096, None, 400, None, 0) == -1
    assert tr(h, None, 2, 4096, None, 400, p(conv), 0) == -1
    assert tr(h, p(a), 2, 4096, None, 400, p(conv), 5) == -1
    assert tr(h, p(a), 0, 4096, None, 400, p(conv), 0) == -1
    assert tr(None, p(a), 2, 4096, None, 400, p(conv), 0) == -1
    assert (out == 12345.0).all() and (conv == 12345.0).all()
    with pytest.raises(ValueError):
        gpu_engine.reduce_noise_probe(a, what='phase', noise_length=100)
    with pytest.raises(HipLibraryError, match='31-bit'):
        gpu_engine.reduce_noise_probe(np.zeros((1, 8), np.float32), what='padded', noise_length=1 << 30)
    after = _all_of(gpu_engine, inputs)
    for s in before:
        assert _bits(before[s], after[s]), s
    assert gpu_engine.trim_silence(np.ones(5000, np.float32), 16000) == (0, 5000)


# ---- trim convolution ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', T.NAMES)
def test_trim_convolution(gpu_engine, name):
    """The convolution rows against np.convolve in float64: zeros exact, everything else within (W + 2) * 2^-52 relative,
    nothing of the NaN / 1e30 tails; and the ordinary call's (start, end) are audio_ref's rule applied to these rows, in all
    three modes."""
    case = T.BY_NAME[name]
    audio, lens = T.audio_of(case)
    conv = gpu_engine.trim_silence_probe(audio, lengths=lens, window_length=case.wl)
    assert conv.shape == (len(lens), max(case.N, case.W) + 1) and conv.dtype == np.float64
    errs = []
    for b, L in enumerate(lens):
        nc = abs(int(L) - case.W) + 1
        errs.append(T.conv_error(conv[b, :nc], T.reference(name)[b]))
    print(name, 'conv error / ((W + 2) 2^-52):', ' '.join(f'{x / ((case.W + 2) * 2.0 ** -52):.3g}' for x in errs))
    assert max(errs) <= (case.W + 2) * 2.0 ** -52, errs
    for mode in T.MODES:
        start, end = gpu_engine.trim_silence(audio, lengths=lens, window_length=case.wl, mode=mode)
        for b, L in enumerate(lens):
            nc = abs(int(L) - case.W) + 1
            assert (int(start[b]), int(end[b])) == audio_ref.trim_bounds(conv[b, :nc], int(L), case.wl, mode=mode), (name, mode, b)
    again = gpu_engine.trim_silence_probe(audio, lengths=lens, window_length=case.wl)
    assert np.array_equal(conv, again, equal_nan=True)


def test_probes_on_device_memory(gpu_engine):
    """The probes through device pointers (C ABI only) give the bits they give through host memory."""
    import torch
    name = 'sine_4609_1500_20480_noise3000'
    audio, lens, noise, nl = C.inputs_of(C.BY_NAME[name])
    got = _run(gpu_engine, name)
    a_d, n_d = torch.from_numpy(audio).cuda(), torch.from_numpy(noise).cuda()
    lib, h = gpu_engine._lib, gpu_engine._h
    B, N = audio.shape
    for what, s in ((5, 'threshold'), (6, 'mask'), (8, 'frames')):
        out = torch.full(got[s].shape, float('nan'), device='cuda')
        torch.cuda.synchronize()
        rc = lib.tts_hip_reduce_noise_probe(h, ctypes.c_void_p(a_d.data_ptr()), B, N, lens.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.c_void_p(n_d.data_ptr()), nl, what, ctypes.c_void_p(out.data_ptr()), 1)
        assert rc == 0 and _bits(out.cpu().numpy(), got[s]), s
    case = T.BY_NAME['wl1026_mixed']
    x, xl = T.audio_of(case)
    host = gpu_engine.trim_silence_probe(x, lengths=xl, window_length=case.wl)
    conv = torch.full((len(xl), max(case.N, case.W) + 1), float('nan'), device='cuda', dtype=torch.float64)
    x_d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    rc = lib.tts_hip_trim_silence_probe(h, ctypes.c_void_p(x_d.data_ptr()), len(xl), case.N, xl.ctypes.data_as(ctypes.c_void_p),
                                        case.wl, ctypes.c_void_p(conv.data_ptr()), 1)
    assert rc == 0
    conv = conv.cpu().numpy()
    for b, L in enumerate(xl):
        nc = abs(int(L) - case.W) + 1
        assert np.array_equal(conv[b, :nc], host[b, :nc])
