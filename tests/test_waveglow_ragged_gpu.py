"""GPU: WaveGlow on a batch of unequal rows (tts_hip_waveglow_infer_ragged, `waveglow_infer(..., lengths=...)`).

Contract (include/tts_hip.h): audio[b, :lengths[b] * 256] is what a one-row call on the row's own frames returns,
audio[b, lengths[b] * 256:] is exactly 0, nothing beyond a row's length is read (NaN there changes no bit), and
lengths=None is the call without the argument.  Inputs: tests/test_waveglow_gpu.py's recipe; tolerances: the project's own
(1e-4 waveform RMS for fp32 and f16x3 against the oracle, F16_RMS_TOL for f16, 5e-6 / 5e-5 for a batch row against its
HIP batch-1 run -- what test_waveglow_config2_rows_equal_batch1_runs holds rows to).
"""
import numpy as np
import pytest

from conftest import rms

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4
F16_RMS_TOL = 1e-3
PRECISIONS = (('f32', RMS_TOL), ('f16', F16_RMS_TOL), ('f16x3', RMS_TOL))


def _inputs(B, T, seed=7):
    mel = np.random.default_rng(seed).uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    z = np.random.default_rng(seed + 4).standard_normal((B, T * 32, 8)).astype(np.float32)
    return mel, z


def _solo_oracle(mel, z, b, n, wg_weights, wg_cfg):
    from oracle import waveglow_ref
    return waveglow_ref.infer(mel[b:b + 1, :n], wg_weights, wg_cfg, z=z[b:b + 1, :n * 32], sigma=1.0)[0]


def _fill_tails(mel, z, lengths, mel_value, z_value):
    mel, z = mel.copy(), z.copy()
    for b, n in enumerate(lengths):
        mel[b, n:] = mel_value if np.isscalar(mel_value) else mel_value[b, n:]
        z[b, n * 32:] = z_value if np.isscalar(z_value) else z_value[b, n * 32:]
    return mel, z


@pytest.mark.parametrize('B,T,lengths', [(3, 13, (13, 5, 9)), (2, 16, (9, 16))])
def test_ragged_rows_match_their_solo_oracle(gpu_engine, wg_weights, wg_cfg, B, T, lengths):
    """Every row against the numpy oracle on the row's own frames, all three precisions -- and the padded call of the same
    batch (tails filled with -11, the reference's batched path) beside it: its short rows miss their solo oracle by more
    than 100 x the tolerance (3e-2 .. 5e-2 RMS), which is what the per-row lengths are for."""
    mel, z = _inputs(B, T)
    solo = [_solo_oracle(mel, z, b, n, wg_weights, wg_cfg) for b, n in enumerate(lengths)]
    for prec, tol in PRECISIONS:
        out = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths)
        assert out.shape == (B, T * 256) and np.isfinite(out).all()
        for b, n in enumerate(lengths):
            err = rms(out[b, :n * 256] - solo[b])
            print(f'{prec} B={B} T={T} row {b} n={n}: rms_err vs solo oracle {err:.3e} (solo rms {rms(solo[b]):.3f})')
            assert err <= tol
            assert not out[b, n * 256:].any()
    padded_mel, _ = _fill_tails(mel, z, lengths, -11.0, 0.0)
    padded = gpu_engine.waveglow_infer(padded_mel, z=z)
    for b, n in enumerate(lengths):
        err = rms(padded[b, :n * 256] - solo[b])
        print(f'padded call B={B} T={T} row {b} n={n}: rms_err vs solo oracle {err:.3e}')
        if n < T:
            assert err > 100 * RMS_TOL
        else:
            assert err <= RMS_TOL


def test_ragged_winograd_size_against_the_oracle(gpu_engine, wg_weights, wg_cfg):
    """200 frames per call: the fp32 path runs its Winograd form (mel planes and input transforms combine neighbouring frames
    and groups); then the direct form and f16x3 on the same inputs."""
    lengths = (100, 37)
    mel, z = _inputs(2, 100)
    solo = [_solo_oracle(mel, z, b, n, wg_weights, wg_cfg) for b, n in enumerate(lengths)]
    nan_mel, nan_z = _fill_tails(mel, z, lengths, np.nan, np.nan)
    try:
        runs = []
        for form, prec in (('winograd', 'f32'), ('direct', 'f32'), ('winograd', 'f16x3')):
            gpu_engine.set_waveglow_form(form)
            out = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths)
            if prec == 'f32':
                assert gpu_engine.last_waveglow_form == form
            again = gpu_engine.waveglow_infer(nan_mel, z=nan_z, precision=prec, lengths=lengths)
            assert np.array_equal(out, again), f'{form} {prec}: NaN tails changed the result'
            runs.append((form, prec, out))
    finally:
        gpu_engine.set_waveglow_form('winograd')
    for form, prec, out in runs:
        for b, n in enumerate(lengths):
            err = rms(out[b, :n * 256] - solo[b])
            print(f'{form} {prec} row {b} n={n}: rms_err vs solo oracle {err:.3e}')
            assert err <= RMS_TOL and not out[b, n * 256:].any()


def test_ragged_config2_rows_equal_their_batch1_runs(gpu_engine):
    """8 x 800 frames (256-row tiles; fp32 in the Winograd form) with config-3-like lengths: rows against HIP batch-1 runs of
    their own frames, the zero-length row all zeros."""
    lengths = (800, 523, 77, 1, 640, 799, 300, 0)
    mel, z = _inputs(8, 800, seed=41)
    for prec, tol in (('f32', 5e-6), ('f16', 5e-5), ('f16x3', 5e-6)):
        full = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths)
        assert gpu_engine.last_waveglow_tiles == '256-row' and np.isfinite(full).all()
        if prec == 'f32':
            assert gpu_engine.last_waveglow_form == 'winograd'
        for b, n in enumerate(lengths):
            assert not full[b, n * 256:].any()
        for b in (1, 2, 3, 5):
            n = lengths[b]
            single = gpu_engine.waveglow_infer(np.ascontiguousarray(mel[b:b + 1, :n]),
                                               z=np.ascontiguousarray(z[b:b + 1, :n * 32]), precision=prec)
            err = rms(single[0] - full[b, :n * 256])
            print(f'{prec} row {b} n={n}: rms diff to its batch-1 run {err:.3e}')
            assert err <= tol


@pytest.mark.parametrize('B,T,lengths,tiles', [(2, 13, (13, 4), ('64-row',)), (1, 100, (61,), ('128-row', '128x64')),
                                               (2, 128, (128, 50), ('256-row',))])
def test_ragged_tails(gpu_engine, B, T, lengths, tiles):
    """Zero tails, independence of the tail contents (-11 / random / NaN in mel and z), lengths=None and full lengths; host
    and device memory and the stream-ordered entry; one case per tile family."""
    import torch
    mel, z = _inputs(B, T, seed=13)
    other_mel, other_z = _inputs(B, T, seed=99)
    variants = [_fill_tails(mel, z, lengths, -11.0, 0.0), _fill_tails(mel, z, lengths, other_mel, other_z),
                _fill_tails(mel, z, lengths, np.nan, np.nan), _fill_tails(mel, z, lengths, np.inf, -np.inf)]
    for prec in ('f32', 'f16', 'f16x3'):
        base = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths)
        if prec != 'f16x3':
            assert gpu_engine.last_waveglow_tiles in tiles
        assert np.isfinite(base).all()
        for b, n in enumerate(lengths):
            assert not base[b, n * 256:].any() and base[b, :n * 256].any()
        for m2, z2 in variants:
            assert np.array_equal(gpu_engine.waveglow_infer(m2, z=z2, precision=prec, lengths=lengths), base)
        # device memory, the engine's stream and a caller's stream
        dm, dz = torch.as_tensor(variants[2][0]).cuda(), torch.as_tensor(variants[2][1]).cuda()
        assert np.array_equal(gpu_engine.waveglow_infer(dm, z=dz, precision=prec, lengths=lengths).cpu().numpy(), base)
        st = torch.cuda.Stream()
        on_stream = gpu_engine.waveglow_infer(dm, z=dz, precision=prec, lengths=torch.as_tensor(lengths), stream=st)
        st.synchronize()
        assert np.array_equal(on_stream.cpu().numpy(), base)
        # lengths=None is the call without the argument; full lengths compute the same thing
        plain = gpu_engine.waveglow_infer(mel, z=z, precision=prec)
        assert np.array_equal(gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=None), plain)
        full = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=[T] * B)
        assert rms(full - plain) <= 5e-6
    # no z: the deterministic path; seeded noise is drawn in the batch layout, so a row's real part equals the seeded padded
    # call's noise on a clean row only -- here: reproducible and zero-tailed
    a = gpu_engine.waveglow_infer(mel, seed=5, lengths=lengths)
    assert np.array_equal(a, gpu_engine.waveglow_infer(variants[2][0], seed=5, lengths=lengths))
    for b, n in enumerate(lengths):
        assert not a[b, n * 256:].any()


def test_ragged_lengths_are_checked(gpu_engine):
    from text_to_speech_amd._lib import HipLibraryError
    import ctypes
    mel, z = _inputs(2, 6)
    for bad in ((7, 1), (-1, 3), (6,), (1.5, 2.0)):
        with pytest.raises(ValueError):
            gpu_engine.waveglow_infer(mel, z=z, lengths=bad)
    # ... and by the C entry point itself
    out = np.empty((2, 6 * 256), np.float32)
    lens = np.asarray([6, 7], np.int32)
    rc = gpu_engine._lib.tts_hip_waveglow_infer_ragged(
        gpu_engine._h, mel.ctypes.data_as(ctypes.c_void_p), 2, 6, lens.ctypes.data_as(ctypes.c_void_p), None, 1.0,
        out.ctypes.data_as(ctypes.c_void_p), 0, 0)
    assert rc == -1 and b'lengths[1] = 7' in gpu_engine._lib.tts_hip_last_error(gpu_engine._h)
    with pytest.raises(HipLibraryError):
        gpu_engine._check(rc, 'waveglow_infer_ragged')


def test_runtime_and_wrapper_pass_lengths(gpu_engine):
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.waveglow import WaveGlow
    lengths = (9, 4)
    mel, z = _inputs(2, 9, seed=17)
    want = gpu_engine.waveglow_infer(mel, z=z, lengths=lengths)
    voc = WaveGlow(HipRuntime('synthetic', model='waveglow', engine=gpu_engine))
    assert np.array_equal(voc.infer(mel, z=z, lengths=lengths), want)
    assert np.array_equal(voc(mel, z=z), gpu_engine.waveglow_infer(mel, z=z))
    det = voc(mel, deterministic=True, lengths=np.asarray(lengths))
    assert det.shape == (2, 9 * 256) and not det[1, 4 * 256:].any()
