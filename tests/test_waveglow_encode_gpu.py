"""GPU: the forward flow (HipEngine.waveglow_encode, tts_hip_waveglow_encode[_async]) against its float64 restatement
(tests/waveglow_encode_ref.py), its ragged contract, its layout edges and its determinism.

Bounds.  Oracle cases: every case computes the float32 floor of its own inputs from the restatement (never from the engine)
and allows the engine ten times it -- z as an RMS error, the three statistics relative to their float64 value; the floor of a
statistic is not taken below 2^-24, the rounding of a value stored as one float32 (waveglow_encode_ref.Case).  GPU against
GPU (no float64 reference at these sizes): the project's waveform tolerance RMS_TOL = 1e-4.
Shapes: the oracle cases of tests/test_waveglow_gpu.py (8, 10 and 15 frames: one 64-row tile per phase, more than one
block of the position-wise kernels); layout edges at 64 frames (no padding rows), 65 (phase rows turn over to 128) and 150
(the Winograd form, from 144 frames on).
Measured on MI355X: z 1.15 .. 1.30 floors (2.5e-7 RMS on the session weights, 1.4e-6 on the general kernels), sum_z2 and
log_det_w within 1.2 of their 2^-24 floor, sum_log_s 0.1 .. 7 floors; ragged rows bit-equal to their own calls; round trips
1.6e-7 .. 2.0e-7 RMS; Winograd against direct z 2.9e-7.
"""
import numpy as np
import pytest

import waveglow_encode_ref as ref
from conftest import rms
from test_waveglow_gpu import RMS_TOL

pytestmark = pytest.mark.gpu


def _inputs(B, T, seed=21):
    rng = np.random.default_rng(seed + 100 * B + T)
    mel = rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    audio = rng.uniform(-0.9, 0.9, (B, T * 256)).astype(np.float32)
    return audio, mel


def _check_against(case, z, stats, what):
    """Prints every figure, then asserts z and the statistics within the case's bounds."""
    ez, es = case.errors(z, stats)
    print(f'{what}: z rms err {ez:.3e} (floor {case.z_floor:.3e}, {ez / case.z_floor:.2f} floors; z rms {rms(case.z):.3f})')
    for i, name in enumerate(('sum_z2', 'sum_log_s', 'log_det_w')):
        print(f'  {name}: value {case.stats[i].tolist()} rel err {es[i].tolist()} floor {case.stats_floor[i].tolist()}')
    assert np.isfinite(z).all() and np.isfinite(stats).all()
    assert ez <= case.z_bound
    assert np.all(es <= case.stats_bound)


@pytest.fixture(scope='module')
def replaced(wg_weights, wg_cfg):
    return ref.replace_invertible_kernels(wg_weights, wg_cfg)


@pytest.fixture(scope='module')
def eng_replaced(replaced):
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.load_state(replaced)
    eng.finalize()
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def model256():
    from text_to_speech_amd import weights
    from text_to_speech_amd.config import WaveGlowConfig
    from text_to_speech_amd.engine import HipEngine
    cfg = WaveGlowConfig(n_channels=256)
    w = weights.synth_waveglow(cfg, seed=1234)
    eng = HipEngine(0)
    eng.load_state(w)
    eng.finalize()
    yield eng, w, cfg
    eng.close()


# ---- against the float64 restatement
@pytest.mark.parametrize('B,T', [(1, 8), (2, 5), (3, 5)])
def test_encode_matches_the_restatement(gpu_engine, wg_weights, wg_cfg, B, T):
    audio, mel = _inputs(B, T)
    case = ref.Case(audio, mel, wg_weights, wg_cfg)
    z, stats = gpu_engine.waveglow_encode(audio, mel)
    assert z.shape == (B, T * 32, 8) and stats.shape == (3, B) and z.dtype == stats.dtype == np.float32
    assert gpu_engine.last_waveglow_form == 'direct'
    _check_against(case, z, stats, f'{B} x {T}')


def test_encode_with_general_kernels(eng_replaced, replaced, wg_cfg):
    """Kernels Q1 diag(d) Q2 with negative determinants among them: log_det_w is not 0 and a transposed matrix is no inverse."""
    audio, mel = _inputs(2, 5)
    case = ref.Case(audio, mel, replaced, wg_cfg)
    z, stats = eng_replaced.waveglow_encode(audio, mel)
    assert abs(case.stats[2, 0]) > 100
    _check_against(case, z, stats, 'replaced kernels 2 x 5')
    back = eng_replaced.waveglow_infer(mel, z=z, sigma=1.0)
    print(f'  round trip rms {rms(back - audio):.3e}')
    assert rms(back - audio) <= RMS_TOL


def test_encode_256_channels(model256):
    eng, w, cfg = model256
    audio, mel = _inputs(1, 6)
    case = ref.Case(audio, mel, w, cfg)
    z, stats = eng.waveglow_encode(audio, mel)
    assert eng.waveglow_channels == 256
    _check_against(case, z, stats, '256 channels 1 x 6')


# ---- ragged
def test_ragged_rows_are_calls_of_their_own(gpu_engine, wg_weights, wg_cfg):
    T, lengths = 13, [13, 0, 6]
    audio, mel = _inputs(3, T)
    case = ref.Case(audio, mel, wg_weights, wg_cfg, lengths=lengths)
    nan_audio, nan_mel = audio.copy(), mel.copy()
    for b, n in enumerate(lengths):
        nan_audio[b, n * 256:] = np.nan
        nan_mel[b, n:] = np.nan
    z, stats = gpu_engine.waveglow_encode(nan_audio, nan_mel, lengths=lengths)
    _check_against(case, z, stats, f'ragged {lengths} of {T}')
    for b, n in enumerate(lengths):
        assert not z[b, n * 32:].any()                                      # exactly 0 behind a row's length
        if n == 0:
            assert not stats[:, b].any()                                    # the empty row: exactly 0
            continue
        z1, s1 = gpu_engine.waveglow_encode(audio[b:b + 1, :n * 256], mel[b:b + 1, :n])
        err = rms(z[b, :n * 32] - z1[0])
        rel = ref.rel_err(stats[:, b], s1[:, 0])
        print(f'  row {b} ({n} frames) against its own call: z rms {err:.3e}, statistics rel {rel.tolist()}')
        assert err <= RMS_TOL and np.all(rel <= RMS_TOL)


# ---- layout edges, GPU against GPU
@pytest.mark.parametrize('T', [64, 65])
def test_round_trip_at_the_padding_edges(gpu_engine, T):
    audio, mel = _inputs(1, T)
    z, stats = gpu_engine.waveglow_encode(audio, mel)
    back = gpu_engine.waveglow_infer(mel, z=z, sigma=1.0)
    print(f'{T} frames: round trip rms {rms(back - audio):.3e}, z rms {rms(z):.3f}, stats {stats[:, 0].tolist()}')
    assert np.isfinite(z).all() and 0.3 < rms(z) < 1.0
    assert rms(back - audio) <= RMS_TOL
    assert np.isclose(stats[0, 0], np.square(z.astype(np.float64)).sum(), rtol=1e-6)


def test_both_forms_at_150_frames(gpu_engine):
    audio, mel = _inputs(1, 150)
    try:
        gpu_engine.set_waveglow_form('winograd')
        zw, sw = gpu_engine.waveglow_encode(audio, mel)
        assert gpu_engine.last_waveglow_form == 'winograd'
        back_w = gpu_engine.waveglow_infer(mel, z=zw, sigma=1.0)
        gpu_engine.set_waveglow_form('direct')
        zd, sd = gpu_engine.waveglow_encode(audio, mel)
        assert gpu_engine.last_waveglow_form == 'direct'
        back_d = gpu_engine.waveglow_infer(mel, z=zd, sigma=1.0)
    finally:
        gpu_engine.set_waveglow_form('winograd')                            # the handle's default
    rel = ref.rel_err(sw[:2], sd[:2])
    print(f'150 frames: z winograd vs direct rms {rms(zw - zd):.3e}; round trips {rms(back_w - audio):.3e} / '
          f'{rms(back_d - audio):.3e}; statistics rel {rel.tolist()}')
    assert rms(zw - zd) <= RMS_TOL and not np.array_equal(zw, zd)
    assert rms(back_w - audio) <= RMS_TOL and rms(back_d - audio) <= RMS_TOL
    assert np.all(rel <= RMS_TOL) and sw[2, 0] == sd[2, 0]


# ---- equality checks
def test_repeats_host_device_and_stream_give_the_same_bits(gpu_engine):
    import torch
    T, lengths = 13, [13, 0, 6]
    audio, mel = _inputs(3, T)
    before = gpu_engine.waveglow_infer(mel, z=None)
    z, stats = gpu_engine.waveglow_encode(audio, mel, lengths=lengths)
    # an infer call right after an encode call gives the bits it gave before
    assert np.array_equal(gpu_engine.waveglow_infer(mel, z=None), before)
    z2, stats2 = gpu_engine.waveglow_encode(audio, mel, lengths=lengths)
    assert np.array_equal(z, z2) and np.array_equal(stats, stats2)
    da, dm = torch.as_tensor(audio).cuda(), torch.as_tensor(mel).cuda()
    dz, ds = gpu_engine.waveglow_encode(da, dm, lengths=lengths)
    assert dz.is_cuda and ds.is_cuda
    assert np.array_equal(dz.cpu().numpy(), z) and np.array_equal(ds.cpu().numpy(), stats)
    st = torch.cuda.Stream()
    sz, ss = gpu_engine.waveglow_encode(da, dm, lengths=torch.as_tensor(lengths), stream=st)
    st.synchronize()
    assert np.array_equal(sz.cpu().numpy(), z) and np.array_equal(ss.cpu().numpy(), stats)
    # without lengths too, and the plain call differs from the ragged one where it must
    zp, sp = gpu_engine.waveglow_encode(audio, mel)
    zq, sq = gpu_engine.waveglow_encode(da, dm)
    assert np.array_equal(zq.cpu().numpy(), zp) and np.array_equal(sq.cpu().numpy(), sp)
    assert zp[1].any() and not z[1].any()
    with pytest.raises(ValueError, match='stream= needs device tensors'):
        gpu_engine.waveglow_encode(audio, mel, stream=st)


def test_outputs_may_be_null_one_at_a_time(gpu_engine):
    """z or stats NULL through the C symbol: the other output has the bits of the full call."""
    audio, mel = _inputs(2, 5)
    z, stats = gpu_engine.waveglow_encode(audio, mel)
    lib, h, ptr = gpu_engine._lib, gpu_engine._h, gpu_engine._ptr
    z_only, stats_only = np.empty_like(z), np.empty_like(stats)
    assert lib.tts_hip_waveglow_encode(h, ptr(audio), ptr(mel), 2, 5, None, ptr(z_only), None, 0) == 0
    assert lib.tts_hip_waveglow_encode(h, ptr(audio), ptr(mel), 2, 5, None, None, ptr(stats_only), 0) == 0
    assert np.array_equal(z_only, z) and np.array_equal(stats_only, stats)


def test_refusals_through_the_real_symbols(gpu_engine):
    audio, mel = _inputs(2, 5)
    lib, h, ptr = gpu_engine._lib, gpu_engine._h, gpu_engine._ptr
    z, stats = np.full((2, 160, 8), 7, np.float32), np.full((3, 2), 7, np.float32)
    lens = lambda *v: np.array(v, dtype=np.int32)

    def refused(name, *args):
        rc = getattr(lib, name)(h, *args)
        msg = lib.tts_hip_last_error(h).decode()
        assert rc == -1 and msg.startswith(name + ': '), (rc, msg)
        return msg

    sync, a, m = 'tts_hip_waveglow_encode', ptr(audio), ptr(mel)
    assert 'bad mem kind 7' in refused(sync, a, m, 0, 5, None, ptr(z), ptr(stats), 7)          # mem before B
    assert 'B = 0' in refused(sync, a, m, 0, 0, None, None, None, 0)                             # B before T and the outputs
    assert 'T = 0' in refused(sync, a, m, 2, 0, None, None, None, 0)
    assert 'audio or mel is NULL' in refused(sync, None, m, 2, 5, None, ptr(z), ptr(stats), 0)
    assert 'both NULL' in refused(sync, a, m, 2, 5, ptr(lens(5, 9)), None, None, 0)              # outputs before lengths
    assert 'lengths[1] = 9' in refused(sync, a, m, 2, 5, ptr(lens(5, 9)), ptr(z), ptr(stats), 0)
    assert 'lengths[0] = -1' in refused(sync, a, m, 2, 31744, ptr(lens(-1, 0)), ptr(z), ptr(stats), 0)   # lengths before B * T
    assert 'exceeds one run' in refused(sync, a, m, 2, 15873, None, ptr(z), ptr(stats), 0)
    assert 'exceeds one run' in refused('tts_hip_waveglow_encode_async', a, m, 1, 31745, None, ptr(z), ptr(stats), None)
    assert 'both NULL' in refused('tts_hip_waveglow_encode_async', a, m, 2, 5, None, None, None, None)
    assert np.all(z == 7) and np.all(stats == 7)                             # nothing was written
    from text_to_speech_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match='tts_hip_waveglow_encode: B \\* T = 31745 frames exceeds'):
        gpu_engine.waveglow_encode(np.zeros((1, 31745 * 256), np.float32), np.zeros((1, 31745, 80), np.float32))


def test_model_level_encode_and_evaluate(gpu_engine):
    """WaveGlow.encode / evaluate on the real runtime: evaluate's rows are encode's, and the latent re-synthesizes the audio."""
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.waveglow import WaveGlow
    model = WaveGlow(HipRuntime(None, model='waveglow', engine=gpu_engine))
    items = [_inputs(1, t) for t in (6, 9, 4)]
    items = [(a[0, :a.shape[1] - 40], m[0]) for a, m in items]              # (waveform 40 samples short of its mel, mel)
    res = model.evaluate(items, batch_size=2, sigma=0.8)
    assert res['per_item'].shape == (4, 3) and np.isfinite(res['per_item']).all()
    for i, (a, m) in enumerate(items):
        one = model.encode(a, m)
        want = (one['sum_z2'] / (2 * 0.8 ** 2) - one['sum_log_s'] - one['log_det_w']) / (m.shape[0] * 256)
        got = res['per_item'][:, i]
        print(f'item {i}: nll {got[0]:.6f} (alone {want:.6f})')
        assert np.isclose(got[0], want, rtol=RMS_TOL) and np.allclose(got[1:3], [one['sum_z2'], one['sum_log_s']], rtol=RMS_TOL)
        padded = np.zeros(m.shape[0] * 256, np.float32)
        padded[:len(a)] = a
        back = model.infer(m, z=one['z'][None], sigma=1.0, deterministic=True)
        assert rms(np.asarray(back)[0] - padded) <= RMS_TOL
