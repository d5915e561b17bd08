"""GPU: WaveGlow on a batch of unequal rows computed as ONE packed row (tts_hip_waveglow_infer_packed,
`waveglow_infer(..., lengths=..., packed=True)`).

The contract is the ragged call's (include/tts_hip.h): audio[b, :lengths[b] * 256] is what a one-row call on the row's own
frames returns, audio[b, lengths[b] * 256:] is exactly 0, nothing beyond a row's length is read.  Inputs and tolerances are
those of tests/test_waveglow_ragged_gpu.py: 1e-4 waveform RMS for fp32 and f16x3 against the solo oracle, F16_RMS_TOL for
f16, 5e-6 / 5e-5 for a row against a HIP run of the same frames.
"""
import ctypes
import queue

import numpy as np
import pytest

from conftest import rms
from test_waveglow_ragged_gpu import F16_RMS_TOL, PRECISIONS, RMS_TOL, _fill_tails, _inputs, _solo_oracle
from waveglow_packed_ref import header_gap_frames, packing_plan

pytestmark = pytest.mark.gpu

HIP_TOL = {'f32': 5e-6, 'f16': 5e-5, 'f16x3': 5e-6}


@pytest.mark.parametrize('B,T,lengths', [(3, 13, (13, 5, 9)), (2, 16, (9, 16)), (4, 9, (0, 9, 0, 1))])
def test_packed_rows_match_their_solo_oracle(gpu_engine, wg_weights, wg_cfg, B, T, lengths):
    """Every row against the numpy oracle on the row's own frames, all three precisions; tails exactly 0."""
    mel, z = _inputs(B, T)
    solo = [_solo_oracle(mel, z, b, n, wg_weights, wg_cfg) if n else np.zeros(0, np.float32) for b, n in enumerate(lengths)]
    for prec, tol in PRECISIONS:
        out = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths, packed=True)
        assert out.shape == (B, T * 256) and np.isfinite(out).all()
        for b, n in enumerate(lengths):
            err = rms(out[b, :n * 256] - solo[b]) if n else 0.0
            print(f'packed {prec} B={B} T={T} row {b} n={n}: rms_err vs solo oracle {err:.3e}')
            assert err <= tol
            assert not out[b, n * 256:].any()
            assert n == 0 or out[b, :n * 256].any()


def test_packed_winograd_size_against_the_oracle(gpu_engine, wg_weights, wg_cfg):
    """Lengths (100, 37) in a [2, 100] batch -- the oracle runs test_ragged_winograd_size_against_the_oracle uses -- plus a
    third row so that the packed row has F = 100 + 37 + 30 + 2 gaps >= 144 frames: fp32 in its Winograd form (mel planes and
    input transforms combine neighbouring frames and groups, across the gaps), the direct form and f16x3; NaN in every mel /
    z tail changes no bit."""
    lengths = (100, 37, 30)
    F = packing_plan(lengths, 100, header_gap_frames())['F']
    assert F == 167 + 2 * header_gap_frames() >= 144
    mel, z = _inputs(3, 100)
    solo = [_solo_oracle(mel, z, b, n, wg_weights, wg_cfg) for b, n in enumerate(lengths)]
    nan_mel, nan_z = _fill_tails(mel, z, lengths, np.nan, np.nan)
    try:
        runs = []
        for form, prec in (('winograd', 'f32'), ('direct', 'f32'), ('winograd', 'f16x3')):
            gpu_engine.set_waveglow_form(form)
            out = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths, packed=True)
            if prec == 'f32':
                assert gpu_engine.last_waveglow_form == form
            again = gpu_engine.waveglow_infer(nan_mel, z=nan_z, precision=prec, lengths=lengths, packed=True)
            assert np.array_equal(out, again), f'{form} {prec}: NaN tails changed the result'
            runs.append((form, prec, out))
    finally:
        gpu_engine.set_waveglow_form('winograd')
    for form, prec, out in runs:
        for b, n in enumerate(lengths):
            err = rms(out[b, :n * 256] - solo[b])
            print(f'packed {form} {prec} row {b} n={n}: rms_err vs solo oracle {err:.3e}')
            assert err <= RMS_TOL and not out[b, n * 256:].any()


def test_packed_config2_rows_equal_their_batch1_runs_and_the_ragged_call(gpu_engine):
    """8 x 800 frames with config-3-like lengths, F = 3164 packed frames against 6400: every row within the HIP-to-HIP
    tolerance of a batch-1 run of its own frames and of the ragged call's row; the zero-length row all zeros."""
    lengths = (800, 523, 77, 1, 640, 799, 300, 0)
    mel, z = _inputs(8, 800, seed=41)
    for prec in ('f32', 'f16', 'f16x3'):
        tol = HIP_TOL[prec]
        full = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths, packed=True)
        assert np.isfinite(full).all()
        if prec == 'f32':
            assert gpu_engine.last_waveglow_form == 'winograd'
        ragged = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths)
        for b, n in enumerate(lengths):
            assert not full[b, n * 256:].any()
            if n == 0:
                continue
            single = gpu_engine.waveglow_infer(np.ascontiguousarray(mel[b:b + 1, :n]),
                                               z=np.ascontiguousarray(z[b:b + 1, :n * 32]), precision=prec)
            e1, e2 = rms(single[0] - full[b, :n * 256]), rms(ragged[b, :n * 256] - full[b, :n * 256])
            print(f'packed {prec} row {b} n={n}: rms diff to its batch-1 run {e1:.3e}, to the ragged call\'s row {e2:.3e}')
            assert e1 <= tol and e2 <= tol


def test_packed_memory_kinds_streams_and_seeds(gpu_engine):
    """Host arrays, device tensors and `stream=` give the same bits (whatever the tails hold); `seed=` twice gives the same
    bits and, per row, the ragged call's audio: both draw the noise in the batch layout."""
    import torch
    B, T, lengths = 3, 21, (21, 6, 14)
    mel, z = _inputs(B, T, seed=13)
    nan_mel, nan_z = _fill_tails(mel, z, lengths, np.nan, np.inf)
    for prec in ('f32', 'f16', 'f16x3'):
        base = gpu_engine.waveglow_infer(mel, z=z, precision=prec, lengths=lengths, packed=True)
        assert np.array_equal(gpu_engine.waveglow_infer(nan_mel, z=nan_z, precision=prec, lengths=lengths, packed=True), base)
        dm, dz = torch.as_tensor(nan_mel).cuda(), torch.as_tensor(nan_z).cuda()
        dev = gpu_engine.waveglow_infer(dm, z=dz, precision=prec, lengths=lengths, packed=True)
        assert np.array_equal(dev.cpu().numpy(), base)
        st = torch.cuda.Stream()
        on_stream = gpu_engine.waveglow_infer(dm, z=dz, precision=prec, lengths=torch.as_tensor(lengths), stream=st, packed=True)
        st.synchronize()
        assert np.array_equal(on_stream.cpu().numpy(), base)
        # seeded noise: host mel, device mel, a caller's stream
        a = gpu_engine.waveglow_infer(mel, seed=5, offset=3, precision=prec, lengths=lengths, packed=True)
        assert np.array_equal(a, gpu_engine.waveglow_infer(nan_mel, seed=5, offset=3, precision=prec, lengths=lengths, packed=True))
        assert np.array_equal(a, gpu_engine.waveglow_infer(dm, seed=5, offset=3, precision=prec, lengths=lengths,
                                                           packed=True).cpu().numpy())
        s2 = gpu_engine.waveglow_infer(dm, seed=5, offset=3, precision=prec, lengths=lengths, packed=True, stream=st)
        st.synchronize()
        assert np.array_equal(a, s2.cpu().numpy())
        assert not np.array_equal(a, gpu_engine.waveglow_infer(mel, seed=6, offset=3, precision=prec, lengths=lengths, packed=True))
        ragged = gpu_engine.waveglow_infer(mel, seed=5, offset=3, precision=prec, lengths=lengths)
        for b, n in enumerate(lengths):
            err = rms(a[b, :n * 256] - ragged[b, :n * 256])
            print(f'packed {prec} seeded row {b} n={n}: rms diff to the ragged call {err:.3e}')
            assert err <= HIP_TOL[prec] and not a[b, n * 256:].any() and a[b, :n * 256].any()
    # no z, no seed: zeros for noise
    det = gpu_engine.waveglow_infer(mel, lengths=lengths, packed=True)
    assert rms(det - gpu_engine.waveglow_infer(mel, lengths=lengths)) <= HIP_TOL['f32']


def test_packed_row_above_the_one_call_limit_is_refused(gpu_engine):
    """F = 4 x 8000 + 3 gaps = 32012 > 31744: TTS_HIP_EINVAL with F and the limit in the message, nothing launched (the
    output keeps its bytes), no fall-back to the ragged call -- which takes this shape in slices."""
    from text_to_speech_amd._lib import HipLibraryError
    B, T = 4, 8000
    F = packing_plan((T,) * B, T, header_gap_frames())['F']
    mel = np.zeros((B, T, 80), np.float32)
    with pytest.raises(HipLibraryError, match=f'F = {F} frames.*31744'):
        gpu_engine.waveglow_infer(mel, lengths=(T,) * B, packed=True)
    import torch
    dm = torch.zeros((B, T, 80), device='cuda')
    out = torch.full((B, T * 256), 7.0, device='cuda')
    lens = np.full(B, T, np.int32)
    torch.cuda.synchronize()
    for prec in (0, 1, 2):
        rc = gpu_engine._lib.tts_hip_waveglow_infer_packed(
            gpu_engine._h, ctypes.c_void_p(dm.data_ptr()), B, T, lens.ctypes.data_as(ctypes.c_void_p), None, 1.0,
            ctypes.c_void_p(out.data_ptr()), prec, 1)
        assert rc == -1 and f'F = {F} frames'.encode() in gpu_engine._lib.tts_hip_last_error(gpu_engine._h)
    gpu_engine.synchronize()
    assert bool((out == 7.0).all())
    # T alone is not limited: two short rows of a very wide batch fit
    wide = gpu_engine.waveglow_infer(np.zeros((2, 40000, 80), np.float32), lengths=(3, 2), packed=True)
    assert wide.shape == (2, 40000 * 256) and not wide[:, 3 * 256:].any()
    # lengths are checked by the C entry point itself
    bad = np.asarray([T + 1, 0, 0, 0], np.int32)
    rc = gpu_engine._lib.tts_hip_waveglow_infer_packed(
        gpu_engine._h, ctypes.c_void_p(dm.data_ptr()), B, T, bad.ctypes.data_as(ctypes.c_void_p), None, 1.0,
        ctypes.c_void_p(out.data_ptr()), 0, 1)
    assert rc == -1 and b'lengths[0]' in gpu_engine._lib.tts_hip_last_error(gpu_engine._h)


def test_runtime_and_wrapper_pass_packed(gpu_engine):
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.waveglow import WaveGlow
    lengths = (9, 4)
    mel, z = _inputs(2, 9, seed=17)
    want = gpu_engine.waveglow_infer(mel, z=z, lengths=lengths, packed=True)
    rt = HipRuntime('synthetic', model='waveglow', engine=gpu_engine, seed=3)
    voc = WaveGlow(rt)
    assert np.array_equal(voc.infer(mel, z=z, lengths=lengths, packed=True), want)
    assert rms(want - voc(mel, z=z, lengths=lengths)) <= HIP_TOL['f32']
    # the runtime's running noise offset advances as for the ragged call: the next draws agree
    rt2 = HipRuntime('synthetic', model='waveglow', engine=gpu_engine, seed=3)
    voc(mel, lengths=lengths, packed=True)
    WaveGlow(rt2)(mel, lengths=lengths)
    a, b = voc(mel, lengths=lengths, packed=True), WaveGlow(rt2)(mel, lengths=lengths)
    assert rms(a - b) <= HIP_TOL['f32'] and a[0].any() and not a[1, 4 * 256:].any()


def test_stream_backlog_packed_against_the_ragged_backlog(gpu_engine):
    """The 16 sentences of tests/test_stream_backlog_gpu.py, fp32, deterministic: `batch_backlog=8, pack_vocoder=True`
    delivers the same texts in the same order with the same mels as `batch_backlog=8`, and each waveform within 5e-6 RMS of
    the ragged backlog's and of a batch-1 vocoding of its own mel."""
    from test_stream_backlog_gpu import MEL_TOL, _sentences
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2, stream
    from text_to_speech_amd.waveglow import WaveGlow
    model = Tacotron2(HipRuntime('t6', model='tacotron2', engine=gpu_engine, seed=0))
    voc = WaveGlow(HipRuntime('w6', model='waveglow', engine=gpu_engine, seed=0))
    texts = _sentences(16)
    run_kw = dict(model=model, vocoder=voc, max_length=3., deterministic=True, save=False)

    def record(rec):
        return [lambda text, audio, mel, **_: rec.append((text, np.asarray(audio).copy(), [np.asarray(m).copy() for m in mel]))]

    back, pack = [], []
    stream(iter(texts), callbacks=record(back), batch_backlog=8, **run_kw)
    q = queue.Queue()
    for t in texts + [None]:
        q.put(t)
    stream(q, callbacks=record(pack), batch_backlog=8, pack_vocoder=True, **run_kw)
    assert [r[0] for r in back] == [r[0] for r in pack] == texts
    n_tok = [len(model.encode_text(model.clean_text(t), cleaned=True)) for t in texts]
    worst_mel = worst_rag = worst_own = 0.0
    for (_, a, m), (_, b, mb), n in zip(back, pack, n_tok):
        frames = int(np.float32(n) * np.float32(3.))
        assert a.shape == b.shape == (frames * 256,) and np.isfinite(b).all() and b.any()
        assert len(m) == len(mb) == 1 and m[0].shape == mb[0].shape == (frames, 80)
        worst_mel = max(worst_mel, float(np.abs(m[0] - mb[0]).max()))
        own = np.asarray(voc(mb[0][None], deterministic=True))[0]
        worst_own = max(worst_own, rms(own - b))
        worst_rag = max(worst_rag, rms(a - b))
    print(f'packed backlog stream vs ragged backlog stream: mel max abs diff {worst_mel:.2e}; audio RMS diff {worst_rag:.2e}; '
          f'audio RMS diff to a batch-1 vocoding of the own mel {worst_own:.2e}')
    assert worst_mel <= MEL_TOL
    assert worst_own <= 5e-6 and worst_rag <= 5e-6
    with pytest.raises(ValueError, match='pack_vocoder'):
        stream(iter(texts[:2]), pack_vocoder=True, **run_kw)
