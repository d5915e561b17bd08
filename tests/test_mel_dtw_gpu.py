"""GPU: tts_hip_mel_dtw stage by stage (through tts_hip_mel_dtw_probe), each stage against float64 applied to the run's own stage
before it, so that no bound has to cover a tie that float32 and float64 break differently:

  cepstra     within (n_mel + 1) 2^-24 sum_k |D[r][k] m[k]| per coefficient (n_mel fused multiply-adds in sequence)
  distance    within (n_cep + 4) 2^-24 d
  cost        within (i + j + 1) 2^-24 C(i, j): the terms are non-negative and a cell adds one rounding
  step codes  exactly the documented argmin of the run's own cost matrix
  path        exactly the backtrack of the run's own step codes
  statistics  cost bit-equal to the probe's C(la - 1, lb - 1), path_len exact, mcd within two roundings
  end to end  the cost against float64 from the run's own cepstra, within (n_cep + 4 + la + lb) 2^-24 cost

and the path length against the float64 path on the cases tests/test_mel_dtw.py finds decided by a margin (STABLE_PATHS).
Then: rows alone bit-equal to rows in a ragged batch with NaN behind both lengths, host = device = stream, the un-aligned mode,
`return_path=False`, and `Tacotron2.evaluate_synthesis` / `WaveGlow.copy_synthesis` bit-equal to their parts.
"""
import numpy as np
import pytest

import mel_dtw_cases as mc
import mel_dtw_ref as mr

pytestmark = pytest.mark.gpu


def check_row(name, a, b, la, lb, n_cep, c0, got, stats, path):
    """Every stage check of one row: `got` the probe's dense stages of the row, `stats` [3], `path` [K, 2]."""
    n_mel = a.shape[1]
    R = n_cep + int(c0)
    D = mr.dct_table(n_mel, n_cep, c0)
    for key, m, n in (('cepstra_a', a, la), ('cepstra_b', b, lb)):
        c = got[key]
        assert c.shape[1] == R and np.all(c[n:] == 0), (name, key)
        err = np.abs(c[:n].astype(np.float64) - mr.cepstra(m[:n], D))
        bound = mr.cepstra_bound(m[:n], D)
        print(f'{name} {key}: largest error / bound = {(err / bound).max():.3g}')
        assert np.all(err <= bound), (name, key, float((err / bound).max()))
    ca, cb = got['cepstra_a'][:la].astype(np.float64), got['cepstra_b'][:lb].astype(np.float64)
    d, C, step = got['distance'], got['cost'], got['step']
    for m in (d, C, step):
        assert m.shape[0] >= la and m.shape[1] >= lb and np.all(m[la:] == 0) and np.all(m[:, lb:] == 0), name
    d, C, step = d[:la, :lb], C[:la, :lb], step[:la, :lb]
    assert np.isfinite(d).all() and np.isfinite(C).all(), name
    ref_d = mr.distance(ca, cb)
    err = np.abs(d - ref_d)
    print(f'{name} distance: largest error / bound = {(err / np.maximum((n_cep + 4) * mr.EPS * ref_d, 1e-300)).max():.3g}')
    assert np.all(err <= (n_cep + 4) * mr.EPS * ref_d), name
    ref_C, _ = mr.accumulate(d.astype(np.float64))
    ij = np.add.outer(np.arange(la), np.arange(lb)) + 1
    err = np.abs(C - ref_C)
    print(f'{name} cost: largest error / bound = {(err / np.maximum(ij * mr.EPS * ref_C, 1e-300)).max():.3g}')
    assert np.all(err <= ij * mr.EPS * ref_C), name
    assert np.array_equal(step, mr.argmin_codes(C)), name
    want_path = mr.backtrack(step.astype(np.int64))
    n = len(want_path)
    assert path.shape[0] >= la + lb - 1 and np.array_equal(path[:n], np.asarray(want_path)) and np.all(path[n:] == -1), name
    assert stats.dtype == np.float32 and stats[0] == C[la - 1, lb - 1] and stats[1] == n, (name, stats)
    want_mcd = mr.MCD_DB_FACTOR * float(stats[0]) / n
    assert abs(float(stats[2]) - want_mcd) <= 2 * mr.EPS * want_mcd, (name, stats, want_mcd)
    ref = mr.mel_dtw(a, b, la, lb, n_cep, c0, cepstra_in=(ca, cb))
    bound = mr.cost_bound(n_cep, la, lb, ref['stats'][0])
    err = abs(float(stats[0]) - ref['stats'][0])
    print(f'{name} end to end: cost {stats[0]:.6g}, error {err:.3g}, bound {bound:.3g}')
    assert err <= bound, (name, err, bound)
    if name in mc.STABLE_PATHS:
        assert n == len(mr.mel_dtw(a, b, la, lb, n_cep, c0)['path']), name


def probe_all(eng, a, b, la=None, lb=None, **kw):
    return {w: eng.mel_dtw_probe(a, b, la, lb, what=w, **kw) for w in mr.STAGES}


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_every_stage_against_float64_of_the_stage_before(gpu_engine, name):
    a, b = mc.pair(name)
    kw = mc.settings(name)
    got = {w: v[0] for w, v in probe_all(gpu_engine, a, b, **kw).items()}
    stats, path = gpu_engine.mel_dtw(a, b, return_path=True, **kw)
    assert stats.shape == (3, 1) and path.shape == (1, len(a) + len(b) - 1, 2) and path.dtype == np.int32
    check_row(name, a, b, len(a), len(b), kw['n_cep'], kw['include_c0'], got, stats[:, 0], path[0])
    if mc.CASES[name][2] in ('identical', 'repeat'):                 # the closed forms: cost exactly 0 along the known path
        assert stats[0, 0] == 0 and stats[2, 0] == 0 and stats[1, 0] == len(b)
        r = len(b) // len(a)
        assert np.array_equal(path[0, :len(b)], np.stack([np.arange(len(b)) // r, np.arange(len(b))], axis=1))


@pytest.fixture(scope='module')
def ragged(gpu_engine):
    a, b, la, lb = mc.ragged_batch()
    stats, path = gpu_engine.mel_dtw(a, b, la, lb, return_path=True)
    return a, b, la, lb, stats, path


def test_ragged_batch_reads_nothing_behind_the_lengths(gpu_engine, ragged):
    a, b, la, lb, stats, path = ragged
    assert np.isnan(a).any() and np.isnan(b).any()
    got = probe_all(gpu_engine, a, b, la, lb)
    assert np.isfinite(stats).all() and all(np.isfinite(v).all() for v in got.values())
    for r, name in enumerate(mc.RAGGED):
        check_row(name, a[r], b[r], int(la[r]), int(lb[r]), 13, False, {w: v[r] for w, v in got.items()}, stats[:, r], path[r])


def test_a_row_alone_gives_the_bits_it_gives_in_the_batch(gpu_engine, ragged):
    a, b, la, lb, stats, path = ragged
    for r, name in enumerate(mc.RAGGED):
        x, y = mc.pair(name)
        s1, p1 = gpu_engine.mel_dtw(x, y, return_path=True)
        assert np.array_equal(s1[:, 0], stats[:, r]), name
        assert np.array_equal(p1[0], path[r, :p1.shape[1]]) and np.all(path[r, p1.shape[1]:] == -1), name
        for w in ('cepstra_a', 'cost'):
            one = gpu_engine.mel_dtw_probe(x, y, what=w)[0]
            inside = gpu_engine.mel_dtw_probe(a, b, la, lb, what=w)[r]
            assert np.array_equal(one, inside[:one.shape[0], :one.shape[1]]), (name, w)


def test_host_device_and_stream_calls_agree_to_the_bit(gpu_engine, ragged):
    import torch
    a, b, la, lb, stats, path = ragged
    ta, tb = torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()
    s_dev, p_dev = gpu_engine.mel_dtw(ta, tb, la, lb, return_path=True)
    assert s_dev.is_cuda and p_dev.is_cuda and p_dev.dtype == torch.int32
    assert np.array_equal(s_dev.cpu().numpy(), stats) and np.array_equal(p_dev.cpu().numpy(), path)
    stream = torch.cuda.Stream()
    s_str, p_str = gpu_engine.mel_dtw(ta, tb, la, lb, return_path=True, stream=stream)
    stream.synchronize()
    assert np.array_equal(s_str.cpu().numpy(), stats) and np.array_equal(p_str.cpu().numpy(), path)
    mixed = gpu_engine.mel_dtw(ta, b, la, lb)                        # one operand on the host: moved, and a tensor comes back
    assert mixed.is_cuda and np.array_equal(mixed.cpu().numpy(), stats)
    cost = gpu_engine.mel_dtw_probe(ta, tb, la, lb, what='cost')
    assert cost.is_cuda and np.array_equal(cost.cpu().numpy(), gpu_engine.mel_dtw_probe(a, b, la, lb, what='cost'))


def test_return_path_false_leaves_the_statistics_unchanged(gpu_engine, ragged):
    a, b, la, lb, stats, _ = ragged
    only = gpu_engine.mel_dtw(a, b, la, lb)
    assert isinstance(only, np.ndarray) and only.shape == (3, len(la)) and np.array_equal(only, stats)


def test_unaligned_mode_against_the_restatement(gpu_engine, ragged):
    a, b, la, lb, _, _ = ragged
    stats, path = gpu_engine.mel_dtw(a, b, la, lb, align=False, return_path=True)
    assert np.isfinite(stats).all()
    for r, name in enumerate(mc.RAGGED):
        n = int(min(la[r], lb[r]))
        ca = gpu_engine.mel_dtw_probe(a, b, la, lb, what='cepstra_a')[r, :la[r]].astype(np.float64)
        cb = gpu_engine.mel_dtw_probe(a, b, la, lb, what='cepstra_b')[r, :lb[r]].astype(np.float64)
        ref = mr.mel_dtw(a[r], b[r], la[r], lb[r], align=False, cepstra_in=(ca, cb))['stats']
        # every distance within (n_cep + 4) 2^-24 of itself, their float64 sum rounded once
        assert abs(float(stats[0, r]) - ref[0]) <= (13 + 4 + 1) * mr.EPS * ref[0], (name, stats[:, r], ref)
        assert stats[1, r] == n and abs(float(stats[2, r]) - mr.MCD_DB_FACTOR * float(stats[0, r]) / n) <= 2 * mr.EPS * ref[2]
        assert np.array_equal(path[r, :n], np.stack([np.arange(n)] * 2, axis=1)) and np.all(path[r, n:] == -1), name
    assert np.array_equal(gpu_engine.mel_dtw(a, b, la, lb, align=False), stats)
    x, y = mc.pair(mc.RAGGED[0])
    assert np.array_equal(gpu_engine.mel_dtw(x, y, align=False)[:, 0], stats[:, 0])


@pytest.mark.parametrize('name', mc.UNALIGNED)
def test_unaligned_mode_on_both_sides_of_its_block(gpu_engine, name):
    """The reduction kernel's 256 threads and its stride of 256 frames: diagonals of 1, 97, 256, 257, 512 and 513 frames."""
    a, b = mc.pair(name)
    n = min(len(a), len(b))
    stats, path = gpu_engine.mel_dtw(a, b, align=False, return_path=True)
    ca = gpu_engine.mel_dtw_probe(a, b, what='cepstra_a')[0].astype(np.float64)
    cb = gpu_engine.mel_dtw_probe(a, b, what='cepstra_b')[0].astype(np.float64)
    ref = mr.mel_dtw(a, b, align=False, cepstra_in=(ca, cb))['stats']
    err, bound = abs(float(stats[0, 0]) - ref[0]), (13 + 4 + 1) * mr.EPS * ref[0]
    print(f'{name} un-aligned: cost {stats[0, 0]:.6g}, error {err:.3g}, bound {bound:.3g}')
    assert err <= bound, (name, err, bound)                        # every distance within (n_cep + 4) 2^-24, the sum rounded once
    assert stats[1, 0] == n and abs(float(stats[2, 0]) - mr.MCD_DB_FACTOR * float(stats[0, 0]) / n) <= 2 * mr.EPS * ref[2]
    assert np.array_equal(path[0, :n], np.stack([np.arange(n)] * 2, axis=1)) and np.all(path[0, n:] == -1)
    # one frame more or less moves the cost by that frame's distance: no frame of the diagonal is skipped or counted twice
    if n > 1:
        less = gpu_engine.mel_dtw(a[:n - 1], b[:n - 1], align=False)
        last = mr.distance(ca[n - 1:n], cb[n - 1:n])[0, 0]
        assert abs((float(stats[0, 0]) - float(less[0, 0])) - last) <= 2 * bound + (13 + 4) * mr.EPS * last, name


def test_the_library_refuses_by_name(gpu_engine):
    from text_to_speech_amd import HipLibraryError
    a = np.zeros((1, 8193, 2), np.float32)
    with pytest.raises(HipLibraryError, match='mel_dtw: Ta = 8193, Tb = 1: above 8192 frames'):
        gpu_engine.mel_dtw(a, a[:, :1], n_cep=1)
    with pytest.raises(HipLibraryError, match=r'mel_dtw: B\*Ta\*Tb too large \(B = 1, Ta = 8192, Tb = 4097'):
        gpu_engine.mel_dtw(a[:, :8192], a[:, :4097], n_cep=1)
    thin = np.zeros((65, 8192, 2), np.float32)
    with pytest.raises(HipLibraryError, match=r'mel_dtw: B\*\(Ta\+Tb\) too large \(B = 65, Ta = 8192, Tb = 1: above 524288 frames'):
        gpu_engine.mel_dtw(thin, thin[:, :1], n_cep=1)


def test_evaluate_synthesis_is_its_parts_bit_for_bit(gpu_engine):
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2
    rt = HipRuntime('synthetic', engine=gpu_engine, seed=7)
    model = Tacotron2(rt, lang='en')
    texts = ['Hello there.', 'A somewhat longer sentence, this one.', 'Hi']
    rng = np.random.default_rng(11)
    mels = [mc.log_mel(rng, n) for n in (23, 41, 9)]
    res = model.evaluate_synthesis(list(zip(texts, mels)), batch_size=2, max_length=3.)
    assert res['names'] == ['mcd_dtw', 'path_len', 'frames', 'target_frames', 'frame_ratio', 'stopped']
    per = res['per_item']
    assert per.shape == (6, 3) and per.dtype == np.float32
    toks = [np.asarray(model.encode_text(model.clean_text(t), cleaned=True), np.int32) for t in texts]
    for rows in ([0, 1], [2]):                                       # two batches, unequal texts
        tok = np.zeros((len(rows), max(len(toks[i]) for i in rows)), np.int32)
        target = np.zeros((len(rows), max(len(mels[i]) for i in rows), 80), np.float32)
        for r, i in enumerate(rows):
            tok[r, :len(toks[i])], target[r, :len(mels[i])] = toks[i], mels[i]
        out = rt.tacotron2_infer(tok, max_length=3., deterministic=True, on_device=True)
        assert out.mel.is_cuda
        assert out.mel.shape[1] == int(np.float32(tok.shape[1]) * np.float32(3.))          # the batch's frame cap: 3 per token
        frames = out.lengths.cpu().numpy()
        assert frames.min() >= 1
        wanted = np.array([len(mels[i]) for i in rows], np.int32)
        stats = gpu_engine.mel_dtw(out.mel, target, frames, wanted).cpu().numpy()
        assert np.array_equal(per[0, rows], stats[2]) and np.array_equal(per[1, rows], stats[1])
        assert np.array_equal(per[2, rows], frames) and np.array_equal(per[3, rows], wanted)
        assert np.array_equal(per[4, rows], (frames / wanted).astype(np.float32))
        assert np.array_equal(per[5, rows], frames < out.mel.shape[1])
    assert np.isfinite(per).all() and np.all(per[0] > 0)
    for k, name in enumerate(res['names']):
        assert res['mean'][name] == pytest.approx(float(per[k].astype(np.float64).mean()), rel=1e-12)


def test_copy_synthesis_is_its_parts_bit_for_bit(gpu_engine):
    import torch
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.waveglow import WaveGlow
    rt = HipRuntime('synthetic', engine=gpu_engine, seed=7)
    mel = mc.log_mel(np.random.default_rng(12), 40)
    res = WaveGlow(rt).copy_synthesis([mel], seed=5)
    assert res['names'] == ['mcd', 'frames'] and res['per_item'].shape == (2, 1)
    dev = torch.as_tensor(mel).cuda()[None]
    audio = rt.waveglow_infer(dev, seed=5)
    again = gpu_engine.mel_stft(audio)
    assert audio.is_cuda and tuple(again.shape) == (1, 41, 80)
    stats = gpu_engine.mel_dtw(dev, again, align=False).cpu().numpy()
    assert np.array_equal(res['per_item'][:, 0], [stats[2, 0], stats[1, 0]]) and stats[1, 0] == 40
    assert np.isfinite(stats).all() and res['mean'] == {'mcd': float(stats[2, 0]), 'frames': 40.0}
