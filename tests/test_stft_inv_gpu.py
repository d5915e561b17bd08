"""GPU: the STFT with phase, its inverse and Griffin-Lim (csrc/stft_inv.hip) against the float64 restatement of
tests/stft_inv_ref.py, stage by stage (`HipEngine.griffin_lim_probe`) and end to end; bounds from tests/stft_inv_cases.py."""
import ctypes

import numpy as np
import pytest

import denoise_ref as D
import stft_inv_cases as C
import stft_inv_ref as R

pytestmark = pytest.mark.gpu


def _stft(eng, g):
    from text_to_speech_amd.stft import STFT
    return STFT(filter_length=g.fl, hop_length=g.hop, win_length=g.wl, engine=eng)


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize('name', C.NAMES)
def test_transform(gpu_engine, name):
    """Real / imaginary planes and the magnitude bit-equal to the mel plan's probes; the phase against float64 arctan2 of the
    run's own real / imaginary parts."""
    case = C.BY_NAME[name]
    g, x = case.geom, C.audio_of(case)
    fn = _stft(gpu_engine, g)
    plan = fn._plan()
    re, im = gpu_engine.stft_transform(plan, x, polar=False)
    mag, ph = gpu_engine.stft_transform(plan, x, polar=True)
    spec = gpu_engine.mel_fn_probe(plan, x, 'spectrum')
    assert re.shape == (1, case.F, g.cut)
    assert _bits(re, spec[..., :g.cut]) and _bits(im, spec[..., g.cut:])
    assert _bits(mag, gpu_engine.mel_fn_probe(plan, x, 'magnitude'))
    want = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    m = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2)
    if case.signal in ('tone', 'full'):
        keep = m >= C.PHASE_FLOOR * m.max(axis=-1, keepdims=True)
        assert 1.0 - keep.mean() <= C.PHASE_LEFT_OUT
    else:
        ref = R.transform(x, g)
        keep = (np.abs(ref[..., :g.cut]) + np.abs(ref[..., g.cut:]) > 0) & (m >= C.PHASE_FLOOR * m.max(axis=-1, keepdims=True))
    d = np.abs(ph.astype(np.float64) - want)
    d = np.minimum(d, 2 * np.pi - d)
    err = float(d[keep].max()) if keep.any() else 0.0
    print(name, f'phase {err:.3e} over {keep.mean():.0%} of the bins')
    assert np.isfinite(ph).all() and err <= C.PHASE_BOUND
    # the object: to_magnitude=False stacks the parts
    from text_to_speech_amd.stft import STFT
    stacked, ph2 = STFT(g.fl, g.hop, g.wl, to_magnitude=False, engine=gpu_engine).transform(x)
    assert stacked.shape == (1, case.F, g.cut, 2) and _bits(stacked[..., 0], re) and _bits(stacked[..., 1], im) and _bits(ph2, ph)
    assert _bits(fn(x[0]), mag)


@pytest.mark.parametrize('name', C.NAMES)
def test_inverse_and_round_trip(gpu_engine, name):
    case = C.BY_NAME[name]
    g, x = case.geom, C.audio_of(case)
    fn = _stft(gpu_engine, g)
    plan = fn._plan()
    re, im = gpu_engine.stft_transform(plan, x, polar=False)
    mag, ph = gpu_engine.stft_transform(plan, x, polar=True)
    spec64 = np.concatenate([re, im], -1).astype(np.float64)
    want = R.inverse(spec64, g)
    got = gpu_engine.stft_inverse(plan, re, im, polar=False)
    assert got.shape == (1, case.F * g.hop) and gpu_engine.mel_fn_samples(plan, case.F) == case.n
    e_inv = R.row_error(got, want)
    polar64 = np.concatenate([mag * np.cos(ph.astype(np.float64)), mag * np.sin(ph.astype(np.float64))], -1)
    got_p = gpu_engine.stft_inverse(plan, mag, ph, polar=True)
    e_pol = R.row_error(got_p, R.inverse(polar64, g))
    e_rt = R.row_error(got[:, :case.n], x)
    print(name, f'inverse {e_inv:.3e} polar {e_pol:.3e} round trip {e_rt:.3e}')
    assert (got[:, case.n:] == 0).all()
    assert e_inv <= C.BOUNDS['inverse'] and e_pol <= C.BOUNDS['inverse'] and e_rt <= C.BOUNDS['roundtrip']
    assert _bits(fn.inverse(np.stack([re, im], -1)), got) and _bits(fn.inverse(mag, ph), got_p)


@pytest.mark.parametrize('g,F', [(R.GEOMS[0], 8), (R.GEOMS[1], 9), (R.GEOMS[2], 12), (R.GEOMS[3], 65)])
def test_ragged_rows_equal_single_rows(gpu_engine, g, F):
    """Five rows of {1, 2, F / 2, F - 1, F} frames, NaN behind each row's frames: every row bit-equal to the row alone."""
    plan = _stft(gpu_engine, g)._plan()
    frames = [1, 2, F // 2, F - 1, F]
    rng = np.random.default_rng(F)
    re = rng.standard_normal((5, F, g.cut)).astype(np.float32)
    im = rng.standard_normal((5, F, g.cut)).astype(np.float32)
    for b, Fb in enumerate(frames):
        re[b, Fb:] = np.nan
        im[b, Fb:] = np.nan
    got = gpu_engine.stft_inverse(plan, re, im, frames=frames, polar=False)
    assert np.isfinite(got).all()
    for b, Fb in enumerate(frames):
        alone = gpu_engine.stft_inverse(plan, re[b:b + 1, :Fb], im[b:b + 1, :Fb], polar=False)
        S = g.samples(Fb)
        assert _bits(got[b, :S], alone[0, :S]) and (got[b, S:] == 0).all(), (b, Fb)
        want = R.inverse(np.concatenate([re[b:b + 1, :Fb], im[b:b + 1, :Fb]], -1).astype(np.float64), g)
        assert S == 0 or R.row_error(alone[:, :S], want[:, :S]) <= C.BOUNDS['inverse']


@pytest.mark.parametrize('with_init', [False, True], ids=['zero_phase', 'init'])
@pytest.mark.parametrize('momentum', C.MOMENTA)
@pytest.mark.parametrize('name', C.NAMES)
def test_loop_stage_by_stage(gpu_engine, name, momentum, with_init):
    case = C.BY_NAME[name]
    plan = _stft(gpu_engine, case.geom)._plan()
    S = C.target_of(name)
    init = C.init_of(name) if with_init else None
    cache = {}

    def runner(what, k):
        if (what, k) not in cache:
            cache[(what, k)] = gpu_engine.griffin_lim_probe(plan, S, k, what, n_iters=C.N_ITERS, momentum=momentum, init=init)
        return cache[(what, k)]

    assert _bits(runner('target', 0), S)
    errs = C.stage_errors(name, momentum, init, runner)
    print(name, momentum, with_init, ' '.join(f'{s} {e:.3e}' for s, e in errs.items()))
    for s, e in errs.items():
        assert e <= C.BOUNDS[s], (s, e)
    # a repeat gives the same bits, and the call itself ends where the probe's last signal does
    again = gpu_engine.griffin_lim_probe(plan, S, C.N_ITERS, 'signal', n_iters=C.N_ITERS, momentum=momentum, init=init)
    assert _bits(again, runner('signal', C.N_ITERS))
    audio = gpu_engine.griffin_lim(plan, S, n_iters=C.N_ITERS, momentum=momentum, init=init)
    g = case.geom
    assert _bits(audio[:, :case.n], again[:, g.half:g.half + case.n]) and (audio[:, case.n:] == 0).all()


# ---- the second table: plans whose frames leave samples uncovered, and a filter above 1024 -----------------------------------
@pytest.mark.parametrize('name', C.EXTRA_NAMES)
def test_inverse_on_the_extra_geometries(gpu_engine, name):
    """test_inverse_and_round_trip's comparisons under EXTRA_BOUNDS.  Where no window covers a sample (gapped, sparse) there is
    no round trip: those samples are exactly 0 and the covered ones follow the float64 inverse."""
    case = C.case_of(name)
    g, x, bounds = case.geom, C.audio_of(case), C.EXTRA_BOUNDS[C.geom_name(name)]
    fn = _stft(gpu_engine, g)
    plan = fn._plan()
    re, im = gpu_engine.stft_transform(plan, x, polar=False)
    mag, ph = gpu_engine.stft_transform(plan, x, polar=True)
    assert re.shape == (1, case.F, g.cut) and np.isfinite(ph).all()
    spec64 = np.concatenate([re, im], -1).astype(np.float64)
    e_spec = R.frame_error(spec64, R.transform(x, g), g)
    got = gpu_engine.stft_inverse(plan, re, im, polar=False)
    assert got.shape == (1, case.F * g.hop) and gpu_engine.mel_fn_samples(plan, case.F) == case.n
    polar64 = np.concatenate([mag * np.cos(ph.astype(np.float64)), mag * np.sin(ph.astype(np.float64))], -1)
    got_p = gpu_engine.stft_inverse(plan, mag, ph, polar=True)
    bare = C.uncovered(g, case.F)
    covered = lambda a: np.asarray(a)[:, :case.n][:, ~bare]
    e_inv = R.row_error(covered(got), covered(R.inverse(spec64, g)))
    e_pol = R.row_error(covered(got_p), covered(R.inverse(polar64, g)))
    e_rt = R.row_error(got[:, :case.n], x) if 'roundtrip' in bounds else None
    print(name, f'spectrum {e_spec:.3e} inverse {e_inv:.3e} polar {e_pol:.3e} round trip {e_rt} uncovered {int(bare.sum())}')
    assert np.isfinite(got).all() and np.isfinite(got_p).all()
    assert (got[:, case.n:] == 0).all() and (got_p[:, case.n:] == 0).all()
    assert (got[0, :case.n][bare] == 0).all() and (got_p[0, :case.n][bare] == 0).all()
    assert bare.any() == ('roundtrip' not in bounds)
    assert e_spec <= bounds['spectrum'] and e_inv <= bounds['inverse'] and e_pol <= bounds['inverse']
    assert e_rt is None or e_rt <= bounds['roundtrip']
    assert _bits(fn.inverse(np.stack([re, im], -1)), got) and _bits(fn.inverse(mag, ph), got_p)


@pytest.mark.parametrize('name', C.EXTRA_NAMES)
def test_loop_stage_by_stage_on_the_extra_geometries(gpu_engine, name):
    """test_loop_stage_by_stage at momentum 0.99 with `init`, under EXTRA_BOUNDS; the probed signal is exactly 0 at every
    sample no window covers, its reflected copies included."""
    case = C.case_of(name)
    g, bounds, momentum = case.geom, C.EXTRA_BOUNDS[C.geom_name(name)], 0.99
    plan = _stft(gpu_engine, g)._plan()
    S, init = C.target_of(name), C.init_of(name)
    cache = {}

    def runner(what, k):
        if (what, k) not in cache:
            cache[(what, k)] = gpu_engine.griffin_lim_probe(plan, S, k, what, n_iters=C.N_ITERS, momentum=momentum, init=init)
        return cache[(what, k)]

    assert _bits(runner('target', 0), S)
    errs = C.stage_errors(name, momentum, init, runner)
    print(name, momentum, ' '.join(f'{s} {e:.3e}' for s, e in errs.items()))
    for s, e in errs.items():
        assert e <= bounds[s], (s, e)
    bare = np.pad(C.uncovered(g, case.F), g.half, mode='reflect')
    for k in C.PROBE_KS:
        sig = runner('signal', k)
        assert sig.shape == (1, bare.size) and np.isfinite(sig).all() and (sig[0, bare] == 0).all(), k
    audio = gpu_engine.griffin_lim(plan, S, n_iters=C.N_ITERS, momentum=momentum, init=init)
    last = runner('signal', C.N_ITERS)
    assert _bits(audio[:, :case.n], last[:, g.half:g.half + case.n]) and (audio[:, case.n:] == 0).all()


_ROWS_GEOMS = {'16_16_4': R.GEOMS[0], '64_48_10': R.GEOMS[2], '1024_1024_256': R.GEOMS[3], 'gapped': C.EXTRA_GEOMS['gapped'][0]}


@pytest.mark.parametrize('gname', sorted(_ROWS_GEOMS))
def test_transform_rows(gpu_engine, gname):
    """The transform on a batch and on ragged rows: five rows of N = 64 hops hold {1, win_length - 1, win_length, 63 hops - 1,
    N} samples, NaN behind them (65 frame slots a row: the batch crosses the GEMM's 64-row tile).  On gapped the plan refuses
    a row of max(L, win_length) <= filter_length // 2 = 8 samples, so its three short rows hold 9, 10 and 12."""
    from text_to_speech_amd._lib import HipLibraryError
    g = _ROWS_GEOMS[gname]
    eng, plan = gpu_engine, _stft(gpu_engine, g)._plan()
    N = g.hop * 64
    short = [1, g.wl - 1, g.wl]
    if gname == 'gapped':
        with pytest.raises(HipLibraryError, match='not more than filter_length // 2'):
            eng.stft_transform(plan, np.zeros((3, N), np.float32), lengths=short)
        short = [g.half + 1, g.half + 2, 3 * g.hop]
    lengths = short + [g.hop * 63 - 1, N]
    F = eng.mel_fn_frames(plan, N)
    assert F == g.frames(N) == 65
    rng = np.random.default_rng(g.fl + g.hop)
    clean = rng.uniform(-0.9, 0.9, (5, N)).astype(np.float32)
    x, x7 = clean.copy(), clean.copy()
    for b, L in enumerate(lengths):
        x[b, L:] = np.nan
        x7[b, L:] = 7.0
    worst = 0.0
    for polar in (False, True):
        p0, p1 = eng.stft_transform(plan, x, lengths=lengths, polar=polar)
        assert p0.shape == p1.shape == (5, F, g.cut) and np.isfinite(p0).all() and np.isfinite(p1).all()
        q0, q1 = eng.stft_transform(plan, x7, lengths=lengths, polar=polar)
        assert _bits(p0, q0) and _bits(p1, q1)
        for b, L in enumerate(lengths):
            Fb = eng.mel_fn_frames(plan, L)
            assert Fb == g.frames(L) and (p0[b, Fb:] == 0).all() and (p1[b, Fb:] == 0).all(), (b, L)
            a0, a1 = eng.stft_transform(plan, clean[b:b + 1, :L], polar=polar)
            assert a0.shape == (1, Fb, g.cut) and _bits(p0[b, :Fb], a0[0]) and _bits(p1[b, :Fb], a1[0]), (polar, b, L)
            if not polar:
                want = R.transform(D.padded_row(clean[b], L, g), g)
                err = R.frame_error(np.concatenate([p0[b:b + 1, :Fb], p1[b:b + 1, :Fb]], -1), want, g)
                worst = max(worst, err)
                assert err <= C.BOUNDS['spectrum'], (b, L, err)
        # no lengths: three rows in one call are three calls of one row
        b0, b1 = eng.stft_transform(plan, clean[:3], polar=polar)
        for b in range(3):
            a0, a1 = eng.stft_transform(plan, clean[b:b + 1], polar=polar)
            assert _bits(b0[b:b + 1], a0) and _bits(b1[b:b + 1], a1), (polar, b)
    print(gname, f'spectrum of the ragged rows {worst:.3e}')


@pytest.mark.parametrize('name', sorted(C.LOG_MEL_PLANS))
def test_log_mel_input_on_a_ragged_batch(gpu_engine, name):
    """Log-mel rows of {7, 12, 11} frames, NaN behind them, on plans of 8 (n_mel < 32), 32 (no K padding column) and 80
    channels: the target is 0 behind a row's frames and max(0, exp(mel) . Minv) inside them, under the plan's own inverse and
    a caller's; three iterations give finite audio, every row the bits of the row alone."""
    eng = gpu_engine
    g, mel, W, Minv = C.log_mel_rows(name)
    plan = eng.mel_fn(C.log_mel_config(name))
    frames, F = list(C.LOG_MEL_FRAMES), C.LOG_MEL_F
    own = eng.griffin_lim_probe(plan, mel, 0, 'target', frames=frames, kind='log_mel', n_iters=0)
    given = eng.griffin_lim_probe(plan, mel, 0, 'target', frames=frames, kind='log_mel', n_iters=0, mel_inverse=Minv)
    audio = eng.griffin_lim(plan, mel, frames=frames, kind='log_mel', n_iters=3)
    assert own.shape == (3, F, g.cut) and audio.shape == (3, F * g.hop) and np.isfinite(audio).all()
    for b, Fb in enumerate(frames):
        want = R.mel_target(mel[b:b + 1, :Fb], Minv)
        e_own, e_given = R.target_error(own[b:b + 1, :Fb], want), R.target_error(given[b:b + 1, :Fb], want)
        print(name, b, f'target {e_own:.3e} with the caller\'s inverse {e_given:.3e}')
        assert (own[b, Fb:] == 0).all() and (given[b, Fb:] == 0).all(), b
        assert e_own <= C.BOUNDS['target'] and e_given <= C.BOUNDS['target'], (b, e_own, e_given)
        n = g.samples(Fb)
        alone = eng.griffin_lim(plan, mel[b:b + 1, :Fb], kind='log_mel', n_iters=3)
        assert _bits(audio[b, :n], alone[0, :n]) and (audio[b, n:] == 0).all() and np.abs(audio[b, :n]).max() > 0, (b, Fb)


def test_phasor_at_the_ends_of_the_float_range(gpu_engine):
    """P(init) on FLT_MIN-sized, subnormal, 3e38-sized and mismatched pairs: with S = 1 the first operand is the phasor.  Every
    pair has an exact unit answer, so the bound is absolute and unweighted."""
    g = R.GEOMS[0]
    plan = _stft(gpu_engine, g)._plan()
    pairs = C.phasor_pairs()
    F = 9
    idx = np.arange(F * g.cut) % len(pairs)
    init = pairs[idx].reshape(1, F, g.cut, 2)
    S = np.ones((1, F, g.cut), np.float32)
    op = gpu_engine.griffin_lim_probe(plan, S, 0, 'operand', n_iters=0, init=init)
    assert op.shape == (1, F, 2 * g.cut) and np.isfinite(op).all()
    got_r, got_i = op[0, :, :g.cut].reshape(-1).astype(np.float64), op[0, :, g.cut:].reshape(-1).astype(np.float64)
    want_r, want_i = R.phasor(pairs[:, 0].astype(np.float64), pairs[:, 1].astype(np.float64))
    origin = (pairs == 0).all(axis=1)
    assert origin.sum() == 2 and (want_r[origin] == 1).all() and (want_i[origin] == 0).all()
    err = np.maximum(np.abs(got_r - want_r[idx]), np.abs(got_i - want_i[idx]))
    for j, (a, b) in enumerate(pairs):
        print(f'P({a:.3e}, {b:.3e}) = ({got_r[j]:.9g}, {got_i[j]:.9g}) error {err[idx == j].max():.3e}')
    assert err.max() <= C.BOUNDS['phasor'], err.max()
    assert np.abs(np.hypot(got_r, got_i) - 1).max() <= C.BOUNDS['phasor']
    assert (got_r[origin[idx]] == 1).all() and (got_i[origin[idx]] == 0).all()


@pytest.mark.parametrize('g,F', [(R.GEOMS[0], 10), (R.GEOMS[1], 9), (R.GEOMS[2], 12), (R.GEOMS[3], 65)])
def test_ragged_griffin_lim_rows_equal_single_rows(gpu_engine, g, F):
    """Rows of unequal frame counts inside F, NaN behind each row's frames: the padded overlap-add layout, the forward DFT over
    a short row's F frame slots and the phase update's own-frame mask give every row the bits of the row called alone, the
    probed operand of the last iteration is 0 behind a row's frames, and the float64 loop agrees."""
    plan = _stft(gpu_engine, g)._plan()
    frames = [F // 2 + 1, F, F - 1]
    rng = np.random.default_rng(40 + F)
    S = np.abs(rng.standard_normal((3, F, g.cut))).astype(np.float32)
    init = rng.standard_normal((3, F, g.cut, 2)).astype(np.float32)
    for b, Fb in enumerate(frames):
        S[b, Fb:] = np.nan
        init[b, Fb:] = np.nan
    kw = dict(n_iters=C.N_ITERS, momentum=0.99)
    got = gpu_engine.griffin_lim(plan, S, frames=frames, init=init, **kw)
    assert np.isfinite(got).all()
    op = gpu_engine.griffin_lim_probe(plan, S, C.N_ITERS, 'operand', frames=frames, init=init, **kw)
    for b, Fb in enumerate(frames):
        n = g.samples(Fb)
        alone = gpu_engine.griffin_lim(plan, S[b:b + 1, :Fb], init=init[b:b + 1, :Fb], **kw)
        assert _bits(got[b, :n], alone[0, :n]) and (got[b, n:] == 0).all(), (b, Fb)
        assert (op[b, Fb:] == 0).all() and np.abs(op[b, :Fb]).max() > 0
        # one iteration from the probed operand, in float64: the run's last inverse
        want = R.inverse(op[b:b + 1, :Fb].astype(np.float64), g)
        assert R.row_error(alone[:, :n], want[:, :n]) <= C.BOUNDS['inverse']


@pytest.mark.parametrize('name', C.E2E)
def test_end_to_end(gpu_engine, name):
    """32 iterations, momentum 0, against the float64 loop: within ten times the float32 numpy loop's own distance."""
    case = C.BY_NAME[name]
    g, S = case.geom, C.target_of(name)
    plan = _stft(gpu_engine, g)._plan()
    got = gpu_engine.griffin_lim(plan, S, n_iters=C.E2E_ITERS, momentum=0.0)
    want = R.griffin_lim(S, g, C.E2E_ITERS)
    err = R.row_error(got, want)
    inc, inc0 = R.inconsistency(got[:, :case.n], S, g), R.inconsistency(gpu_engine.griffin_lim(plan, S, n_iters=0)[:, :case.n], S, g)
    print(name, f'end to end {err:.3e} (bound {C.E2E_BOUNDS[name]:.1e}); inconsistency {inc0:.4f} -> {inc:.4f}')
    assert err <= C.E2E_BOUNDS[name]
    assert inc < inc0


def _default_mel(eng):
    from text_to_speech_amd.stft import TacotronSTFT
    return TacotronSTFT(engine=eng)


def test_log_mel_input(gpu_engine):
    """mel_to_audio(TacotronSTFT(audio)): the target against float64 max(0, exp(mel) . Minv); Griffin-Lim brings the
    re-analysed mel closer to the input mel than the zero-phase inverse does."""
    fn = _default_mel(gpu_engine)
    x, _, Minv = C.log_mel_case()
    mel = fn(x)
    plan = fn._plan()
    want = R.mel_target(mel, Minv)
    got = gpu_engine.griffin_lim_probe(plan, mel, 0, 'target', kind='log_mel', n_iters=0)
    err = R.target_error(got, want)
    print(f'target {err:.3e}')
    assert err <= C.BOUNDS['target']
    # a caller's own Minv takes the same path
    got2 = gpu_engine.griffin_lim_probe(plan, mel, 0, 'target', kind='log_mel', n_iters=0, mel_inverse=Minv)
    assert R.target_error(got2, want) <= C.BOUNDS['target']
    a0 = fn.mel_to_audio(mel, n_iters=0)
    a1 = fn.mel_to_audio(mel, n_iters=32, momentum=0.0)
    assert a1.shape == (1, 65 * 256) and np.isfinite(a1).all()
    d0, d1 = np.abs(fn(a0[:, :x.shape[1]]) - mel).mean(), np.abs(fn(a1[:, :x.shape[1]]) - mel).mean()
    print(f'mel distance {d0:.4f} -> {d1:.4f}')
    assert d1 < d0


def test_seeded_rows_do_not_depend_on_the_batch(gpu_engine):
    import torch
    from oracle import philox_ref
    from text_to_speech_amd.runtime import stream_key
    from text_to_speech_amd.stft import PHASE_STREAM, seeded_phase
    fn = _default_mel(gpu_engine)
    g = R.GEOMS[3]
    mels = torch.as_tensor(np.stack([fn(R.signal('tone', g.samples(12), g, seed=b)[None])[0] for b in range(5)])).cuda()
    streams = [(7, b) for b in range(5)]
    batch = fn.mel_to_audio(mels, n_iters=4, seed=11, streams=streams)
    alone = fn.mel_to_audio(mels[3:4], n_iters=4, seed=11, streams=streams[3:4])
    assert torch.equal(batch[3], alone[0]) and bool(torch.isfinite(batch).all())
    assert not torch.equal(batch[3], fn.mel_to_audio(mels[3:4], n_iters=4, seed=12, streams=streams[3:4])[0])
    # the initial phasors are the row stream's normals, normalised
    init = seeded_phase(gpu_engine, mels[3:4], g.cut, 11, streams[3:4]).cpu().numpy()
    key = stream_key(11, PHASE_STREAM, 7, 3)
    want = philox_ref.normal(init.size, key, 0).reshape(init.shape).astype(np.float64)
    assert np.abs(init - want).max() <= 1e-6
    ph = gpu_engine.griffin_lim_probe(fn._plan(), np.ones((1, 12, g.cut), np.float32), 0, 'operand', n_iters=0, init=init)
    n = np.sqrt(want[..., 0] ** 2 + want[..., 1] ** 2)
    assert np.abs(ph[..., :g.cut] - want[..., 0] / n).max() <= 1e-6 and np.abs(ph[..., g.cut:] - want[..., 1] / n).max() <= 1e-6


def test_refusals_through_the_real_symbols(gpu_engine):
    from text_to_speech_amd._lib import HipLibraryError
    g = R.GEOMS[0]
    eng = gpu_engine
    plan = _stft(eng, g)._plan()
    F = 9
    S = np.ones((1, F, g.cut), np.float32)
    lib, h = eng._lib, eng._h
    out = np.zeros((1, F * g.hop), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fr = lambda *v: p(np.asarray(v, np.int32))

    def gl(spec=p(S), B=1, F_=F, C=g.cut, frames=None, fn=plan.handle, kind=0, n_iters=1, momentum=0.5, audio=p(out), mem=0):
        rc = lib.tts_hip_griffin_lim(h, spec, B, F_, C, frames, fn, kind, None, None, n_iters, momentum, audio, mem)
        return rc, (lib.tts_hip_last_error(h) or b'').decode()

    whisper = eng.mel_fn(dict(kind='whisper', sampling_rate=16000, n_mel_channels=80, filter_length=400, hop_length=160,
                              win_length=400, mel_fmin=0.0, mel_fmax=8000.0))
    pre = eng.mel_fn(dict(sampling_rate=22050, n_mel_channels=1, filter_length=16, hop_length=4, win_length=16, mel_fmin=0.0,
                          mel_fmax=11025.0, pre_emph=0.97))
    norm = eng.mel_fn(dict(sampling_rate=22050, n_mel_channels=4, filter_length=16, hop_length=4, win_length=16, mel_fmin=0.0,
                           mel_fmax=11025.0, normalize_mode='per_feature'))
    table = [
        (dict(spec=None), 'NULL pointer'), (dict(audio=None), 'NULL pointer'), (dict(B=0), 'must be >= 1'),
        (dict(F_=0), 'must be >= 1'), (dict(frames=fr(0)), 'frames[0] = 0 outside'), (dict(frames=fr(F + 1)), 'outside [1, F'),
        (dict(C=g.cut + 1), "C = 10, but the plan's bins"), (dict(n_iters=-1), 'n_iters = -1 < 0'),
        (dict(momentum=1.0), 'momentum'), (dict(momentum=-0.1), 'momentum'), (dict(momentum=float('nan')), 'momentum'),
        (dict(fn=whisper.handle, C=201), 'Whisper'), (dict(fn=pre.handle), 'pre_emph'),
        (dict(fn=norm.handle, kind=1, C=4), 'not invertible'), (dict(frames=fr(3)), 'not more than filter_length // 2'),
        (dict(B=70000), 'too large'), (dict(fn=ctypes.c_void_p(0x1234)), 'not a plan of this handle'), (dict(mem=7), 'bad mem kind'),
        (dict(kind=2), 'input_kind'),
    ]
    for kw, word in table:
        rc, msg = gl(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    def refused(rc, word, who):
        msg = (lib.tts_hip_last_error(h) or b'').decode()
        assert rc == -1 and msg.startswith(who + ': ') and word in msg, (who, word, rc, msg)

    for k, what, word in ((4, 0, 'k = 4 outside [0, n_iters = 1]'), (-1, 0, 'k = -1 outside'), (0, 6, 'no stage 6 (0 .. 5)'),
                          (0, -1, 'no stage -1'), (1, 4, 'ends at its signal')):
        refused(lib.tts_hip_griffin_lim_probe(h, p(S), 1, F, g.cut, None, plan.handle, 0, None, None, 1, 0.5, k, what, p(out), 0),
                word, 'griffin_lim_probe')
    # the inverse and the transform
    inv = lambda *a: lib.tts_hip_stft_inverse(h, *a)
    refused(inv(p(S), 1, F, None, None, plan.handle, 1, p(out), 0), 'NULL pointer', 'stft_inverse')
    refused(inv(p(S), 1, F, p(S), fr(F + 1), plan.handle, 1, p(out), 0), 'frames[0] = 10 outside [1, F = 9]', 'stft_inverse')
    refused(inv(p(S), 1, F, p(S), None, whisper.handle, 1, p(out), 0), 'Whisper', 'stft_inverse')
    refused(inv(p(S), 1, F, p(S), None, plan.handle, 2, p(out), 0), 'form 2 not 0', 'stft_inverse')
    refused(inv(p(S), 1, F, p(S), None, plan.handle, 1, p(out), 5), 'bad mem kind 5', 'stft_inverse')
    refused(inv(p(S), 1, F, p(S), None, ctypes.c_void_p(0x1234), 1, p(out), 0), 'not a plan of this handle', 'stft_inverse')
    x = np.zeros((1, 400), np.float32)
    tr = lambda *a: lib.tts_hip_stft_transform(h, *a)
    refused(tr(p(x), 1, 400, None, whisper.handle, 0, p(out), p(out), 0), 'Whisper', 'stft_transform')
    refused(tr(p(x), 1, 400, None, plan.handle, 0, p(out), None, 0), 'bad argument', 'stft_transform')
    refused(tr(p(x), 1, 400, None, plan.handle, 2, p(out), p(out), 0), 'what 2 not 0', 'stft_transform')
    refused(tr(p(x), 1, 400, fr(401), plan.handle, 0, p(out), p(out), 0), 'lengths[0] = 401 outside', 'stft_transform')
    refused(tr(p(x), 1, 400, None, ctypes.c_void_p(0x1234), 0, p(out), p(out), 0), 'not a plan of this handle', 'stft_transform')
    # an empty mel channel: the Cholesky inverse does not exist
    empty = eng.mel_fn(dict(sampling_rate=22050, n_mel_channels=128, filter_length=64, hop_length=16, win_length=64, mel_fmin=0.0,
                            mel_fmax=8000.0))
    with pytest.raises(HipLibraryError, match='minimum-norm inverse'):
        eng.griffin_lim(empty, np.zeros((1, 9, 128), np.float32), kind='log_mel', n_iters=1)
    # a good call on the same handle still succeeds
    rc, msg = gl()
    assert rc == 0, msg
    assert np.isfinite(out).all() and np.abs(out).max() > 0


def test_vocoder_path(gpu_engine, taco_weights, tmp_path):
    """Tacotron2.infer(text, vocoder=GriffinLim(engine)) on the synthetic small model: finite audio of frames * 256 samples per
    part; tts(..., vocoder='griffin_lim') the same from a weight file that holds no WaveGlow tensor."""
    from text_to_speech_amd import weights
    from text_to_speech_amd.griffin_lim import GriffinLim
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2, tts
    model = Tacotron2(HipRuntime('t', model='tacotron2', engine=gpu_engine, seed=0))
    voc = GriffinLim(gpu_engine, n_iters=4)
    assert voc.infer.__func__ is GriffinLim.__call__ and voc.compiled_infer.engine is gpu_engine
    res = tts('Hello there. General test!', model=model, vocoder=voc, max_length=6., max_text_length=-2, save=False)
    frames = [m.shape[0] for m in res['mel']]
    assert frames == [6 * 13, 6 * 13]
    assert res['audio'].shape == (sum(frames) * 256,) and np.isfinite(res['audio']).all() and np.abs(res['audio']).max() > 0
    path = str(tmp_path / 'taco_only.ttsw')
    weights.save_ttsw(path, taco_weights)
    res2 = tts('Hello there. General test!', path=path, vocoder='griffin_lim', max_length=6., max_text_length=-2, save=False)
    assert res2['audio'].shape == (sum(frames) * 256,) and np.isfinite(res2['audio']).all()
