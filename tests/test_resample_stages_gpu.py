"""GPU: FFT resampling (csrc/resample.hip) pass by pass against float64 -- the FFT of the chains alone through
tts_hip_resample_fft_probe at every length 2^6 .. 2^25 in both directions, the forward spectrum through
tts_hip_resample_probe, and the samples end to end -- on the cases of tests/resample_cases.py; then the grouping of ragged
batches and the equal-rate copy path.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import resample_cases as C
import resample_ref

pytestmark = pytest.mark.gpu


# ---- the FFT of the chains ---------------------------------------------------------------------------------------------
def _index_at(logL, positions, stored):
    """The bin (sample) that stands at `positions` of a line in stored (natural) order."""
    positions = np.asarray(positions, np.int64)
    if not stored or logL <= C.LOG_PMAX:
        return positions
    return (positions >> C.LOG_PMAX) + ((positions & (C.PMAX - 1)) << (logL - C.LOG_PMAX))


def _exp(logL, sign, e):
    """exp(sign * 2 pi i e / 2^logL) in complex128, the phase reduced in integers."""
    L = 1 << logL
    return np.exp(sign * 2j * np.pi * ((np.asarray(e, np.int64) & (L - 1)) / L))


def _tone(logL, sign, p, stored, out):
    """out[:] = exp(sign * 2 pi i p q / L) over the indices q of a line in stored / natural order.  Above 2^13 both orders
    are an outer product over the [L2][8192] grid: q = k2 + L2 * k1 (stored) or 8192 * n2 + n1 (natural)."""
    L = 1 << logL
    if logL <= C.LOG_PMAX:
        out[:] = _exp(logL, sign, p * np.arange(L, dtype=np.int64))
        return
    L2 = L >> C.LOG_PMAX
    slow, fast = np.arange(L2, dtype=np.int64), np.arange(C.PMAX, dtype=np.int64)
    if stored:
        slow, fast = slow, fast * L2
    else:
        slow, fast = slow * C.PMAX, fast
    np.multiply(_exp(logL, sign, p * slow)[:, None], _exp(logL, sign, p * fast)[None, :], out=out.reshape(L2, C.PMAX))


def _chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


@pytest.mark.parametrize('inverse', [False, True], ids=['forward', 'inverse'])
@pytest.mark.parametrize('logL', C.FFT_LOGS)
def test_fft_probe_impulses_tones_and_random_lines(gpu_engine, logL, inverse):
    """Forward: natural order in, stored order out, exponent -; inverse: stored order in, natural order out, exponent +,
    unscaled.  A unit impulse at p transforms to a unit-modulus exponential, a tone on p to L at p and 0 elsewhere."""
    L = 1 << logL
    sign = 1.0 if inverse else -1.0
    tag = f'fft 2^{logL} {"inverse" if inverse else "forward"}'
    full = logL <= C.FFT_FULL_CHECK_MAX_LOG
    if full:
        where = np.arange(L)
    else:       # every k2 for a few k1 and every k1 for a few k2 of the [L2][8192] grid
        grid = np.arange(L).reshape(L >> C.LOG_PMAX, C.PMAX)
        where = np.unique(np.concatenate([grid[:, k1] for k1 in (0, 1, 4095, 8191)] +
                                         [grid[k2] for k2 in (0, 1, (L >> C.LOG_PMAX) - 1)]))
    out_index = _index_at(logL, where, stored=not inverse)
    worst = {'impulse': 0.0, 'tone': 0.0, 'roundtrip': 0.0}
    for ci, group in enumerate(_chunks(C.fft_points(logL), C.fft_lines_per_call(logL))):
        # impulses: 1 at the position that holds index p
        x = np.zeros((len(group), L), np.complex64)
        for i, p in enumerate(group):
            x[i, C.stored_position(logL, p) if inverse else p] = 1.0
        got = gpu_engine.resample_fft_probe(x, inverse)
        for i, p in enumerate(group):
            worst['impulse'] = max(worst['impulse'], C.stage_error(got[i, where], _exp(logL, sign, p * out_index)))
        if full or ci == 0:     # the other direction on what came out: L at the same place, 0 elsewhere
            back = gpu_engine.resample_fft_probe(got, not inverse)
            for i in range(len(group)):
                worst['roundtrip'] = max(worst['roundtrip'], float(np.abs(back[i] - L * x[i]).max()) / L)
            del back
        # tones: the conjugate exponential on index p over the input positions
        for i, p in enumerate(group):
            _tone(logL, -sign, p, stored=inverse, out=x[i])
        got = gpu_engine.resample_fft_probe(x, inverse)
        for i, p in enumerate(group):
            pos = p if inverse else C.stored_position(logL, p)
            peak = complex(got[i, pos])
            got[i, pos] = 0
            worst['tone'] = max(worst['tone'], abs(peak - L) / L, float(np.abs(got[i]).max()) / L)
        del x, got
    if full:                    # random lines against np.fft in complex128, and their round trip
        rng = np.random.default_rng(900 + logL)
        x = (rng.standard_normal((2, L)) + 1j * rng.standard_normal((2, L))).astype(np.complex64)
        idx = C.stored_index(logL)
        nat = x.astype(np.complex128)
        if inverse:
            nat[:, idx] = x     # the lines came in stored order
        F = np.fft.ifft(nat, axis=1) * L if inverse else np.fft.fft(nat, axis=1)[:, idx]
        got = gpu_engine.resample_fft_probe(x, inverse)
        worst['random'] = C.stage_error(got, F)
        back = gpu_engine.resample_fft_probe(got, not inverse)
        worst['roundtrip'] = max(worst['roundtrip'], C.stage_error(back, L * x.astype(np.complex128)))
    print(f'{tag}, passes {[tuple(p) for p in C.passes(logL)]}: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= C.BOUNDS['roundtrip' if k == 'roundtrip' else 'fft'], (tag, k, v)


def test_fft_probe_refusals_write_nothing(gpu_engine):
    from text_to_speech_amd import _lib
    lib, h = _lib.load_library(), gpu_engine._h
    x = np.ones((2, 64, 2), np.float32)
    out = np.full((2, 64, 2), 5.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for args in ((p(x), 2, 5, 0, p(out)), (p(x), 2, 26, 0, p(out)), (p(x), 0, 6, 0, p(out)), (p(x), -1, 6, 1, p(out)),
                 (p(x), 8, 25, 0, p(out)), (p(x), 1 << 22, 6, 0, p(out)), (None, 2, 6, 0, p(out)), (p(x), 2, 6, 0, None)):
        assert lib.tts_hip_resample_fft_probe(h, *args) == -1, args[1:4]
        assert b'resample_fft_probe' in lib.tts_hip_last_error(h)
        assert (out == 5.0).all()
    assert lib.tts_hip_resample_fft_probe(h, p(x), 2, 6, 0, p(out)) == 0
    assert np.array_equal(out[:, 0], [[64, 64], [64, 64]]) and not out[:, 1:].any()      # 64 points of 1 + 1i


# ---- the forward spectrum and the samples, case by case --------------------------------------------------------------------
@pytest.mark.parametrize('name', [c.name for c in C.CASES])
def test_spectrum_and_samples_against_float64(gpu_engine, name):
    c = C.BY_NAME[name]
    a = C.case_inputs(name)
    X, y = C.case_reference(name)
    S = gpu_engine.resample_probe(a, c.rate, c.target)
    out = gpu_engine.resample(a, c.rate, c.target)
    assert S.shape == X.shape and out.shape == y.shape and out.dtype == np.float32
    checks = []
    for i, kind in enumerate(c.inputs):
        es, ey = C.stage_error(S[i], X[i]), C.stage_error(out[i], y[i])
        line = f'{name} (L_fwd 2^{c.logs[0]}, L_inv 2^{c.logs[1]}) {kind}: spectrum {es:.2e}, samples {ey:.2e}'
        checks += [(es, 'spectrum', kind), (ey, 'resample', kind)]
        n0 = C.impulse_at(kind, c.N)
        if n0 is not None:                          # the closed forms: unit-modulus bins, the periodic sinc
            cs = C.stage_error(S[i], C.impulse_spectrum(c.N, n0))
            cy = C.stage_error(out[i], C.impulse_resampled(c.N, c.M, n0))
            line += f'; against the closed forms {cs:.2e}, {cy:.2e}'
            checks += [(cs, 'spectrum', kind + ' closed form'), (cy, 'resample', kind + ' closed form')]
        print(line)
    for err, stage, what in checks:
        assert err <= C.BOUNDS[stage], (name, what, stage, err)


# ---- groups ------------------------------------------------------------------------------------------------------------
def _ragged_call(eng, r):
    a = C.ragged_batch(r)
    return a, eng.resample(a, r.rate, r.target, lengths=list(r.lens)), eng.resample_probe(a, r.rate, r.target, lengths=list(r.lens))


@pytest.mark.parametrize('name', ['groups_down', 'groups_up', 'one_sample_out'])
def test_groups_equal_their_one_row_calls_bitwise(gpu_engine, name):
    r = C.RAGGED_BY_NAME[name]
    a, out, S = _ragged_call(gpu_engine, r)
    N, M = a.shape[1], resample_ref.resampled_length(a.shape[1], r.rate, r.target)
    assert out.shape == (len(r.lens), M) and S.shape == (len(r.lens), N // 2 + 1)
    worst = [0.0, 0.0]
    for b, (n, m) in enumerate(zip(r.lens, r.mlens)):
        one = gpu_engine.resample(a[b, :n], r.rate, r.target)
        assert one.shape == (m,) and np.array_equal(out[b, :m], one), b
        assert not out[b, m:].any(), b                              # zeros, not NaN, beyond M_b
        one_s = gpu_engine.resample_probe(a[b, :n], r.rate, r.target)
        assert one_s.shape == (1, n // 2 + 1) and np.array_equal(S[b, :n // 2 + 1], one_s[0]), b
        assert not S[b, n // 2 + 1:].any(), b
        x64 = a[b, :n].astype(np.float64)
        worst[0] = max(worst[0], C.stage_error(S[b, :n // 2 + 1], np.fft.rfft(x64)))
        worst[1] = max(worst[1], C.stage_error(out[b, :m], resample_ref.resample(x64, m)))
    print(f'{name}: groups {[(g.logf, g.logi, g.rows) for g in C.groups(r.lens, r.mlens)]}: spectrum {worst[0]:.2e}, '
          f'samples {worst[1]:.2e}')
    assert worst[0] <= C.BOUNDS['spectrum'] and worst[1] <= C.BOUNDS['resample']


def test_workspace_grows_and_is_reused_bitwise(gpu_engine):
    small, large = C.RAGGED_BY_NAME['small'], C.RAGGED_BY_NAME['groups_up']
    first = [_ragged_call(gpu_engine, r)[1:] for r in (small, large)]
    again = [_ragged_call(gpu_engine, r)[1:] for r in (small, large, small)]
    for (out, S), (out0, S0) in zip(again, first + first[:1]):
        assert np.array_equal(out, out0) and np.array_equal(S, S0)
        assert np.isfinite(out).all() and np.isfinite(S.view(np.float32)).all()


def test_probe_refusals_write_nothing(gpu_engine):
    from text_to_speech_amd import _lib
    lib, h = _lib.load_library(), gpu_engine._h
    x = np.ones((2, 1000), np.float32)
    out = np.full((2, 501, 2), 5.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad = np.array([1000, 1001], np.int32)
    for args in ((p(x), 2, 1000, None, 2, 1, p(out), 499, 0), (p(x), 2, 1000, p(bad), 2, 1, p(out), 500, 0),
                 (p(x), 2, 1000, None, 0, 1, p(out), 500, 0), (p(x), 2, 1000, None, 7, 7, p(out), 1000, 0),
                 (p(x), 2, 1000, None, 2, 1, p(out), 500, 3)):
        assert lib.tts_hip_resample_probe(h, *args) == -1, args[1:]
        assert b'resample_probe' in lib.tts_hip_last_error(h)
        assert (out == 5.0).all()


# ---- equal rates: copies only ------------------------------------------------------------------------------------------
def test_equal_rates_copy_ragged_rows(gpu_engine):
    torch = pytest.importorskip('torch')
    lens = [1, 5000, 37, 4999, 5000, 2]
    rng = np.random.default_rng(5)
    a = np.full((len(lens), 5000), np.nan, np.float32)
    for b, n in enumerate(lens):
        a[b, :n] = rng.standard_normal(n)
    want = np.nan_to_num(a, nan=0.0)
    host = gpu_engine.resample(a, 22050, 22050, lengths=lens)
    assert host.dtype == np.float32 and np.array_equal(host, want)
    dev = torch.as_tensor(a, device=f'cuda:{gpu_engine.device}')
    got = gpu_engine.resample(dev, 22050, 22050, lengths=lens)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    s = torch.cuda.Stream(device=dev.device)
    got2 = gpu_engine.resample(dev, 22050, 22050, lengths=lens, stream=s)
    s.synchronize()
    assert np.array_equal(got2.cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), a, equal_nan=True)      # the input is left alone
