"""CPU: the case table of the resampling stage tests (tests/resample_cases.py) reaches what it claims, its numpy restatements
of the passes agree with np.fft, the complex64 restatement of the chain stays within every case's bound, and every planted
mistake -- applied to those restatements -- exceeds ten times the bound of a named table case in the stage it belongs to."""
import numpy as np
import pytest

import resample_cases as C
import resample_ref


def test_tables_reach_every_transform_length():
    fft, logf, logi = C.reached()
    every = set(range(6, 26))
    assert fft == every and logf == every and logi == every
    # ... and with them every lds_fft configuration: one workgroup at logP 6 .. 13, the column pass at logP 1 .. 12 with
    # nl = 4096 .. 2 lines per workgroup, the row pass at logP 13
    configs = {(p.kind, p.logP, p.nl) for k in every for p in C.passes(k)}
    assert configs == ({('lds', k, 1) for k in range(6, 14)} | {('col', c, 8192 >> c) for c in range(1, 13)} | {('row', 13, 1)})
    for c in C.CASES:
        assert 1 <= c.N <= C.RS_MAX_LEN and 1 <= c.M <= C.RS_MAX_LEN
        assert resample_ref.resampled_length(c.N, c.rate, c.target) == c.M and c.rate != c.target
    assert C.BY_NAME['pow2_2e24_to_2e23'].N == C.RS_MAX_LEN


def test_lengths_are_the_smallest_that_reach_a_transform():
    for k in range(7, 26):
        n, m = C.smallest_n_for_fwd(k), C.smallest_m_for_inv(k)
        assert n + n // 2 > 1 << (k - 1) >= (n - 1) + (n - 1) // 2
        assert 2 * m - 1 > 1 << (k - 1) >= 2 * (m - 1) - 1
    for k in range(6, 23):
        c = C.BY_NAME[f'len_2e{k}']
        assert c.logs == (k, k) and (c.N, c.M) == (C.smallest_n_for_fwd(k), C.smallest_m_for_inv(k))
    for n, m in ((1, 1), (42, 32), (43, 33), (5461, 4096), (5462, 4097), (1 << 24, 1 << 24)):
        lf, li = resample_ref.bluestein_lengths(n, m)
        assert C.rs_lens(n, m) == (lf.bit_length() - 1, li.bit_length() - 1)


def test_ragged_cases_form_the_groups_they_are_meant_to():
    for name, down in (('groups_down', True), ('groups_up', False)):
        r = C.RAGGED_BY_NAME[name]
        gs = C.groups(r.lens, r.mlens)
        assert [b for g in gs for b in g.rows] != list(range(len(r.lens)))          # launch order is not batch order
        big = [g for g in gs if len(g.rows) >= 3]
        assert len(big) >= 2
        for g in big:
            assert all(b1 - b0 > 1 for b0, b1 in zip(g.rows, g.rows[1:]))               # non-adjacent
            assert len({r.lens[b] for b in g.rows}) == len(g.rows)                      # different N_b
            assert g.xstride == max(r.lens[b] for b in g.rows) // 2 + 1
        assert any(len(g.rows) >= 2 and max(g.logf, g.logi) > C.LOG_PMAX for g in gs)   # a four-step group of G >= 2
        assert all((g.logf > g.logi) == down for g in gs if min(g.logf, g.logi) > 6)    # (both are 64 for the shortest rows)
        assert len({g.xstride for g in gs}) == len(gs)
    one = C.RAGGED_BY_NAME['one_sample_out']
    assert sorted(one.mlens) == [1, 1, 1, 1, 500]


@pytest.mark.parametrize('logP', range(1, 14))
def test_lds_fft_restatement_is_a_dft(logP):
    rng = np.random.default_rng(logP)
    x = rng.standard_normal((3, 1 << logP)) + 1j * rng.standard_normal((3, 1 << logP))
    assert C.stage_error(C.lds_fft(x), np.fft.fft(x, axis=1)) < 1e-13
    assert C.stage_error(C.lds_fft(x, inverse=True), np.fft.ifft(x, axis=1) * (1 << logP)) < 1e-13


@pytest.mark.parametrize('logL', range(14, 19))
def test_four_step_restatement_and_stored_order(logL):
    L = 1 << logL
    rng = np.random.default_rng(logL)
    x = rng.standard_normal((2, L)) + 1j * rng.standard_normal((2, L))
    F = np.fft.fft(x, axis=1)
    idx = C.stored_index(logL)
    assert sorted(idx) == list(range(L))
    assert all(idx[C.stored_position(logL, k)] == k for k in (0, 1, 8191, 8192, 8193, L // 2, L - 1))
    assert C.stage_error(C.four_step(x), F[:, idx]) < 1e-13
    assert C.stage_error(C.four_step(F[:, idx], inverse=True), L * x) < 1e-13


def test_pass_restatements_agree_with_the_rule_set():
    for name in ('len_2e6', 'len_2e10', 'nyquist_down', 'nyquist_up', 'equal_length', 'down_even_even', 'up_even_odd'):
        c = C.BY_NAME[name]
        a = C.case_inputs(name)
        X, y = C.case_reference(name)
        for i in range(len(c.inputs)):
            assert C.stage_error(C.spectrum_by_passes(a[i]), X[i]) < 1e-12
            assert C.stage_error(C.resample_by_passes(a[i], c.M), y[i]) < 1e-12
    r = C.RAGGED_BY_NAME['groups_down']
    a = np.nan_to_num(C.ragged_batch(r))
    S = C.batch_spectra(a, r.lens, r.mlens)
    for b, n in enumerate(r.lens):
        assert np.array_equal(S[b, :n // 2 + 1], np.fft.rfft(a[b, :n].astype(np.float64))) and not S[b, n // 2 + 1:].any()


def test_closed_forms_of_the_impulse_rows():
    for n, m in ((1002, 334), (334, 1002), (1000, 500), (1000, 1501), (683, 257), (500, 500), (7, 3), (6, 16)):
        for n0 in (0, 1, n // 2, n - 1):
            x = np.zeros(n)
            x[n0] = 1.0
            assert C.stage_error(C.impulse_spectrum(n, n0), np.fft.rfft(x)) < 1e-12
            assert C.stage_error(C.impulse_resampled(n, m, n0), resample_ref.resample(x, m)) < 1e-11, (n, m, n0)


def _small_enough(c):
    return max(c.logs) <= 22


@pytest.mark.parametrize('name', [c.name for c in C.CASES if _small_enough(c)])
def test_complex64_restatement_within_the_bound(name):
    """d32, the deviation of the complex64 restatement (numpy rounds each whole FFT once): a floor under the GPU's error."""
    c = C.BY_NAME[name]
    a = C.case_inputs(name)
    _, y = C.case_reference(name)
    for i, kind in enumerate(c.inputs):
        d32 = C.stage_error(resample_ref.resample_bluestein(a[i], c.M), y[i])
        print(f'{name} {kind}: d32 {d32:.2e}')
        assert d32 <= C.BOUNDS['resample'], (name, kind)


# ---- planted mistakes --------------------------------------------------------------------------------------------------
def _fft_line(logL):
    rng = np.random.default_rng(100 + logL)
    L = 1 << logL
    return rng.standard_normal((1, L)) + 1j * rng.standard_normal((1, L))


def _fft_mistake(logL, inverse, mistake):
    x = _fft_line(logL)
    F = np.fft.fft(x, axis=1)
    idx = C.stored_index(logL)
    if mistake == 'stored_order_swapped':            # the helper that maps the probe's output to bins, not the passes
        return C.stage_error(F[:, C.stored_index(logL, swap=True)], C.four_step(x))
    if inverse:
        return C.stage_error(C.four_step(F[:, idx], True, mistake), x.shape[1] * x)
    return C.stage_error(C.four_step(x, False, mistake), F[:, idx])


def _row(case, kind):
    c = C.BY_NAME[case]
    i = c.inputs.index(kind)
    X, y = C.case_reference(case)
    return c, C.case_inputs(case)[i], X[i], y[i]


def _resample_mistake(case, kind, mistake):
    c, x, _, y = _row(case, kind)
    return C.stage_error(C.resample_by_passes(x, c.M, mistake), y)


def _spectrum_mistake(case, kind, **how):
    _, x, X, _ = _row(case, kind)
    return C.stage_error(C.spectrum_by_passes(x, **how), X)


def _group_mistake(mistake):
    r = C.RAGGED_BY_NAME['groups_down']
    a = np.nan_to_num(C.ragged_batch(r))
    good, bad = C.batch_spectra(a, r.lens, r.mlens), C.batch_spectra(a, r.lens, r.mlens, mistake)
    return max(C.stage_error(bad[b], good[b]) for b in range(len(r.lens)))


# name -> (stage whose bound it must exceed tenfold, the table case that catches it, its error there)
PLANTED = {
    'four-step twiddle exponent s * (j + 1)': ('fft', 'fft 2^14 forward', lambda: _fft_mistake(14, False, 'twiddle_j_plus_1')),
    'four-step twiddle exponent s * (j + 1), inverse': ('fft', 'fft 2^18 inverse', lambda: _fft_mistake(18, True, 'twiddle_j_plus_1')),
    'inverse twiddle not conjugated': ('fft', 'fft 2^14 inverse', lambda: _fft_mistake(14, True, 'inverse_twiddle_not_conjugated')),
    'k1 / k2 swapped in the stored order': ('fft', 'fft 2^14 forward', lambda: _fft_mistake(14, False, 'stored_order_swapped')),
    'radix-2 tail skipped, one workgroup': ('fft', 'fft 2^7 forward', lambda: _fft_mistake(7, False, 'skip_radix2_tail')),
    'radix-2 tail skipped, inverse': ('fft', 'fft 2^9 inverse', lambda: _fft_mistake(9, True, 'skip_radix2_tail')),
    'radix-2 tail skipped, column pass of logP 3': ('fft', 'fft 2^16 forward', lambda: _fft_mistake(16, False, 'skip_radix2_tail')),
    'Nyquist factor wrong, down': ('resample', 'nyquist_down', lambda: _resample_mistake('nyquist_down', 'nyquist', 'nyquist_factor_swapped')),
    'Nyquist factor wrong, up': ('resample', 'nyquist_up', lambda: _resample_mistake('nyquist_up', 'nyquist', 'nyquist_factor_swapped')),
    'Nyquist factor wrong, four-step': ('resample', 'nyquist_down_4step',
                                        lambda: _resample_mistake('nyquist_down_4step', 'nyquist', 'nyquist_factor_swapped')),
    'Nyquist factor applied when M == N': ('resample', 'equal_length',
                                           lambda: _resample_mistake('equal_length', 'nyquist', 'nyquist_at_equal_length')),
    'Hermitian mirror M - off - 1': ('resample', 'len_2e10', lambda: _resample_mistake('len_2e10', 'noise', 'mirror_off_by_one')),
    'Hermitian mirror M - off - 1, impulse': ('resample', 'down_even_even',
                                              lambda: _resample_mistake('down_even_even', 'impulse_last', 'mirror_off_by_one')),
    'L_fwd one power short': ('spectrum', 'len_2e10', lambda: _spectrum_mistake('len_2e10', 'impulse_last', lf_short=True)),
    'L_fwd one power short, noise': ('spectrum', 'len_2e12', lambda: _spectrum_mistake('len_2e12', 'noise', lf_short=True)),
    'chirp phase from an fp32 j * j': ('spectrum', 'len_2e16', lambda: _spectrum_mistake('len_2e16', 'impulse_last', fp32_square=True)),
    'chirp phase from an fp32 j * j, burst': ('spectrum', 'len_2e16', lambda: _spectrum_mistake('len_2e16', 'burst', fp32_square=True)),
    "a row reads its neighbour's N_b": ('spectrum', 'groups_down', lambda: _group_mistake('neighbour_length')),
    'xstride of the wrong group': ('spectrum', 'groups_down', lambda: _group_mistake('xstride_of_other_group')),
}


@pytest.mark.parametrize('name', list(PLANTED))
def test_planted_mistake_is_caught(name):
    stage, case, error = PLANTED[name]
    assert case.startswith('fft 2^') or case in C.BY_NAME or case in C.RAGGED_BY_NAME
    err = error()
    print(f'{name}: {err:.3e} in {case} against 10 x {C.BOUNDS[stage]:.1e} ({stage})')
    assert err > 10 * C.BOUNDS[stage]


def test_chirp_from_fp32_square_is_exact_up_to_4096():
    j = np.arange(4097)
    assert np.array_equal(C.chirp(j, 5000, fp32_square=True), C.chirp(j, 5000))
    assert not np.array_equal(C.chirp(np.arange(4097, 9000), 9001, fp32_square=True), C.chirp(np.arange(4097, 9000), 9001))


def test_imaginary_part_of_bin_m_half_cannot_show_in_the_output():
    """A finding, not a catch.  The kernel drops the imaginary part of bin M / 2 (M even) as numpy's irfft does, but the
    inverse chain ends in Re(w_j c_j): at k = M / 2 the DFT factor exp(-i pi j) is real, so that imaginary part only reaches
    the imaginary part of the result, which is never stored.  Keeping it changes no output sample beyond rounding (here:
    below 1e-14 of peak in float64 on every even-M case), so no end-to-end case can catch this mistake at any bound; bin 0
    is the same.  The line is redundant in the kernel rather than untested."""
    for case in ('down_even_even', 'nyquist_down', 'nyquist_down_4step', 'equal_length', 'nyquist_up'):
        c = C.BY_NAME[case]
        assert c.M % 2 == 0
        for i, kind in enumerate(c.inputs):
            x = C.case_inputs(case)[i]
            X = np.fft.rfft(x.astype(np.float64))
            if c.M < c.N and kind == 'noise':
                assert abs(X[c.M // 2].imag) > 1e-3                                     # there is something to keep
            good, kept = C.resample_by_passes(x, c.M), C.resample_by_passes(x, c.M, 'nyquist_imag_kept')
            assert C.stage_error(kept, good) < 1e-14
