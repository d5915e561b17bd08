"""CPU: the reduce_noise case table (tests/reduce_noise_cases.py) -- its float64 stages are the restatement of audio_ref.py
and reproduce the golden, its float32 form passes the checks the GPU has to pass, it reaches every edge it names, and its
bounds still separate the planted errors they exist to catch.  The trim-convolution table (tests/trim_conv_cases.py) reaches
its edges and never decides on a coin toss."""
import os

import numpy as np
import pytest

import audio_ref
import reduce_noise_cases as C
import trim_conv_cases as T

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def test_float64_stages_are_the_restatement():
    """Row by row, `stages` in float64 gives what audio_ref.reduce_noise gives on the row alone.  audio_ref rounds the
    spectrum to complex64 and the threshold to float32, `stages` does not: 1e-6 of the row's peak covers that (measured
    <= 2e-7), and the renormalised rows agree likewise."""
    for name in ('noise_1_511_4410_20000', 'sine_1023_1024_1025_2047_2048', 'sine_4609_1500_20480_noise3000', 'lead3000_10000',
                 'burst_300_8000', 'noise_6000_tone3000', 'dc_5000_1025_6000_quiet3000', 'zero_row1_3000_2500_700', 'alt_3000'):
        audio, lens, noise, nl = C.inputs_of(C.BY_NAME[name])
        ref = C.reference(name)
        for b, L in enumerate(lens):
            want = audio_ref.reduce_noise(audio[b, :L], noise=None if noise is None else noise[b], noise_length=nl)
            peak = max(float(np.abs(want).max()), 1e-30)
            err = float(np.abs(ref['out'][b, :L] - want).max()) / peak
            assert err <= 1e-6, (name, b, err)
            assert not ref['out'][b, L:].any() and not ref['out_norm'][b, L:].any()
            nrm = audio_ref.normalize_audio(want)
            assert float(np.abs(ref['out_norm'][b, :L] - nrm).max()) <= 1e-6 * max(1.0, abs(want.mean()) / max(np.abs(want - want.mean()).max(), 1e-30)), (name, b)


def test_float64_stages_reproduce_the_golden():
    f = np.load(os.path.join(GOLDEN, 'audio_processing_fixture.npz'))
    rate, raw = audio_ref.read_wav(os.path.join(GOLDEN, 'audio_test_16k.wav'))
    x = audio_ref.normalize_audio(raw)
    s = C.stages(x[None], noise_len=int(0.2 * rate))
    err = float(np.abs(s['out_norm'][0] - f['reduce_noise']).max())
    print('float64 stages vs golden max-abs', err)
    assert err <= 1e-6


@pytest.mark.parametrize('name', C.NAMES)
def test_float32_form_passes_what_the_gpu_has_to_pass(name):
    """The float32 restatement in the GPU's place: every stage inside its bound, the tie frames zero, and at most 0.1 % of
    the valid cells within DB_TOL of their threshold (a condition on the case, not a measurement)."""
    inputs = C.inputs_of(C.BY_NAME[name])
    e = C.compare(inputs, C.stages(*inputs, dtype=np.float32))
    print(name, ' '.join(f'{k} {v:.3g}' for k, v in e.items()))
    assert C.failures(e) == []


def test_case_table_reaches_every_edge():
    assert len(C.CASES) == len(C.BY_NAME)
    assert all(c.N <= 20480 and c.B <= 5 for c in C.CASES)
    one_row = {c.lengths[0] for c in C.CASES if c.B == 1 and c.clip is None and c.signal == 'noise'}
    assert {1, 300, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4409, 4410, 4411, 20480} <= one_row
    in_batches = {L for c in C.CASES if c.B > 1 for L in c.lengths}
    assert {1, 300, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4409, 4410, 4411, 4608, 20000, 20480} <= in_batches
    assert (1, 511, 4410, 20000) in {c.lengths for c in C.CASES}
    for lo, hi in ((511, 512), (1023, 1024), (2047, 2048)):                      # every F_b step
        a, b = (C.geometry(1, L, None, None, C.CLIP).F[0] for L in (lo, hi))
        assert b == a + 1 and C.geometry(1, hi + 1, None, None, C.CLIP).F[0] == b
    assert {1, 511, 512, 3000, 4607, 4608} <= {c.clip_len for c in C.CASES if c.clip}
    nF = lambda nl: int(C.geometry(1, 5000, None, np.zeros((1, nl)), nl).nF[0])
    assert (nF(1), nF(511), nF(512), nF(3000), nF(4607), nF(4608)) == (1, 1, 2, 6, 9, 10)
    assert {4608, 4609} <= {c.lengths[0] for c in C.CASES if c.clip_len == 4608}
    assert {c.signal for c in C.CASES} == {'noise', 'sine', 'speech', 'zeros', 'zero_row1', 'lead3000', 'lead6000', 'burst', 'dc',
                                           'impulse', 'alt'}
    assert {c.clip for c in C.CASES} == {None, 'noise', 'tone', 'quiet'}
    for c in C.CASES:
        audio, lens, noise, nl = C.inputs_of(c)
        again = C.inputs_of(c)[0]
        assert audio.shape == (c.B, c.N) and np.array_equal(audio, again, equal_nan=True)
        for b, L in enumerate(lens):                                             # what lies past L_b is poison
            assert np.isfinite(audio[b, :L]).all()
            assert L == c.N or (np.isnan(audio[b, L:]).all() if b % 2 == 0 else np.abs(audio[b, L:]).max() > 1e28)
        g = C.geometry(c.B, c.N, lens, noise, nl)
        assert g.F.max() <= g.Fr and g.nF.max() <= g.Frn
    assert any(c.tail for c in C.CASES if c.B == 1)


def test_signals_do_what_they_are_for():
    """From the float64 stages: a clip that is partly silence, the burst and the tone clip put more than 30 % of the noise
    cells on the top_db floor; the short rows, the silent rows and the burst contain exact ties; the silent clip gives a
    threshold of -400 and gates nothing; a DC row reaches |mean| / m > 100 before renormalising."""
    def facts(name):
        inputs = C.inputs_of(C.BY_NAME[name])
        ref = C.reference(name)
        return ref, C.compare(inputs, ref, end_to_end=False), C.geometry(inputs[0].shape[0], inputs[0].shape[1], *inputs[1:])
    for name in ('lead3000_10000', 'burst_8000', 'noise_6000_tone3000'):
        assert facts(name)[1]['clamped_noise'] > 0.3, name
    for name in ('noise_1', 'noise_300', 'noise_511', 'noise_1_300_511_512_513', 'zeros_2048', 'zero_row1_3000_2500_700', 'burst_8000',
                 'burst_300_8000'):
        ref, e, g = facts(name)
        assert e['ties'] > 0 and e['mask'] == 0, name
        # the ties are exact in float64: dB == threshold in every tie cell of a row's own frames
        tie = C.tie_cells(g, ref['spectrum'], ref['noise_spectrum'], ref['power_max'])
        for b in range(g.B):
            db = C.db_of(ref['spectrum'][b, :g.F[b]], ref['power_max'][0][b])[0]
            assert (db == ref['threshold'][b][None])[tie[b, :g.F[b]]].all(), (name, b)
    assert facts('noise_512')[1]['ties'] == 0
    ref, e, g = facts('burst_8000')
    assert e['ties'] > 1000                                                     # not just a handful
    ref, e, g = facts('lead6000_12000')
    assert (ref['threshold'] == -400).all() and not ref['mask'].any()
    audio = C.inputs_of(C.BY_NAME['lead6000_12000'])[0]
    assert float(np.abs(ref['out'][0] - audio[0]).max()) <= 1e-12             # stft -> istft alone
    ref, e, g = facts('zeros_300_2048_5000')
    assert not ref['out'].any() and not ref['out_norm'].any() and not ref['mask'].any()
    assert facts('dc_5000_quiet3000')[1]['mean_over_m'] > 100
    assert facts('dc_5000_1025_6000_quiet3000')[1]['mean_over_m'] > 100


# per mutation, the cases it is looked for in
TEETH_CASES = {
    None: ('noise_20480', 'sine_4609_1500_20480_noise3000', 'lead3000_10000', 'burst_8000', 'noise_6000_tone3000', 'noise_511',
           'dc_5000_quiet3000', 'impulse_4096', 'speech_8000'),
    # more than one noise frame everywhere (the sample std of one frame is NaN, which any check catches)
    'ddof_1': ('noise_20480', 'sine_4609_1500_20480_noise3000', 'lead3000_10000', 'noise_6000_tone3000'),
}
TEETH_MARGIN = 3.0


@pytest.mark.parametrize('mutation', sorted(C.MUTATIONS))
def test_bounds_have_teeth(mutation):
    """Every planted error exceeds the bound of the first stage it touches by TEETH_MARGIN on at least one case (for the
    stages that count cells: at least TEETH_MARGIN cells), so a kernel wrong in that way fails the GPU comparison.  (The
    same cases pass unmutated: test_float32_form_passes_what_the_gpu_has_to_pass.)"""
    stage = C.MUTATIONS[mutation]
    errs = {}
    for name in TEETH_CASES.get(mutation, TEETH_CASES[None]):
        inputs = C.inputs_of(C.BY_NAME[name])
        errs[name] = C.compare(inputs, C.stages(*inputs, mutation=mutation), end_to_end=False)[stage]
    assert not any(np.isnan(v) for v in errs.values()), errs
    worst = max(errs, key=errs.get)
    print(f'{mutation}: {stage} error {errs[worst]:.3g} on {worst}; bound {C.BOUNDS[stage]:.3g}')
    assert errs[worst] >= TEETH_MARGIN * max(C.BOUNDS[stage], 1.0 if C.BOUNDS[stage] == 0 else 0.0), errs


# ---- trim convolution ----------------------------------------------------------------------------------------------------
def test_trim_table_reaches_every_edge():
    assert {c.wl for c in T.CASES} >= {4, 5, 1022, 1024, 1026, 2048, 4410, 4411}
    assert {c.W % 4 for c in T.CASES} == {0, 2}
    assert {c.W for c in T.CASES if c.W < T.TRIM_JC} and {c.W for c in T.CASES if c.W == T.TRIM_JC} and \
        {c.W for c in T.CASES if T.TRIM_JC < c.W <= 2 * T.TRIM_JC} and {c.W for c in T.CASES if c.W > 4 * T.TRIM_JC}
    for wl in (4, 5, 1022, 1024, 1026, 2048, 4410, 4411):
        c = T.BY_NAME[f'wl{wl}_mixed']
        assert {1, 2, 1023, 1024, 1025, 2049} <= {L - c.W + 1 for L in c.lengths if L >= c.W}      # around TRIM_OUT
        assert {c.W - 1, c.W, c.W + 1, 1} <= set(c.lengths)
        assert min(c.lengths) < c.W <= c.N                                                          # both kernels launch
    assert T.BY_NAME['wl1024_short_only'].N < 1024
    for c in T.CASES:
        a, lens = T.audio_of(c)
        for b, L in enumerate(lens):
            assert np.isfinite(a[b, :L]).all()
            assert L == c.N or (np.isnan(a[b, L:]).all() if b % 2 == 0 else np.abs(a[b, L:]).max() > 1e28)
            assert len(T.reference(c.name)[b]) == abs(L - c.W) + 1
    for wl in (4, 5, 1022, 1024, 1026, 2048, 4410, 4411):
        c = T.BY_NAME[f'wl{wl}_mixed']
        rows = [T.audio_of(c)[0][b, :L] for b, L in enumerate(c.lengths)]
        assert not rows[1].any() and (rows[0] == 1).any() and len(np.unique(rows[2])) > 2
        # the row that fills one block exactly and the row of one output carry data, and their convolutions are not zero
        for b in (2, 5):
            assert c.lengths[b] - c.W + 1 == (T.TRIM_OUT, 1)[b == 5] and len(np.unique(rows[b])) > 2
            assert (T.reference(c.name)[b] > 0).all(), (c.name, b)


def test_trim_thresholds_are_never_a_coin_toss():
    """No convolution value of any case lies within 1e-12 (relative) of either threshold, so the indices follow from the
    convolution alone, and audio_ref.trim_bounds on the reference convolution is audio_ref.trim_window."""
    for c in T.CASES:
        a, lens = T.audio_of(c)
        for b, L in enumerate(lens):
            conv = T.reference(c.name)[b]
            for th in T.thresholds(conv, c.wl):
                assert (np.abs(conv - th) > T.THRESHOLD_MARGIN * th).all(), (c.name, b)
            for mode in T.MODES:
                assert audio_ref.trim_bounds(conv, int(L), c.wl, mode=mode) == audio_ref.trim_window(a[b, :L], None, window_length=c.wl, mode=mode)
