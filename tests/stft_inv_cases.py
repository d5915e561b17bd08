"""Shared cases, stage comparisons and bounds of the STFT-inverse / Griffin-Lim tests (tests/test_stft_inv.py on the CPU,
test_stft_inv_gpu.py on an MI355X).

Every stage is compared with float64 applied to the SAME run's previous stage (`stage_errors`), so a stage's error is its
own.  `runner(what, k)` returns a probed stage; on the CPU it is the float32 numpy copy of the loop (`numpy_runner`), whose
distances from float64 the bounds come from: BOUNDS[stage] is ten times the worst float32 distance over CASES, rounded up to
two digits ('spectrum' reuses the mel-STFT bound of tests/mel_stft_cases.py, derived there by the same rule).
test_stft_inv.py asserts that every bound lies above the float32 distance and a factor ten below the weakest planted mistake
(stft_inv_ref.MISTAKES) at the stage that mistake first shows in.

A second table (EXTRA_GEOMS, EXTRA_CASES, EXTRA_BOUNDS) holds the plans the first leaves out -- frames that do not cover every
sample, a filter above 1024 -- under the same rule; LOG_MEL_PLANS and `phasor_pairs` feed the ragged log-mel and the
float-range tests.  CASES, NAMES, BOUNDS are as they were.
"""
import functools
from typing import NamedTuple

import numpy as np

import mel_fn_cases
import stft_inv_ref as R

N_ITERS = 3
PROBE_KS = (0, 1, N_ITERS - 1, N_ITERS)      # iteration n_iters ends at its signal: spectrum and phasor stop at n_iters - 1
MOMENTA = (0.0, 0.99)

# measured float32 numpy distances (test_stft_inv.py::test_bounds_lie_above_float32 and
# test_target_bound print and check them): frames 1.3e-7, signal 2.2e-7,
# spectrum 9.4e-7, phasor 1.1e-7, operand 1.3e-7, inverse 1.25e-6, roundtrip 1.43e-6, target 2.8e-7
BOUNDS = {
    'frames': 1.3e-6,
    'signal': 2.2e-6,
    'spectrum': 1.7e-5,         # tests/mel_stft_cases.py BOUNDS['spectrum']
    'phasor': 1.1e-6,
    'operand': 1.3e-6,
    'inverse': 1.3e-5,
    'roundtrip': 1.5e-5,
    'target': 2.8e-6,
}
PHASE_BOUND = 2e-6              # atan2f is within 2 ulps (HIP math API): 2 * 2^-23 * pi = 7.5e-7 at +-pi, doubled
PHASE_FLOOR = 1e-4              # bins below this fraction of the frame's largest magnitude are left out of the phase check
PHASE_LEFT_OUT = 0.20           # ... which may leave out at most this share of the bins on the tone cases


class Case(NamedTuple):
    name: str
    geom: R.Geom
    F: int
    signal: str

    @property
    def n(self):
        return self.geom.samples(self.F)


def _cases():
    out = []
    for g, Fs in ((R.GEOMS[0], (9,)), (R.GEOMS[1], (9,)), (R.GEOMS[2], (13,)), (R.GEOMS[3], (63, 64, 65))):
        for F in Fs:
            for sig in ('tone', 'impulse', 'silence', 'full'):
                if g.fl == 1024 and F != 65 and sig != 'tone':
                    continue                    # the tile edge needs one signal; every signal runs at F = 65
                out.append(Case(f'{g.fl}_{g.wl}_{g.hop}_f{F}_{sig}', g, F, sig))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)
E2E = ('64_48_10_f13_tone', '1024_1024_256_f65_tone')       # (64, 48, 10) and (1024, 1024, 256) at F = 65
E2E_ITERS = 32
# ten times the distance of the float32 numpy loop from the float64 one after E2E_ITERS iterations at momentum 0, as
# stft_inv_ref.row_error (measured 5.7e-7 and 1.96e-4; test_stft_inv.py::test_end_to_end_bounds checks them)
E2E_BOUNDS = {'64_48_10_f13_tone': 5.7e-6, '1024_1024_256_f65_tone': 2.0e-3}


# ---- the second table: plans whose frames do not cover every sample, and a filter above 1024 ---------------------------------
# name: (geometry, F, signals).  Each F passes stft_inv_check (samples(F) > filter_length // 2) and is what the plan gives
# samples(F) samples (Geom.frames(samples(F)) == F) as first chosen: none had to change (test_stft_inv.py asserts both).
#   gapped  the periodic Hann of 4 is [0, .5, 1, .5]: one kept sample in four has a summed squared window of exactly 0
#   sparse  hop > filter_length: runs of samples no frame covers; hop % 4 == 0, the strided forward path.  The Hann window
#           and filter_length = 16 are kept: the factor ten to every planted mistake holds as it is (test_stft_inv.py)
#   long    K > 1024 in both GEMMs, win_length < filter_length
EXTRA_GEOMS = {
    'gapped': (R.Geom(16, 4, 4), 9, ('tone', 'full', 'impulse')),
    'sparse': (R.Geom(16, 16, 24), 5, ('tone', 'full')),
    'long': (R.Geom(2048, 1200, 300), 9, ('tone', 'full')),
}
EXTRA_CASES = tuple(Case(f'{gname}_f{F}_{sig}', g, F, sig) for gname, (g, F, sigs) in EXTRA_GEOMS.items() for sig in sigs)
EXTRA_BY_NAME = {c.name: c for c in EXTRA_CASES}
EXTRA_NAMES = tuple(c.name for c in EXTRA_CASES)


# BOUNDS' rule on the extra cases alone, geometry by geometry: ten times the worst float32 numpy distance from float64
# (beside each bound; test_stft_inv.py::test_extra_bounds_lie_above_float32 prints and checks them), rounded up to two digits.
# 'spectrum' is the forward plan's: mel_stft_cases' bound for K <= 1024, mel_fn_cases.BOUNDS['wide'] for `long`.  gapped and
# sparse cannot rebuild the samples no window covers: no round-trip bound.  On gapped one frame covers a sample and its
# squared window is 1/4 or 1: the division and the scale are exact in any float format, so 'signal' is held to 0.
EXTRA_BOUNDS = {
    'gapped': {
        'frames': 7.7e-7,       # 7.666e-8
        'signal': 0.0,          # 0
        'spectrum': BOUNDS['spectrum'],
        'phasor': 8.9e-7,       # 8.802e-8
        'operand': 8.3e-7,      # 8.232e-8
        'inverse': 1.4e-6,      # 1.391e-7
    },
    'sparse': {
        'frames': 3.3e-7,       # 3.232e-8
        'signal': 9.6e-7,       # 9.516e-8
        'spectrum': BOUNDS['spectrum'],
        'phasor': 7.0e-7,       # 6.972e-8
        'operand': 7.9e-7,      # 7.875e-8
        'inverse': 5.1e-6,      # 5.049e-7: the division by a squared Hann edge of 1.4e-3 amplifies the frames' rounding
    },
    'long': {
        'frames': 3.5e-7,       # 3.493e-8
        'signal': 2.4e-6,       # 2.390e-7
        'spectrum': mel_fn_cases.BOUNDS['wide']['spectrum'],
        'phasor': 1.1e-6,       # 1.002e-7
        'operand': 9.7e-7,      # 9.689e-8
        'inverse': 1.1e-5,      # 1.050e-6
        'roundtrip': 1.4e-5,    # 1.311e-6
    },
}


def geom_name(name):
    """'gapped' | 'sparse' | 'long' of an extra case."""
    return name.split('_')[0]


def case_of(name):
    return BY_NAME[name] if name in BY_NAME else EXTRA_BY_NAME[name]


def uncovered(g, F):
    """bool [samples(F)]: the kept samples whose summed squared window (float64) is not above FLT_MIN -- the overlap-add
    leaves them undivided, and since every frame is 0 where its window is, they are exactly 0."""
    w2 = R.centred_window(g) ** 2
    ws = np.zeros(g.hop * (F - 1) + g.fl)
    for f in range(F):
        ws[f * g.hop:f * g.hop + g.fl] += w2
    return (ws <= R.FLT_MIN)[g.half:g.half + g.samples(F)]


def log_mel_case():
    """(audio [1, n], W [80, 513], Minv [80, 513]) of the log-mel test: the tone at (1024, 1024, 256), F = 65, under the default
    plan's filterbank (22 050 Hz, 80 channels, 0 - 8000 Hz)."""
    g = R.GEOMS[3]
    W = R.slaney_filterbank(22050, 1024, 80, 0.0, 8000.0)
    return R.signal('tone', g.samples(65), g, seed=65)[None], W, R.mel_inverse(W)


# Log-mel input on a ragged batch: (filter_length, win_length, hop_length, n_mel) at 22 050 Hz, 0 - 8000 Hz.  EK = n_mel
# rounded up to 32 is the K of the target's GEMM: 8 -> 32 (n_mel < 32), 32 -> 32 (no padding column), 80 -> 96 (the default
# plan).  32 channels need filter_length = 256: on 33 bins seven channels are empty, on 65 none is but the filterbank's rank
# is 26 and the plan's own Cholesky inverse rightly does not exist; 129 bins give rank 32.  With filter_length = 256 the
# hop is 32, not 16, so that the shortest row's samples(7) = 192 pass filter_length // 2 = 128 (stft_inv_check).
LOG_MEL_PLANS = {'mel8': (64, 64, 16, 8), 'mel32': (256, 64, 32, 32), 'mel80': (1024, 1024, 256, 80)}
LOG_MEL_F = 12
LOG_MEL_FRAMES = (LOG_MEL_F // 2 + 1, LOG_MEL_F, LOG_MEL_F - 1)


def log_mel_config(name):
    fl, wl, hop, n_mel = LOG_MEL_PLANS[name]
    return dict(sampling_rate=22050, n_mel_channels=n_mel, filter_length=fl, hop_length=hop, win_length=wl, mel_fmin=0.0,
                mel_fmax=8000.0)


@functools.lru_cache(maxsize=None)
def log_mel_rows(name):
    """(geometry, mel [3, F, n_mel] float32, W, Minv) of a plan of LOG_MEL_PLANS: row b is what TacotronSTFT returns for a
    seeded tone (float64 transform, rounded once), NaN at and beyond its LOG_MEL_FRAMES[b] frames."""
    fl, wl, hop, n_mel = LOG_MEL_PLANS[name]
    g = R.Geom(fl, wl, hop)
    W = R.slaney_filterbank(22050, fl, n_mel, 0.0, 8000.0)
    x = np.stack([R.signal('tone', g.samples(LOG_MEL_F), g, seed=30 + b) for b in range(len(LOG_MEL_FRAMES))])
    mel = np.log(np.maximum(R.polar(R.transform(x, g), g)[0] @ W.T, 1e-5)).astype(np.float32)
    for b, Fb in enumerate(LOG_MEL_FRAMES):
        mel[b, Fb:] = np.nan
    mel.setflags(write=False)
    return g, mel, W, R.mel_inverse(W)


def phasor_pairs():
    """float32 [11, 2]: (re, im) pairs at the ends of the float range -- FLT_MIN-sized, subnormal, 3e38-sized, mismatched by
    68 orders of magnitude, and the origin with either sign of zero.  Every one has an exact unit answer."""
    tiny = R.FLT_MIN
    return np.array([(tiny, tiny), (tiny, 0), (0, -tiny), (1e-42, 1e-42), (0, 1e-45), (3e38, 3e38), (-3e38, 1e-30), (1e-30, 3e38),
                     (1, 1e-30), (0, 0), (-0.0, 0)], np.float32)


def audio_of(case):
    return R.signal(case.signal, case.n, case.geom, seed=case.F)[None]


@functools.lru_cache(maxsize=None)
def target_of(name):
    """float32 magnitudes [1, F, cut] of a case: the float64 transform of its audio, rounded."""
    case = case_of(name)
    S = R.polar(R.transform(audio_of(case), case.geom), case.geom)[0].astype(np.float32)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def init_of(name):
    """A fixed complex initial phase [1, F, cut, 2] float32: pairs of any length, a few of them (0, 0)."""
    case = case_of(name)
    rng = np.random.default_rng(77 + case.F)
    init = rng.standard_normal((1, case.F, case.geom.cut, 2)).astype(np.float32) * 3.0
    init[0, ::3, ::5] = 0.0
    init.setflags(write=False)
    return init


def numpy_runner(name, momentum, init, dtype=np.float32, plant=None):
    """runner(what, k) over a numpy copy of the loop in `dtype`, every stage kept."""
    case = case_of(name)
    g = case.geom
    S, op = R.first_operand(target_of(name), g, init, None, dtype, plant)
    tprev = np.zeros_like(op)
    kept = {('target', 0): S}
    for k in range(N_ITERS + 1):
        kept[('operand', k)] = op
        st = R.loop_step(S, op, tprev, g, momentum, None, dtype, plant)
        for what in ('frames', 'signal', 'spectrum', 'phasor'):
            kept[(what, k)] = st[what]
        kept[('tprev', k)] = st['tprev']
        op, tprev = st['operand'], st['tprev']
    return lambda what, k: kept[(what, 0 if what == 'target' else k)]


def stage_errors(name, momentum, init, runner, tprev_of=None):
    """{stage: worst error over PROBE_KS} of a run against float64 applied to its own previous stage.  `tprev_of(k)`: the
    t_prev iteration k subtracts (default: the run's spectrum of iteration k - 1, which is what the definition says)."""
    case = case_of(name)
    g = case.geom
    f64 = lambda a: np.asarray(a, np.float64)
    S = f64(runner('target', 0))
    errs = {s: 0.0 for s in ('frames', 'signal', 'spectrum', 'phasor', 'operand')}
    alpha = float(np.float32(momentum / (1.0 + momentum)))
    _, op0 = R.first_operand(S, g, init)
    errs['operand'] = R.frame_error(runner('operand', 0), op0, g)
    for k in PROBE_KS:
        op = f64(runner('operand', k))
        tf = f64(runner('frames', k))
        errs['frames'] = max(errs['frames'], R.frames_error(tf, R.time_frames(op, g), op, g))
        sig = f64(runner('signal', k))
        errs['signal'] = max(errs['signal'], R.row_error(sig, R.overlap_add(tf, g, padded=True)))
        if k == N_ITERS:
            continue
        Y = f64(runner('spectrum', k))
        idx = np.arange(case.F)[:, None] * g.hop + np.arange(g.fl)[None, :]
        errs['spectrum'] = max(errs['spectrum'], R.frame_error(Y, sig[:, idx] @ f64(R.tables(g)[0]).T, g))
        tprev = np.zeros_like(Y) if k == 0 else f64(tprev_of(k) if tprev_of else runner('spectrum', k - 1))
        c = Y - alpha * tprev
        pr, pi = R.phasor(c[..., :g.cut], c[..., g.cut:])
        want = np.concatenate([pr, pi], -1)
        got = f64(runner('phasor', k))
        # a phasor is as good as its c: weigh a cell's error by |c| relative to the frame's largest |Y| or |t_prev| ...
        cm = np.sqrt(c[..., :g.cut] ** 2 + c[..., g.cut:] ** 2)
        ym = np.maximum(np.sqrt(Y[..., :g.cut] ** 2 + Y[..., g.cut:] ** 2), np.sqrt(tprev[..., :g.cut] ** 2 + tprev[..., g.cut:] ** 2))
        ym = ym.max(axis=-1, keepdims=True)
        wgt = np.concatenate([cm, cm], -1) / np.where(ym > 0, ym, 1.0)
        e = float((np.abs(got - want) * wgt).max()) if np.isfinite(got).all() else float('inf')
        # ... and P(0, 0) = (1, 0) exactly
        zero = np.concatenate([cm == 0, cm == 0], -1)
        if zero.any() and not np.array_equal(got[zero], want[zero]):
            e = float('inf')
        errs['phasor'] = max(errs['phasor'], e)
        nxt = f64(runner('operand', k + 1))
        errs['operand'] = max(errs['operand'], R.frame_error(nxt, R.stack(S, got[..., :g.cut], got[..., g.cut:]), g))
    return errs
