"""Shared cases, stage comparisons and bounds of the STFT-inverse / Griffin-Lim tests (tests/test_stft_inv.py on the CPU,
test_stft_inv_gpu.py on an MI355X).

Every stage is compared with float64 applied to the SAME run's previous stage (`stage_errors`), so a stage's error is its
own.  `runner(what, k)` returns a probed stage; on the CPU it is the float32 numpy copy of the loop (`numpy_runner`), whose
distances from float64 the bounds come from: BOUNDS[stage] is ten times the worst float32 distance over CASES, rounded up to
two digits ('spectrum' reuses the mel-STFT bound of tests/mel_stft_cases.py, derived there by the same rule).
test_stft_inv.py asserts that every bound lies above the float32 distance and a factor ten below the weakest planted mistake
(stft_inv_ref.MISTAKES) at the stage that mistake first shows in.
"""
import functools
from typing import NamedTuple

import numpy as np

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


def log_mel_case():
    """(audio [1, n], W [80, 513], Minv [80, 513]) of the log-mel test: the tone at (1024, 1024, 256), F = 65, under the default
    plan's filterbank (22 050 Hz, 80 channels, 0 - 8000 Hz)."""
    g = R.GEOMS[3]
    W = R.slaney_filterbank(22050, 1024, 80, 0.0, 8000.0)
    return R.signal('tone', g.samples(65), g, seed=65)[None], W, R.mel_inverse(W)


def audio_of(case):
    return R.signal(case.signal, case.n, case.geom, seed=case.F)[None]


@functools.lru_cache(maxsize=None)
def target_of(name):
    """float32 magnitudes [1, F, cut] of a case: the float64 transform of its audio, rounded."""
    case = BY_NAME[name]
    S = R.polar(R.transform(audio_of(case), case.geom), case.geom)[0].astype(np.float32)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def init_of(name):
    """A fixed complex initial phase [1, F, cut, 2] float32: pairs of any length, a few of them (0, 0)."""
    case = BY_NAME[name]
    rng = np.random.default_rng(77 + case.F)
    init = rng.standard_normal((1, case.F, case.geom.cut, 2)).astype(np.float32) * 3.0
    init[0, ::3, ::5] = 0.0
    init.setflags(write=False)
    return init


def numpy_runner(name, momentum, init, dtype=np.float32, plant=None):
    """runner(what, k) over a numpy copy of the loop in `dtype`, every stage kept."""
    case = BY_NAME[name]
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
    case = BY_NAME[name]
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
