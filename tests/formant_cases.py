"""Shared cases, stage comparisons and bounds of the formant-match tests (tests/test_formant.py on the CPU,
test_formant_gpu.py on an MI355X).

Every stage is compared with float64 applied to the SAME run's previous stage (`stage_errors`), so a stage's error is its own:
the log-magnitudes against the float64 logarithm of that run's spectra (on the GPU: `mel_fn_probe`'s), the envelopes against
the float64 product of those log-magnitudes with the table, the gain against float64 steps 4 - 6 on those envelopes and the
audio's spectrum, the operand against that gain times that spectrum, the time frames against the float64 inverse basis on that
operand, the audio against the float64 overlap-add of those frames.  `runner(what)` returns a stage of the case's batch; on the
CPU it is the float32 numpy copy (`numpy_runner`), whose distance from float64 the bounds come from: BOUNDS[group][stage] is
MARGIN = 10 times the worst float32 distance over the group's cases, rounded up to two digits.  test_formant.py asserts that
every bound lies above that distance and a factor ten below each planted mistake (formant_ref.MISTAKES) at the stage it first
shows in.

The rows of a case share one pair of signal kinds (audio, source), one lifter cut and one maximum gain; each row has its own
seed, length and warp.  2 * B * F, the rows of the envelope GEMM, is even: it cannot be 63 or 65.  The row counts are chosen so
that B * F -- the row at which the audio's half of the stacked operand begins -- is 63, 64 and 65 (2 * B * F = 126, 128, 130
around the GEMM's second 64-row tile), and so that 2 * B * F is 64 and 66 around its first.
"""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import formant_ref as Fm
import stft_inv_ref as R
import time_stretch_cases as TC

MARGIN = 10
GEOMS = {name: TC.GEOMS[name] for name in ('small', 'gapped', 'default')}
WARPS = (0.5, 0.8, 1.0, 1.37, 2.0)
UNLIKE = (('tone', 'noisy'), ('noisy', 'impulse'), ('impulse', 'dc'), ('dc', 'full'), ('full', 'zeros'), ('zeros', 'gaps'),
          ('gaps', 'tone'))


class Case(NamedTuple):
    name: str
    group: str
    N: int
    lengths: Tuple[int, ...]
    audio: str
    source: Optional[str]           # None: the call's source is NULL
    scale: float                    # the source's amplitude against the signal kind's own
    Q: int
    warps: Tuple[float, ...]
    max_gain_db: float = 24.0

    @property
    def geom(self):
        return GEOMS[self.group]

    @property
    def B(self):
        return len(self.lengths)


def max_len(g):
    return 9 * g.fl // 2 + 7


def _cases():
    out = []

    def add(group, tag, lengths, audio, source, Q=None, warps=(1.0,), scale=1.0, db=24.0, N=None):
        g = GEOMS[group]
        lengths = tuple(int(n) for n in lengths)
        warps = tuple(warps) * len(lengths) if len(warps) == 1 else tuple(warps)
        Q = Fm.default_lifter(g.fl) if Q is None else Q
        out.append(Case(f'{group}_{tag}', group, N or max(lengths), lengths, audio, source, scale, Q, warps, db))

    for group in GEOMS:
        g = GEOMS[group]
        n, top = max_len(g), g.fl // 2 - 1
        for i, (a, s) in enumerate(UNLIKE):                      # unlike pairs, a warp each
            add(group, f'{a}_{s}', [n], a, s, warps=(WARPS[i % len(WARPS)],), Q=(None, 1, top)[i % 3])
        for w in WARPS:                                          # every warp against the audio itself (source NULL)
            add(group, f'self_w{w:g}', [n - 3], 'noisy', None, warps=(w,))
        add(group, 'louder', [n], 'noisy', 'tone', scale=1000.0)            # the clamp from above
        add(group, 'quieter', [n], 'noisy', 'tone', scale=0.001, warps=(1.37,))         # ... and from below
        add(group, 'mixed_clamp', [n], 'gaps', 'noisy', scale=30.0, db=6.0, warps=(0.8,))
        add(group, 'short', [g.wl - g.hop - 1], 'noisy', 'tone', warps=(2.0,))          # a row shorter than win_length
        add(group, 'q1', [n], 'noisy', 'full', Q=1)
        add(group, 'qtop', [n], 'noisy', 'full', Q=top, warps=(0.5,))
    # row counts: F = frames(N) slots per row
    g = GEOMS['small']
    for B, F in ((7, 9), (4, 16), (5, 13), (2, 16), (3, 11)):    # B * F = 63, 64, 65, 32, 33
        N = (F - 1) * g.hop + 5
        assert g.frames(N) == F and N <= max_len(g)
        lengths = [N] + [N - 1 - 7 * b for b in range(1, B)]
        add('small', f'rows_{B}x{F}', lengths, 'noisy', 'tone', warps=[WARPS[b % len(WARPS)] for b in range(B)], N=N)
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)
assert len(BY_NAME) == len(CASES)
STAGES = ('logmag', 'envelope', 'gain', 'operand', 'frames', 'audio')

# measured float32 numpy distances, worst case of each group (test_formant.py::test_bounds_lie_above_float32 prints and
# checks them)
MEASURED = {
    'small': {'logmag': 5.379e-07, 'envelope': 3.815e-06, 'gain': 6.523e-07, 'operand': 5.139e-08, 'frames': 3.523e-08, 'audio': 1.854e-07},
    'gapped': {'logmag': 5.146e-07, 'envelope': 4.442e-06, 'gain': 5.312e-07, 'operand': 5.483e-08, 'frames': 4.958e-08, 'audio': 1.879e-07},
    'default': {'logmag': 5.778e-07, 'envelope': 2.861e-05, 'gain': 1.028e-06, 'operand': 5.528e-08, 'frames': 4.262e-08, 'audio': 2.029e-07},
}
BOUNDS = {
    'small': {'logmag': 5.4e-06, 'envelope': 3.9e-05, 'gain': 6.6e-06, 'operand': 5.2e-07, 'frames': 3.6e-07, 'audio': 1.9e-06},
    'gapped': {'logmag': 5.2e-06, 'envelope': 4.5e-05, 'gain': 5.4e-06, 'operand': 5.5e-07, 'frames': 5.0e-07, 'audio': 1.9e-06},
    'default': {'logmag': 5.8e-06, 'envelope': 2.9e-04, 'gain': 1.1e-05, 'operand': 5.6e-07, 'frames': 4.3e-07, 'audio': 2.1e-06},
}
# the stage each planted mistake first shows in
MISTAKE_STAGE = {'w_edge': 'envelope', 'v_single': 'envelope', 'Q_minus': 'envelope', 'Q_plus': 'envelope', 'no_floor': 'logmag',
                 'floor_on_log': 'logmag', 'warp_inverted': 'gain', 'no_top_hold': 'gain', 'clamp_sx': 'gain', 'db_as_nepers': 'gain',
                 'no_energy': 'gain', 'energy_no_sqrt': 'gain', 'swapped': 'logmag', 'real_only': 'operand'}


@functools.lru_cache(maxsize=None)
def inputs_of(name):
    """(audio [B, N], source [B, N] or None) float32; zeros behind every row's length."""
    case = BY_NAME[name]
    g = case.geom
    x = np.zeros((case.B, case.N), np.float32)
    s = None if case.source is None else np.zeros((case.B, case.N), np.float32)
    for b, n in enumerate(case.lengths):
        x[b, :n] = TC.signal(case.audio, n, g, seed=n + b)
        if s is not None:
            s[b, :n] = np.float32(case.scale) * TC.signal(case.source, n, g, seed=1000 + n + b)
    for a in (x, s):
        if a is not None:
            a.setflags(write=False)
    return x, s


def _pad(a, F):
    """[.., F_b, w] -> [.., F, w]: zeros in the frames behind the row's own."""
    a = np.asarray(a)
    pad = [(0, 0)] * a.ndim
    pad[-2] = (0, F - a.shape[-2])
    return np.pad(a, pad)


def numpy_runner(name, dtype=np.float32, plant=None):
    """runner(what) over a numpy copy of the call in `dtype`, every stage kept: spectrum [2, B, F, 2 cut], logmag and envelope
    [2, B, F, cut], gain [B, F, cut], operand [B, F, 2 cut], frames [B, F, fl], audio [B, N]."""
    case = BY_NAME[name]
    g, F = case.geom, case.geom.frames(case.N)
    x, s = inputs_of(name)
    rows = [Fm.stages(x[b, :n], None if s is None else s[b, :n], g, case.Q, case.warps[b], case.max_gain_db, dtype=dtype, plant=plant)
            for b, n in enumerate(case.lengths)]
    kept = {}
    for what in ('logmag', 'envelope'):
        kept[what] = np.stack([_pad(r[what], F) for r in rows], axis=1)
    # the spectra are the call's inputs, not a stage of it: no planted mistake reaches them
    kept['spectrum'] = np.stack([_pad(np.stack([Fm.row_spectrum((x if s is None else s)[b], n, g, dtype), Fm.row_spectrum(x[b], n, g, dtype)]), F)
                                 for b, n in enumerate(case.lengths)], axis=1)
    for what in ('gain', 'operand', 'frames'):
        kept[what] = np.stack([_pad(r[what], F) for r in rows])
    kept['audio'] = np.stack([np.pad(r['audio'], (0, case.N - len(r['audio']))) for r in rows])
    return lambda what: kept[what]


def stage_errors(name, runner):
    """{stage: error} of a run against float64 applied to its own previous stage, the worst row of the case; frames behind a
    row's own must hold zeros (else the stage is infinitely far)."""
    case = BY_NAME[name]
    g, F = case.geom, case.geom.frames(case.N)
    f64 = lambda a: np.asarray(a, np.float64)
    spec, l, S, gain, op, tf, audio = (f64(runner(what)) for what in ('spectrum', 'logmag', 'envelope', 'gain', 'operand', 'frames',
                                                                      'audio'))
    errs = {s: 0.0 for s in STAGES}
    worse = lambda s, e: errs.__setitem__(s, max(errs[s], e))
    for b, n in enumerate(case.lengths):
        Fb = g.frames(n)
        for s, a in (('logmag', l[:, b, Fb:]), ('envelope', S[:, b, Fb:]), ('gain', gain[b, Fb:]), ('operand', op[b, Fb:]),
                     ('frames', tf[b, Fb:]), ('audio', audio[b, max(0, min(n, g.samples(Fb))):])):
            if a.size and not (a == 0).all():
                worse(s, float('inf'))
        worse('logmag', Fm.abs_error(l[:, b, :Fb], Fm.logmag(spec[:, b, :Fb], g)))
        worse('envelope', Fm.abs_error(S[:, b, :Fb], Fm.envelope(l[:, b, :Fb], g, case.Q)))
        want = Fm.gains(S[0, b, :Fb], S[1, b, :Fb], spec[1, b, :Fb], g, case.warps[b], case.max_gain_db)
        worse('gain', Fm.gain_error(gain[b, :Fb], want))
        worse('operand', R.frame_error(op[None, b, :Fb], Fm.apply_gain(gain[b, :Fb], spec[1, b, :Fb], g)[None], g))
        worse('frames', R.frames_error(tf[None, b, :Fb], R.time_frames(op[None, b, :Fb], g), op[None, b, :Fb], g))
        worse('audio', R.row_error(audio[None, b, :n], Fm.finish(tf[b, :Fb], g, n)[None]))
    return errs
