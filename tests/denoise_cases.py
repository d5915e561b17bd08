"""Shared cases, stage comparisons and bounds of the denoiser tests (tests/test_denoise.py on the CPU, test_denoise_gpu.py on
an MI355X).

The geometries, frame counts and signals are those of tests/stft_inv_cases.py (the 64-row GEMM tile turns over at F = 63, 64,
65 of the default geometry), each at the strengths 0.1, 1 and 10, against a bias that is the frame-0 magnitude of a fixed
seeded noise-plus-tone signal under the same geometry.  Every stage is compared with float64 applied to the SAME run's previous
stage (`stage_errors`), so a stage's error is its own.  `runner(what)` returns a probed stage; on the CPU it is the float32
numpy copy (`numpy_runner`).  BOUNDS['operand'] is ten times the worst float32 distance over CASES, rounded up to two
digits; the time frames and the audio reuse the STFT inverse's bounds.  test_denoise.py asserts that every bound lies above
the float32 distance and a factor ten below each planted mistake (denoise_ref.MISTAKES) on the case it shows best in.
"""
import functools
from typing import NamedTuple

import numpy as np

import denoise_ref as D
import stft_inv_cases as SC
import stft_inv_ref as R

STRENGTHS = (0.1, 1.0, 10.0)

# measured float32 numpy distances (test_denoise.py::test_bounds_lie_above_float32 prints and checks them):
# operand 1.83e-7, frames 1.49e-7, audio 1.01e-6
BOUNDS = {
    'operand': 1.9e-6,
    'frames': SC.BOUNDS['frames'],
    'audio': SC.BOUNDS['inverse'],
}
CLAMPED = (0.10, 0.90)          # share of the bins a tone case at strength 1 must clamp: both branches of the gate run


class Case(NamedTuple):
    name: str
    base: str                   # the case of stft_inv_cases
    strength: float

    @property
    def geom(self):
        return SC.case_of(self.base).geom

    @property
    def F(self):
        return SC.case_of(self.base).F

    @property
    def n(self):
        return SC.case_of(self.base).n

    @property
    def signal(self):
        return SC.case_of(self.base).signal

    @property
    def s(self):
        """The strength the kernel uses: rounded to float32."""
        return float(np.float32(self.strength))


CASES = tuple(Case(f'{c.name}_s{s:g}', c.name, s) for c in SC.CASES for s in STRENGTHS)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)

# The second table: the tone of each extra geometry of stft_inv_cases (gapped, sparse, long) at strength 0.5.
EXTRA_STRENGTH = 0.5
EXTRA_CASES = tuple(Case(f'{gname}_s{EXTRA_STRENGTH:g}', f'{gname}_f{F}_tone', EXTRA_STRENGTH)
                    for gname, (g, F, _) in SC.EXTRA_GEOMS.items())
EXTRA_BY_NAME = {c.name: c for c in EXTRA_CASES}
EXTRA_NAMES = tuple(c.name for c in EXTRA_CASES)
# BOUNDS' rule geometry by geometry: the operand ten times the float32 numpy distance (beside it;
# test_denoise.py::test_extra_bounds_lie_above_float32 prints and checks them), the time frames and the audio the STFT
# inverse's bounds of that geometry.  Measured operand distances: gapped 1.082e-7, sparse 1.203e-7, long 1.109e-7
EXTRA_BOUNDS = {
    'gapped': {'operand': 1.1e-6, 'frames': SC.EXTRA_BOUNDS['gapped']['frames'], 'audio': SC.EXTRA_BOUNDS['gapped']['inverse']},
    'sparse': {'operand': 1.3e-6, 'frames': SC.EXTRA_BOUNDS['sparse']['frames'], 'audio': SC.EXTRA_BOUNDS['sparse']['inverse']},
    'long': {'operand': 1.2e-6, 'frames': SC.EXTRA_BOUNDS['long']['frames'], 'audio': SC.EXTRA_BOUNDS['long']['inverse']},
}


def case_of(name):
    return BY_NAME[name] if name in BY_NAME else EXTRA_BY_NAME[name]


def audio_of(case):
    return SC.audio_of(SC.case_of(case.base))


@functools.lru_cache(maxsize=None)
def bias_of(g):
    """float32 [cut]: the frame-0 magnitude of a fixed noise-plus-tone signal under `g`."""
    n = g.samples(9)
    rng = np.random.default_rng(4242)
    t = np.arange(n, dtype=np.float64)
    x = 0.05 * np.sin(2 * np.pi * max(1.3, g.fl / 5.3) * t / g.fl) + 0.02 * rng.standard_normal(n)
    bias = D.magnitude(R.transform(x[None], g), g)[0, 0].astype(np.float32)
    bias.setflags(write=False)
    return bias


def numpy_runner(name, dtype=np.float32, plant=None):
    """runner(what) over a numpy copy of the call in `dtype`, every stage kept."""
    case = case_of(name)
    g, x = case.geom, audio_of(case)
    kept = {'spectrum': R.transform(x, g, dtype)}
    kept['operand'] = D.gate(kept['spectrum'], bias_of(g), case.s, g, None, dtype, plant)
    kept['frames'] = R.time_frames(kept['operand'], g, dtype)
    kept['audio'] = D.cut_rows(R.overlap_add(kept['frames'], g, None, dtype), [case.n], g, case.n, dtype, plant)
    return lambda what: kept[what]


def stage_errors(name, runner):
    """{stage: error} of a run against float64 applied to its own previous stage; the audio against float64 on its operand."""
    case = case_of(name)
    g = case.geom
    f64 = lambda a: np.asarray(a, np.float64)
    spec, op, tf, audio = (f64(runner(what)) for what in ('spectrum', 'operand', 'frames', 'audio'))
    want_audio = D.cut_rows(R.inverse(op, g), [case.n], g, case.n)
    return {'operand': D.operand_error(op, D.gate(spec, bias_of(g), case.s, g), spec, g),
            'frames': R.frames_error(tf, R.time_frames(op, g), op, g),
            'audio': R.row_error(audio, want_audio)}
