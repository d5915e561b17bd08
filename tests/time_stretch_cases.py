"""Shared cases, stage comparisons and bounds of the time-stretch tests (tests/test_time_stretch.py on the CPU,
test_time_stretch_gpu.py on an MI355X).

Every stage is compared with float64 applied to the SAME run's previous stage (`stage_errors`), so a stage's error is its own:
the spectrum against the float64 transform of the audio, m against the float64 magnitudes of that spectrum, the owners (which
must be equal) against the peaks of that m, the operand against the float64 chain on that spectrum, m and owners, the time
frames against the float64 inverse basis on that operand, the audio against the float64 overlap-add of those frames.
`runner(what)` returns a stage of the case's one row; on the CPU it is the float32 numpy copy (`numpy_runner`), whose distance
from float64 the bounds come from: BOUNDS[group][stage] is MARGIN = 10 times the worst float32 distance over the group's cases,
rounded up to two digits.  test_time_stretch.py asserts that every bound lies above that distance and a factor ten below each
planted mistake (time_stretch_ref.MISTAKES) at the stage it first shows in.
"""
import functools
from typing import NamedTuple

import numpy as np

import stft_inv_ref as R
import time_stretch_ref as V

MARGIN = 10
RATES = (0.25, 0.5, 0.8, 1.0, 1.25, 1.37, 2.0, 4.0)
SIGNALS = ('tone', 'noisy', 'impulse', 'dc', 'full', 'zeros', 'gaps')

# small: cut 33, one bin per thread of the parallel pass; gapped: win_length < filter_length; coarse: hop > filter_length / 2,
# the plan with rows of 2 and 3 analysis frames; default: cut 513, runs of 3 bins per thread; wide: cut 2049, more bins than
# the chain has threads
GEOMS = {'small': R.Geom(64, 64, 16), 'gapped': R.Geom(64, 48, 16), 'coarse': R.Geom(64, 64, 48), 'default': R.Geom(1024, 1024, 256),
         'wide': R.Geom(4096, 4096, 1024)}


class Case(NamedTuple):
    name: str
    group: str
    n: int
    signal: str
    rate: float

    @property
    def geom(self):
        return GEOMS[self.group]


def _cases():
    out = []
    add = lambda group, n, sig, r: out.append(Case(f'{group}_n{n}_{sig}_r{r:g}', group, n, sig, r))
    for sig in SIGNALS:
        for r in (0.5, 1.37):
            add('small', 701, sig, r)
    for r in RATES:
        if r not in (0.5, 1.37):
            add('small', 701, 'tone', r)
    for sig, r in (('tone', 0.8), ('gaps', 2.0), ('noisy', 0.25)):
        add('gapped', 500, sig, r)
    # F = 2 (n <= 95) and F = 3 with T = 1 (all zeros under an even filter_length) and T = 2
    for n, r in ((70, 2.0), (70, 1.5), (100, 4.0), (100, 2.0)):
        add('coarse', n, 'noisy', r)
    for sig, r in (('noisy', 0.5), ('noisy', 1.25), ('gaps', 0.8), ('noisy', 4.0)):
        add('default', 5000, sig, r)
    add('wide', 9000, 'noisy', 0.5)
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)
STAGES = ('spectrum', 'magnitude', 'owner', 'operand', 'frames', 'audio')

# measured float32 numpy distances, worst case of each group (test_time_stretch.py::test_bounds_lie_above_float32 prints and
# checks them); the owners must be equal
MEASURED = {
    'small': {'spectrum': 3.042e-7, 'magnitude': 1.273e-7, 'operand': 6.122e-7, 'frames': 7.471e-8, 'audio': 1.902e-7},
    'gapped': {'spectrum': 2.249e-7, 'magnitude': 1.131e-7, 'operand': 8.646e-7, 'frames': 3.991e-8, 'audio': 1.816e-7},
    'coarse': {'spectrum': 1.017e-7, 'magnitude': 4.660e-8, 'operand': 7.314e-8, 'frames': 1.406e-8, 'audio': 9.160e-8},
    'default': {'spectrum': 6.188e-7, 'magnitude': 1.023e-7, 'operand': 2.418e-7, 'frames': 6.021e-9, 'audio': 2.029e-7},
    'wide': {'spectrum': 2.693e-7, 'magnitude': 4.429e-8, 'operand': 2.255e-7, 'frames': 9.168e-10, 'audio': 2.427e-7},
}
BOUNDS = {
    'small': {'spectrum': 3.1e-6, 'magnitude': 1.3e-6, 'operand': 6.2e-6, 'frames': 7.5e-7, 'audio': 2.0e-6},
    'gapped': {'spectrum': 2.3e-6, 'magnitude': 1.2e-6, 'operand': 8.7e-6, 'frames': 4.0e-7, 'audio': 1.9e-6},
    'coarse': {'spectrum': 1.1e-6, 'magnitude': 4.7e-7, 'operand': 7.4e-7, 'frames': 1.5e-7, 'audio': 9.2e-7},
    'default': {'spectrum': 6.2e-6, 'magnitude': 1.1e-6, 'operand': 2.5e-6, 'frames': 6.1e-8, 'audio': 2.1e-6},
    'wide': {'spectrum': 2.7e-6, 'magnitude': 4.5e-7, 'operand': 2.3e-6, 'frames': 9.2e-9, 'audio': 2.5e-6},
}
# the stage each planted mistake first shows in ('owner': bins that differ, which the GPU tests hold to 0; a wrong frame
# count puts every stage from the magnitudes on infinitely far)
MISTAKE_STAGE = {'no_locking': 'operand', 'adv_t': 'operand', 'own_prev': 'operand', 'tie_up': 'owner', 'a_swapped': 'magnitude',
                 'rate_inverted': 'magnitude', 'T_short': 'magnitude', 'no_zero_frame': 'magnitude', 'rel_conj': 'operand',
                 'p0_zero': 'operand'}


def signal(kind, n, g, seed=0):
    """float32 [n]: 'tone' two partials, 'noisy' the same plus noise at -40 dB, 'impulse', 'dc', 'full' (+-1 full scale), 'zeros',
    'gaps' (the noisy tone with two stretches of exact zeros longer than a frame, so that whole frames are silent)."""
    rng = np.random.default_rng(500 + seed)
    t = np.arange(n, dtype=np.float64)
    k = max(2.3, g.fl / 9.7)
    tone = 0.5 * np.sin(2 * np.pi * k * t / g.fl + 0.4) + 0.2 * np.sin(2 * np.pi * 3.1 * k * t / g.fl)
    if kind == 'tone':
        x = tone
    elif kind in ('noisy', 'gaps'):
        x = tone + 0.005 * rng.standard_normal(n)
        if kind == 'gaps':
            x[n // 5:n // 5 + 2 * g.fl + g.hop] = 0.0
            x[n - n // 4:] = 0.0
    elif kind == 'impulse':
        x = np.zeros(n)
        x[n // 3] = 1.0
    elif kind == 'dc':
        x = np.full(n, 0.7)
    elif kind == 'full':
        x = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    elif kind == 'zeros':
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def audio_of(name):
    case = BY_NAME[name]
    x = signal(case.signal, case.n, case.geom, seed=case.n)
    x.setflags(write=False)
    return x


def numpy_runner(name, dtype=np.float32, plant=None):
    """runner(what) over a numpy copy of the call in `dtype`, every stage kept."""
    case = BY_NAME[name]
    kept = V.stages(audio_of(name), case.geom, case.rate, dtype=dtype, plant=plant)
    return lambda what: kept[what]


def stage_errors(name, runner):
    """{stage: error} of a run against float64 applied to its own previous stage; 'owner' counts the bins that differ.  A
    stage of another shape than the definition gives (a wrong frame count) is infinitely far."""
    case = BY_NAME[name]
    g, r = case.geom, case.rate
    f64 = lambda a: np.asarray(a, np.float64)
    spec, m, op, tf, audio = (f64(runner(what)) for what in ('spectrum', 'magnitude', 'operand', 'frames', 'audio'))
    own = np.asarray(runner('owner')).astype(np.int64)
    X = V.to_complex(spec, g)
    errs = {'spectrum': R.frame_error(spec[None], V.row_spectrum(audio_of(name), case.n, g)[None], g)}
    want_m = V.magnitudes(X, r)
    if want_m.shape != m.shape or V.out_samples(case.n, r) != len(audio):
        return dict(errs, magnitude=float('inf'), owner=float('inf'), operand=float('inf'), frames=float('inf'), audio=float('inf'))
    errs['magnitude'] = V.magnitude_error(m, want_m)
    errs['owner'] = int((own != V.owners(m)).sum())
    errs['operand'] = R.frame_error(op[None], V.from_complex(V.chain(X, r, m, own))[None], g)
    errs['frames'] = R.frames_error(tf[None], R.time_frames(op[None], g), op[None], g)
    errs['audio'] = R.row_error(audio[None], V.finish(tf, g, case.n, r)[None])
    return errs
