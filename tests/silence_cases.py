"""Inputs that take silence removal (csrc/silence.hip) past its carried scans and onto its rounding edges, and the reference
side of the stages HipEngine.remove_silence_probe returns (tests/test_silence_stages.py holds the conditions on these
inputs, tests/test_silence_stages_gpu.py compares the GPU with them).

The carries: sil_row_scan_kernel works in chunks of 1024 tiles of 2048 samples (a row of more than 2 097 152 samples has a
second chunk); sil_rms_runs_kernel runs three passes in chunks of 1024 entries: over the block flags (`prev_loud`, `ns`),
over the listed silences (`nm`) and over the merged ones.  The rounding edges: a voice of exactly min_voice_time between
two silences, and a trailing silence that ends one sample before the row does, where a fused multiply-add decides the
other way than the reference's doubles.
"""
from fractions import Fraction

import numpy as np

import silence_ref as sr

TILE, CHUNK = 2048, 1024


def blocks_signal(silent_flags, bs, L, seed):
    """L samples in blocks of bs: loud samples alternate in sign with |x| in [0.25, 0.5], silent ones have |x| <= 2e-3, so
    every block's peak stands 0.96 or more (relative) from the -25 dB threshold 0.0562.  Samples behind the last flag's
    block are loud."""
    flags = np.asarray(silent_flags, bool)
    assert (len(flags) - 1) * bs < L
    u = (sr.lcg(L, seed) >> np.uint64(8)).astype(np.float64) / float(1 << 24)             # [0, 1)
    t = np.arange(L)
    silent = np.zeros(L, bool)
    rep = np.repeat(flags, bs)[:L]
    silent[:len(rep)] = rep
    loud = (0.25 + 0.25 * u) * np.where(t % 2 == 0, 1.0, -1.0)
    x = np.where(silent, (u - 0.5) * 4e-3, loud).astype(np.float32)
    x.setflags(write=False)
    return x


def runs_pattern(n_blocks, seed, silent_runs=(1, 3), loud_runs=(1, 4), first_silent=True):
    """n_blocks flags: alternating silent and loud runs whose lengths the LCG draws from the two inclusive ranges."""
    draws = (sr.lcg(n_blocks, seed) >> np.uint64(16)).astype(np.int64)
    flags, silent, k = [], first_silent, 0
    while len(flags) < n_blocks:
        lo, hi = silent_runs if silent else loud_runs
        flags += [silent] * (lo + int(draws[k]) % (hi - lo + 1))
        silent, k = not silent, k + 1
    return np.array(flags[:n_blocks], bool)


def fma(a, b, c):
    """a * b + c rounded once, as v_fma_f64 gives it."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fused_link(j_prev, i_next, L, rate, bs, mvt):
    """The link decision of a pair of listed silences with the product of the later start fused into the subtraction."""
    bt = bs / rate
    return fma(float(i_next), bt, -min(L / rate, j_prev * bt)) < mvt


def fused_ends_row(j, L, rate, bs):
    """`ends within one sample of the row's end` of a silence that ends at block j with e * rate fused into the subtraction."""
    e = min(L / rate, j * (bs / rate))
    return abs(fma(e, float(rate), -float(L))) <= 1.0


class Rms:
    """One rms input and the settings it is run with: `kws` lists the keyword sets of the calls (mode apart)."""

    def __init__(self, name, rate, x, kws, modes=sr.RMS_MODES):
        self.name, self.rate, self.x, self.kws, self.modes = name, rate, x, kws, modes

    def calls(self):
        return [dict(kw, mode=m) for kw in self.kws for m in self.modes]


def _carry():
    bs, nb = 16, 20000
    x = blocks_signal(runs_pattern(nb, CARRY_SEED), bs, nb * bs - 5, 41)
    base = dict(block_size=bs, min_silence=0.001)
    return Rms('carry', 22050, x, [dict(base, min_voice_time=mvt, replace_by=rb) for mvt in (0.002, 0) for rb in (8, 0)])


def _cap_edge():
    flags = np.arange(2051) % 2 == 0                    # silent, loud, ..., silent: 1026 silences of one block
    return Rms('cap_edge', 22050, blocks_signal(flags, 4, 2051 * 4, 42),
               [dict(block_size=4, min_silence=0, min_voice_time=0, replace_by=2)])


def _chunk_rows():
    """Rows of 1024 and 1025 blocks of 16 samples: the second chunk of the flag pass holds nothing, one silent flag (the end
    of a run that began in the first chunk) or one loud flag (behind a run that ends with the first chunk)."""
    f = runs_pattern(1025, 7)
    one_chunk = f[:1024].copy()
    over_silent, over_loud = f.copy(), f.copy()
    over_silent[1021:1025] = [False, True, True, True]
    over_loud[1021:1025] = [False, True, True, False]
    kws = [dict(block_size=16, min_silence=0.001, min_voice_time=0.002, replace_by=8)]
    return [Rms('one_chunk', 22050, blocks_signal(one_chunk, 16, 1024 * 16, 43), kws),
            Rms('one_over_silent', 22050, blocks_signal(over_silent, 16, 1025 * 16, 44), kws),
            Rms('one_over_loud', 22050, blocks_signal(over_loud, 16, 1025 * 16 - 3, 45), kws)]


def _pattern(runs):
    """[(blocks, silent)] -> flags"""
    return np.concatenate([np.full(n, s, bool) for n, s in runs])


def _gap20():
    flags = _pattern([(10, True), (20, False), (12, True), (25, False), (11, True), (7, False)])
    return Rms('gap20', 16000, blocks_signal(flags, 160, len(flags) * 160, 46), [dict(replace_by=0.05)])


def _tail_one_loud(rate, bs, loud, j, seed):
    flags = _pattern([(loud, False), (j - loud, True), (1, False)])
    return Rms(f'tail_one_loud_{rate}', rate, blocks_signal(flags, bs, j * bs + 1, seed), [dict(replace_by=0.1)])


CARRY_SEED = 20             # picked so that the conditions of test_silence_stages.py::test_carry_reaches_every_carry hold
# what the reference gives: kept samples in modes start_end, start, end, remove
KEPT = {'gap20': (7680, 7680, 13600, 6720), 'tail_one_loud_22050': (4845, 5501, 4845, 4845)}
GAP20_UNMERGED = (12800, 12800, 13600, 10720)

_rms = {}


def rms_cases():
    if not _rms:
        for c in [_carry(), _cap_edge(), *_chunk_rows(), _gap20(), _tail_one_loud(22050, 220, 12, 25, 47),
                  _tail_one_loud(16000, 160, 8, 21, 48)]:
            _rms[c.name] = c
    return _rms


RMS_NAMES = ('carry', 'cap_edge', 'one_chunk', 'one_over_silent', 'one_over_loud', 'gap20', 'tail_one_loud_22050',
             'tail_one_loud_16000')


def rms_reference(x, rate, **kw):
    """Every stage of an rms call on one row: flags, intervals (n, cut, d0, d1), mask, tile offsets, the kept samples."""
    x = np.asarray(x, np.float32)
    iv, cut = sr.rms_intervals(x, rate, **kw)
    mask = sr.interval_mask(len(x), iv, cut)
    return dict(flags=sr.rms_flags(x, rate, **kw), n=len(iv), cut=cut, d0=np.array([a for a, _ in iv], np.int32),
                d1=np.array([b for _, b in iv], np.int32), mask=mask, tile_offsets=tile_offsets(mask), out=x[mask != 0])


def tile_offsets(mask):
    """Kept samples before each tile of 2048: the exclusive cumsum of the tiles' counts."""
    nt = -(-len(mask) // TILE)
    cnt = np.zeros(nt * TILE, np.int64)
    cnt[:len(mask)] = mask
    return np.concatenate([[0], np.cumsum(cnt.reshape(nt, TILE).sum(axis=1))[:-1]]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------- the long batch
LONG_RATE = 22050
LONG_LENGTHS = (TILE * (CHUNK + 1) + 777, TILE * CHUNK, TILE * CHUNK + 1, 30000)
LONG_CALLS = (('rms', dict(mode='remove', replace_by=0.1)), ('remove', {}))
LONG_KEPT = {'rms': 1695448, 'remove': 1798590}     # what the restatement keeps of the long row
LONG_MARGIN = 1e-6         # mean-window, relative: over 2.1 M squares two orders of an fp64 sum differ by 3.5e-10 of it
_long = {}


def long_rows():
    """Four rows cut from one signal of alternating utterances (0.35 to 0.65 s) and pauses (0.2 to 0.32 s), an utterance
    first: one row with a second chunk of tiles, one that fills the first chunk exactly, one with a single sample in the
    second, one short."""
    if not _long:
        need, seg, k = max(LONG_LENGTHS) + 3 * 4099, [], 0
        draws = (sr.lcg(4096, 51) >> np.uint64(8)).astype(np.float64) / float(1 << 24)
        while sum(sr._samples(d, LONG_RATE) for d, _ in seg) < need:
            seg += [(0.35 + 0.3 * float(draws[2 * k]), sr.LOUD), (0.2 + 0.12 * float(draws[2 * k + 1]), sr.Q)]
            k += 1
        base = sr.build(LONG_RATE, seg, 52)
        rows = [base[b * 4099:b * 4099 + L] for b, L in enumerate(LONG_LENGTHS)]
        for r in rows:
            r.setflags(write=False)
        _long['rows'] = rows
    return _long['rows']


def long_batch():
    """[4, N] with NaN behind each row's length."""
    a = np.full((len(LONG_LENGTHS), max(LONG_LENGTHS)), np.nan, np.float32)
    for b, r in enumerate(long_rows()):
        a[b, :len(r)] = r
    return a


def long_reference(b, method):
    """(mask, margin) of row b; the mean-window method from the longdouble prefix."""
    key = (b, method)
    if key not in _long:
        x = long_rows()[b]
        if method == 'rms':
            kw = LONG_CALLS[0][1]
            _long[key] = (sr.keep_mask('rms', x, LONG_RATE, **kw), sr.rms_margin(x, LONG_RATE))
        else:
            _long[key] = sr.mean_window_long(x, LONG_RATE)
    return _long[key]


# ---------------------------------------------------------------------------------------------------------- the prefix bound
# |P_gpu[t] - P[t]| <= PREFIX_DEPTH * 2^-53 * P[t] against the longdouble prefix: all summands are squares, so a summation
# tree errs by at most its depth in roundings, to first order.  The depth of P[t], counted from silence.hip:
#    7   a thread's run of 8 squares (sil_square_sum_kernel; the first add to 0 is exact)
#    6   the wave scan of those, 64 lanes
#    3   the fold of the 4 waves' totals into the tile's sum
#    6   sil_row_scan_kernel: the wave scan of the tile sums
#   15   its fold of up to 16 waves' totals (into `base`, and into `all` for the carry)
#    1   base + the lane before (the exclusive value; nothing is subtracted)
#    2   carry += all once per chunk of 1024 tiles (rows up to 2 chunks here), carry + the chunk's own value
#    1   sil_square_prefix_kernel: toff + its own exclusive scan (wave scan, fold and shift, 6 + 3 + 1, run beside the 40
#        above and are shorter)
#    8   the run inside the thread up to P[t] (8 for P[L])
PREFIX_DEPTH = 7 + 6 + 3 + 6 + 15 + 1 + 2 + 1 + 8           # 49
# Measured on an MI355X, worst |P_gpu - P| / (2^-53 P[t]) over all t >= 1: the long batch PREFIX_MEASURED['long'], the small
# mean-window inputs (which begin with silence) PREFIX_MEASURED['small'].  Before the exclusive scan, when the kernels took a
# thread's (a tile's) own sum off an inclusive value, the short long row, which begins in a pause, measured 161.9 at t = 2048.
PREFIX_MEASURED = {'long': 7.37, 'small': 3.26}             # (the four long rows: 6.99, 6.68, 7.37, 3.49)
