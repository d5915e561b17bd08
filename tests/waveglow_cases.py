"""Shared case table of the WaveGlow-variant tests (tests/test_waveglow_variants.py on the CPU, _gpu.py on an MI355X).

`waveglow_run` (csrc/waveglow.hip) picks its WN-layer GEMMs from the frame count B*T, the precision and the form (`wg_plan`,
csrc/wg_plan.h, then the `kWnKernels` table of `WnKernels`): four
fp32 tile families of the direct form, the Winograd form of layers 1 - 7 (csrc/wn_wino.hip) with its three group kinds and
two measurement forms, the fp16 and the split-fp16 (f16x3) kernels.  `pick_variant` restates those rules, so a test can
say which instantiation a call must take and check that the case table reaches every one of them; tests/test_wg_plan.py
compares the restatement with `wg_plan` itself on the CPU.

References come from the numpy oracle in float64, once per case (`flow11_acts`): the gated activations of the 8 WN layers
of flow 11, the first flow that runs, whose input is exactly sigma * z.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

# ---- bounds ------------------------------------------------------------------------------------------------------------
# One WN layer's gated activations tanh(.) * sigmoid(.) (|acts| < 1, RMS ~0.3) against the float64 oracle.  Three metrics:
# RMS of the error / RMS of the reference over all positions ('rel'), max abs error ('abs'), and the relative RMS over the
# edge windows -- the first and last d positions of every utterance, d the layer's dilation -- where a tap that leaks
# across an utterance end shows ('edge').  Worst values measured on an MI355X over every case x precision x form of
# test_waveglow_variants_gpu.py (flow 11, and flows 7 and 3 from the GPU's own input):
#   f32    rel 1.93e-6 (b1_t193, Winograd)  edge 2.34e-6 (b1_t193, Winograd)  abs 6.41e-5 (b5_t77, Winograd)
#   f16x3  rel 1.55e-6 (b1_t257)            edge 1.43e-6                      abs 2.66e-5 (b3_t64)
#   f16    rel 8.03e-4 (b1_t193)            edge 7.57e-4 (b2_t128)            abs 1.18e-2 (b1_t383)
# The same metrics for runs with row lengths (test_waveglow_rows_gpu.py: MASK_LENS / MASK_FLAGS kernels, zeroed tails, the
# packed row's gather), PER ROW against the oracle on the row's own frames, worst over rows, layers and cases:
#   ragged f32    rel 2.43e-6 (r16x9, Winograd)  edge 2.46e-6 (r16x9, Winograd)  abs 4.04e-5 (r3x171, Winograd)
#          f16x3  rel 1.54e-6 (r1x193)           edge 1.44e-6 (r5x13)            abs 2.11e-5 (r2x128)
#          f16    rel 8.01e-4 (r1x193)           edge 7.60e-4 (r5x77)            abs 1.08e-2 (r2x128)
#   packed f32    rel 2.04e-6 (p193, Winograd)   edge 2.35e-6 (p175, Winograd)   abs 3.91e-5 (p383, Winograd)
#          f16x3  rel 1.55e-6 (p383)             edge 1.44e-6 (p108)             abs 2.27e-5 (p193)
#          f16    rel 8.04e-4 (p175)             edge 7.67e-4 (p108)             abs 1.08e-2 (p383)
# (flows 7 and 3 from the GPU's own state: f32 2.23e-6 / 2.27e-6 / 3.31e-5, f16x3 1.54e-6 / 1.44e-6 / 2.03e-5, f16 8.05e-4 /
# 7.60e-4 / 1.07e-2.)  No bound is new: a masked row is held to what the unmasked matrix is held to.
# fp32 and f16x3 bounds: about 10x those (the fp32 'rel' bound is tests/test_waveglow_gpu.py's ACTS_REL_TOL).  The fp16
# error is the rounding of the operands themselves, the same in every run (rel 5.8e-4 - 8.0e-4 over every fp16 probe): its
# bounds are 2.5x the worst, 10x would pass errors that are large for an fp16 product.
ACTS_REL = {'f32': 2e-5, 'f16x3': 1.6e-5, 'f16': 2e-3}
ACTS_ABS = {'f32': 6.5e-4, 'f16x3': 2.7e-4, 'f16': 3e-2}
ACTS_EDGE_REL = {'f32': 2.5e-5, 'f16x3': 1.5e-5, 'f16': 2e-3}
# ... and fp16 activations must be FAR from the fp32 result, or the precision flag was ignored: an fp32 run is within
# ACTS_REL['f32'] of the oracle, 10x below this floor; fp16-rounded operands land 3x above it (oracle-only control).
F16_FLOOR = 2e-4
# Flow state right after a flow (affine coupling, inverse 1x1 conv, early outputs) against the float64 oracle's
# intermediates, on weights with end_scale = 0.2: relative RMS ('rel') and max abs / max |reference| ('max_rel').
# Measured worst over flows 11, 8, 4, 0 (after flow 0 in every precision): f32 1.48e-6 / 1.78e-6, f16x3 1.77e-6 / 2.18e-6,
# f16 8.41e-4 / 1.19e-3.  Bounds 10x (fp16: 2.5x); a 1e-4 relative error of the `end` conv output moves the state after
# flow 11 by 4.0e-5 / 6.3e-5 already (oracle-only control).
# With row lengths, per row: f32 2.13e-6 / 2.87e-6 (p14, r5x13), f16x3 1.78e-6 / 3.29e-6 (p108), f16 9.58e-4 / 2.13e-3 (r5x13;
# a one-frame row's maximum over 32 positions); and exactly 0 on every frame that is not real.
STATE_REL = {'f32': 1.5e-5, 'f16x3': 1.8e-5, 'f16': 2.5e-3}
STATE_MAX_REL = {'f32': 1.8e-5, 'f16x3': 2.2e-5, 'f16': 3e-3}
STATE_END_SCALE = 0.2

PRECISIONS = ('f32', 'f16', 'f16x3')
FORMS = {'direct': 0, 'winograd': 1, 'winograd-3pass': 2, 'winograd-prepass': 3}    # tts_hip_set_waveglow_form
WINO_MIN_FRAMES = 144        # wg_plan.h TTS_WINO_MIN_FRAMES
NPH = 32                     # sample groups (positions) per mel frame
N_LAYERS = 8


# ---- dispatch rules ----------------------------------------------------------------------------------------------------
class Variant(NamedTuple):
    tiles: str                  # '64-row' | '128x64' | '128-row' | '256-row'  (tts_hip_last_waveglow_tiles)
    wino: bool                  # layers 1 - 7 in their Winograd form (tts_hip_last_waveglow_form == 1)
    PR: int                     # rows per phase block
    kernels: frozenset          # 'gemm_wn_*' wrappers (with their bool argument), Winograd kernels as 'name/group kind'
    groups: Optional[tuple] = None      # Winograd form: (frame group rows, mixed group rows) per block


def _up(n, m):
    return (n + m - 1) // m * m


def frame_groups_per_utt(T):
    return (T + 15) // 16 * 4                                   # wn_wino.hip frame_groups_per_utt


def mixed_groups_per_utt(T):
    return (T + 1) // 2                                         # wn_wino.hip mixed_groups_per_utt


def group_rows(B, T, form):
    # wn_wino.hip group_row_tile, frame_group_rows, mixed_group_rows: padded to 64 rows (fused kernels) or 128
    # (form 2's GEMM)
    g = 128 if form == 2 else 64
    return _up(B * frame_groups_per_utt(T), g), _up(B * mixed_groups_per_utt(T), g)


WINO_KINDS = ('phases', 'mixed', 'frames')      # layers 1 - 3 (d <= 8), 4 (d = 16), 5 - 7 (d >= 32); waveglow_wino_layer


def pick_variant(B, T, precision, form='winograd') -> Variant:
    """The kernels `waveglow_run` runs for B x T frames in `precision` under waveglow form `form` (only fp32 has forms)."""
    BT = B * T
    half, x3 = precision == 'f16', precision == 'f16x3'
    fm = FORMS[form]
    # wg_plan: 128-row tiles when they save 5 % of the rows; 64-row tiles for short calls (fp16: from -25 %
    # rows; split fp16: 64 x 128 vs 256 x 256, from pr64 * 1.25 < pr256)
    pr256, pr128, pr64 = _up(BT, 256), _up(BT, 128), _up(BT, 64)
    tile128 = pr128 * 1.05 < pr256
    pr_big = pr128 if tile128 else pr256
    if x3:
        row64 = pr64 * 1.25 < pr256
    else:
        row64 = BT <= 512 and (pr64 * 4 <= pr_big * 3 if half else pr64 < pr_big)
    # wg_plan: Winograd from 144 fp32 frames; form 2 needs 128-row phase blocks and leaves the 64-row tiles when that pays
    wino_size = precision == 'f32' and fm >= 1 and BT >= WINO_MIN_FRAMES
    if wino_size and fm == 2 and row64 and pr128 * 1120.0 * 1.35 < pr64 * 1856.0:
        row64 = False
    PR = pr64 if row64 else pr128 if tile128 and not x3 else pr256         # wg_plan: PR
    tile64 = not row64 and tile128 and (NPH * PR // 128) * 8 < 768         # wg_plan: tile64
    wino = wino_size and (not row64 or fm != 2)                            # wg_plan: wino_wanted
    tiles = '64-row' if row64 else '256-row' if x3 else '128x64' if tile64 else '128-row' if tile128 else '256-row'  # tiles
    if x3:                                                                 # kWnKernels, split fp16 rows
        k = {f'gemm_wn_in0_x3(small={row64})', f'gemm_wn_in_x3(small={row64})', f'gemm_wn_res_x3(small={row64})'}
    elif half:                                                             # kWnKernels, fp16 rows
        if row64:
            k = {'gemm_wn_in0_r64h', 'gemm_wn_in_r64h', 'gemm_wn_res_r64h'}
        elif tile64:
            k = {'gemm_wn_in0_64h', 'gemm_wn_in_64h', 'gemm_wn_res_64h'}
        else:
            k = {f'gemm_wn_in0_h(t128={tile128})', f'gemm_wn_in_h(t128={tile128})', 'gemm_wn_res_h'}
    else:                                                                  # kWnKernels, fp32 rows
        suf = '_r64' if row64 else '_64' if tile64 else '_128' if tile128 else ''
        k = {'gemm_wn_in0' + suf, 'gemm_wn_res' + (suf if row64 or tile64 else '_skip')}
        if not wino:
            k.add('gemm_wn_in' + suf)
    k.add('wn_end_fold_kernel<%s>' % ('true, true' if x3 else 'true, false' if half else 'false, false'))   # launch_end_fold
    groups = None
    if wino:
        groups = group_rows(B, T, fm)
        if fm == 1:                                                        # waveglow_wino_layer: the fused kernel
            k |= {f'fused2/{g}' for g in WINO_KINDS}
        elif fm == 3:                                                      # ... the same behind the pre-pass
            k |= {f'fused_prepass/{g}' for g in WINO_KINDS}
        else:                                                              # ... three GEMMs, then the combine pass
            k |= {'gemm_wn_wino/phases' if PR % 256 == 0 else 'gemm_wn_wino_128/phases', 'gemm_wn_wino_128/mixed',
                  'gemm_wn_wino_128/frames', 'combine'}
    return Variant(tiles, wino, PR, frozenset(k), groups)


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    B: int
    T: int
    forms: tuple = ('winograd',)        # fp32 forms run; f16 / f16x3 run once (they have no Winograd form)
    seed: int = 0

    @property
    def BT(self):
        return self.B * self.T


_ALL = ('winograd', 'direct', 'winograd-3pass', 'winograd-prepass')
_C = Case
CASES = (
    # utterances shorter than the d = 64 / 128 reach (1 - 3 frames = 32 - 96 positions): taps cross utterance ends
    _C('t1_b5', 5, 1), _C('t2_b7', 7, 2), _C('t3_b4', 4, 3),
    # 64 frames: the largest 64-row call of every precision, no padding; 65: 128 x 64 tiles (fp32, fp16), padded by 63
    _C('b1_t64', 1, 64), _C('b5_t13', 5, 13),
    # the Winograd start: 143 frames direct, 144 Winograd (T odd and not a multiple of 16: partial frame and mixed groups),
    # 150 utterances of one frame in the Winograd form; form 2 keeps 64-row tiles here, i.e. the direct form
    _C('b11_t13', 11, 13), _C('b16_t9', 16, 9, _ALL), _C('b150_t1', 150, 1, ('winograd', 'winograd-prepass')),
    # fp16 pr64 * 4 <= pr_big * 3: 192 frames equal (64-row), 193 not (256 x 256); 193: split fp16's 256 x 256 tiles
    _C('b3_t64', 3, 64), _C('b1_t193', 1, 193, ('winograd', 'direct')),
    # 256-row tiles everywhere: 255 frames (phase blocks padded by one row), 256 (form 2: PR % 256 == 0 -> gemm_wn_wino)
    _C('b5_t51', 5, 51, ('winograd', 'direct', 'winograd-prepass')), _C('b2_t128', 2, 128, _ALL),
    # 257 frames: fp32 64-row (padded by 63), fp16 128-row (padded by 127)
    _C('b1_t257', 1, 257, ('winograd', 'direct')),
    # 300 frames: form 2's row-64 rescue (128-row blocks, PR % 256 != 0 -> gemm_wn_wino_128), fp16 128-row
    _C('b4_t75', 4, 75, _ALL),
    # 383 frames: fp32 128-row tiles padded by one row (tile-64 rule false: 96 blocks * 8 = 768), split fp16 64-row at
    # 480 < 512; 385: split fp16 256 x 256, fp32 64-row (448 rows)
    _C('b1_t383', 1, 383, ('winograd', 'direct')), _C('b5_t77', 5, 77),
    # the row-64 limit: 512 frames (256-row) / 513 (128-row, 640 rows per phase: padded by 127)
    _C('b4_t128', 4, 128), _C('b3_t171', 3, 171, _ALL),
)
CASE_BY_NAME = {c.name: c for c in CASES}
# flows 7 and 3 (n_half 3 and 4), compared from the GPU's own flow input, and the post-flow state (end_scale 0.2 weights)
LATER_FLOW_CASES = ('t3_b4', 'b5_t13', 'b16_t9')
STATE_CASES = ('t3_b4', 'b5_t13')


def runs(case):
    """[(precision, form)] of one case."""
    return [('f32', f) for f in case.forms] + [('f16', 'winograd'), ('f16x3', 'winograd')]


# ---- cases with row lengths --------------------------------------------------------------------------------------------
# Ragged (`lengths=`) and packed (`packed=True`) calls take the MASK_LENS / MASK_FLAGS instantiation of every position-wise
# kernel, wn_zero_tail_kernel behind the start conv and every residual GEMM, the cleared mel copy and (packed) the gather.
# A ragged call is one run of B x T frames; a packed call one row of F frames (packing_plan): `pick_variant(B, T, ..)` and
# `pick_variant(1, F, ..)` say what they take.  Every row goes against the oracle on ITS OWN frames (mel[b:b+1, :n],
# z[b:b+1, :n*32]: the contract of tts_hip_waveglow_infer_ragged), with the row's own ends as edge windows.
GAP = 4                      # include/tts_hip.h TTS_HIP_WG_GAP_FRAMES (tests/test_waveglow_packed.py compares)


class RowsCase(NamedTuple):
    name: str
    B: int
    T: int
    lengths: tuple
    forms: tuple = ('winograd',)
    packed: bool = False

    @property
    def starts(self):
        """First frame of every row in the probe's output: b * T in the batch layout, the packing plan's in the packed row."""
        if not self.packed:
            return tuple(b * self.T for b in range(self.B))
        from waveglow_packed_ref import packing_plan
        return tuple(packing_plan(self.lengths, self.T, GAP)['starts'])

    @property
    def frames(self):
        """Frames of the one run: B * T, or F of the packed row."""
        if not self.packed:
            return self.B * self.T
        rows = sum(n > 0 for n in self.lengths)
        return sum(self.lengths) + GAP * max(rows - 1, 0)

    @property
    def run_shape(self):
        return (1, self.frames) if self.packed else (self.B, self.T)


def _ragged(B, T, lengths, forms=('winograd',)):
    assert len(lengths) == B and max(lengths) <= T
    return RowsCase(f'r{B}x{T}', B, T, tuple(lengths), forms, False)


def _packed(lengths, forms=('winograd', 'direct'), T=None):
    c = RowsCase('', len(lengths), max(lengths) if T is None else T, tuple(lengths), forms, True)
    return c._replace(name=f'p{c.frames}')


RAGGED_CASES = (
    # 64-row in every precision; rows shorter than the d = 64 / 128 reach, and an empty row
    _ragged(4, 3, (3, 1, 0, 2)),
    # 65 frames: 128 x 64 tiles for fp32 and fp16; split fp16 64-row, padded by 63
    _ragged(5, 13, (13, 5, 9, 1, 12)),
    # 144 frames, the Winograd start on 64-row tiles (PR 192); lengths that split frame groups of 16 and mixed groups of 2
    _ragged(16, 9, (9, 0, 1, 8, 3, 9, 2, 7, 4, 9, 5, 6, 9, 1, 0, 9), _ALL),
    # 256-row, fp16 and split fp16 256 x 256; a tail inside the one row
    _ragged(1, 193, (150,), ('winograd', 'direct')),
    # 256 frames, no padding rows; form 2 takes gemm_wn_wino
    _ragged(2, 128, (128, 50), _ALL),
    # 300 frames: fp32 64-row PR 320; form 2 and fp16 128-row PR 384
    _ragged(4, 75, (75, 0, 31, 74), _ALL),
    # 385 frames: fp32 64-row PR 448; fp16 and split fp16 256-row PR 512
    _ragged(5, 77, (77, 40, 1, 76, 33)),
    # 513 frames: fp32 and fp16 128-row PR 640, padded by 127; split fp16 64-row PR 576
    _ragged(3, 171, (171, 100, 37), _ALL),
)
PACKED_CASES = (
    # F = 14, 64-row; T = 300, well above every length: the gather's source index b * T + t is not the packed index
    _packed((3, 0, 1, 2), T=300),
    _packed((30, 1, 45, 20)),                 # F = 108, 128 x 64
    _packed((100, 37, 30)),                   # F = 175, Winograd on 64-row; the oracle rows of tests/test_waveglow_packed_gpu.py
    _packed((120, 1, 64)),                    # F = 193, 256-row; a one-frame row between two gaps
    _packed((200, 77, 98)),                   # F = 383, 128-row padded by one
    _packed((171, 100, 37, 193)),             # F = 513, 128-row PR 640
    # added for the coverage test's rule "a row of length T and one of T - 1 in every table" (above, T is max(lengths) and no
    # row has T - 1 frames, or T = 300): F = 9, 64-row
    _packed((2, 3)),
)
ROWS_CASES = RAGGED_CASES + PACKED_CASES
ROWS_CASE_BY_NAME = {c.name: c for c in ROWS_CASES}
assert len(ROWS_CASE_BY_NAME) == len(ROWS_CASES)
# flows 7 and 3 (the a0p rows of 3 and 4 coupling channels and their constant-1 column, which zero_tail(.., with_a0p) clears)
ROWS_LATER_FLOW_CASES = ('r4x3', 'r5x13', 'r16x9', 'p14', 'p175')
ROWS_STATE_CASES = ('r4x3', 'r5x13', 'p14', 'p108')
ROWS_COND_CASES = ('r16x9', 'r3x171', 'p175', 'p513')
ROWS_256_CASES = ('r4x3', 'p14')             # on a 256-channel handle, fp32: end_fold<false, false, MASK_*>


def rows_variant(case, precision, form='winograd'):
    return pick_variant(*case.run_shape, precision, form)


def mask_kernels(case, precision, channels=512):
    """The MASK_LENS / MASK_FLAGS instantiations of the position-wise kernels a call with lengths launches (waveglow_run):
    init_audio_kernel, and at every flow's end wn_end_last_kernel (fp32 at 512 channels, on the residual GEMMs' partial sums)
    or end_fold<HALF, SPLIT, ..>."""
    m = 'MASK_FLAGS' if case.packed else 'MASK_LENS'
    if precision == 'f32' and channels == 512:
        end = f'wn_end_last_kernel<{m}>'
    else:
        end = 'end_fold<%s, %s>' % ('true, true' if precision == 'f16x3' else 'true, false' if precision == 'f16' else
                                    'false, false', m)
    return {f'init_audio_kernel<{m}>', end}


def rows_inputs(case, nan=True):
    """(mel [B, T, 80], z [B, T*32, 8]) by the recipe of `inputs`, seeded by the case; behind every length NaN (no reference
    may depend on it), or with nan=False the recipe's own values (the oracle-only controls, where a leak must show as a number)."""
    rng = np.random.default_rng(900 + 7 * case.B + case.T + 1000 * sum(case.lengths) + case.packed)
    mel = rng.uniform(-11.5, 1.2, (case.B, case.T, 80)).astype(np.float32)
    z = rng.standard_normal((case.B, case.T * NPH, 8)).astype(np.float32)
    if nan:
        for b, n in enumerate(case.lengths):
            mel[b, n:] = np.nan
            z[b, n * NPH:] = np.nan
    return mel, z


def row_inputs(case, b):
    """Row b's own frames: (mel [1, n, 80], z [1, n*32, 8])."""
    mel, z = rows_inputs(case)
    n = case.lengths[b]
    return np.ascontiguousarray(mel[b:b + 1, :n]), np.ascontiguousarray(z[b:b + 1, :n * NPH])


def row_of(case, out, b):
    """Row b's real positions [1, n*32, W] of a probe's output: [B, T*32, W] (ragged) or [F*32, W] (packed)."""
    n = case.lengths[b]
    if case.packed:
        at = case.starts[b] * NPH
        return out[None, at:at + n * NPH]
    return out[b:b + 1, :n * NPH]


def not_real(case, out):
    """Every position of a probe's output that belongs to no real frame: behind the lengths, or on the gap frames."""
    real = np.zeros(case.frames * NPH, bool)
    for b, n in enumerate(case.lengths):
        real[case.starts[b] * NPH:(case.starts[b] + n) * NPH] = True
    return out.reshape(case.frames * NPH, -1)[~real]


def inputs(case):
    """(mel [B, T, 80], z [B, T*32, 8]) float32, the value ranges of tests/test_waveglow_gpu.py."""
    rng = np.random.default_rng(500 + 7 * case.B + case.T + case.seed)
    mel = rng.uniform(-11.5, 1.2, (case.B, case.T, 80)).astype(np.float32)
    z = rng.standard_normal((case.B, case.T * NPH, 8)).astype(np.float32)
    return mel, z


# ---- oracle ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def config():
    from text_to_speech_amd.config import WaveGlowConfig
    return WaveGlowConfig()


@functools.lru_cache(maxsize=None)
def weights(end_scale=None):
    """The session weights (seed 1234, the GPU tests' `gpu_engine`), or the same seed with another `end` conv scale."""
    from text_to_speech_amd import weights as wmod
    if end_scale is None:
        return wmod.synth_waveglow(config(), seed=1234)
    return wmod.synth_waveglow(config(), seed=1234, end_scale=end_scale)


@functools.lru_cache(maxsize=None)
def weights64(end_scale=None):
    return {k: np.asarray(v, np.float64) for k, v in weights(end_scale).items() if k.startswith('waveglow/')}


def spect_of(mel, w):
    from oracle import waveglow_ref
    return waveglow_ref.regroup(waveglow_ref.upsample(np.asarray(mel, np.float64), w['waveglow/upsample/kernel'],
                                                      w['waveglow/upsample/bias'], config().upsample_stride), config().n_group)


def n_half_of(flow):
    return 2 if flow >= 8 else 3 if flow >= 4 else 4


def flow_acts(a0, spect, flow, w=None, stop_after=N_LAYERS - 1):
    """The gated activations of the WN layers of flow `flow` on its input a0 [B, L, n_half], float64."""
    from oracle import waveglow_ref
    w = weights64() if w is None else w
    acts = []
    waveglow_ref.wn_block(np.asarray(a0, np.float64), spect, w, f'waveglow/block-{flow}', N_LAYERS, 512, collect=acts,
                          stop_after=stop_after)
    return acts


@functools.lru_cache(maxsize=None)
def _flow11_acts(name):
    mel, z = inputs(CASE_BY_NAME[name])
    return tuple(flow_acts(z[:, :, :n_half_of(11)], spect_of(mel, weights64()), 11))


def flow11_acts(case):
    """Oracle activations of the 8 layers of flow 11 (input sigma * z, sigma = 1), cached per process."""
    return _flow11_acts(case.name)


@functools.lru_cache(maxsize=None)
def _states(name, end_scale):
    from oracle import waveglow_ref
    mel, z = inputs(CASE_BY_NAME[name])
    _, inter = waveglow_ref.infer(mel.astype(np.float64), weights(end_scale), config(), z=z.astype(np.float64), sigma=1.0,
                                  dtype=np.float64, return_intermediates=True)
    return {k: inter[f'audio_after_flow_{k}'] for k in (11, 8, 4, 0)}


def states(case, end_scale=STATE_END_SCALE):
    """Oracle flow state after flows 11, 8, 4 and 0 (float64), cached per process."""
    return _states(case.name, end_scale)


@functools.lru_cache(maxsize=None)
def _row_flow11_acts(name, b):
    mel, z = row_inputs(ROWS_CASE_BY_NAME[name], b)
    return tuple(flow_acts(z[:, :, :n_half_of(11)], spect_of(mel, weights64()), 11))


def row_flow11_acts(case, b):
    """Oracle activations of the 8 layers of flow 11 of row b ALONE (its own frames), cached per (case, row)."""
    return _row_flow11_acts(case.name, b)


@functools.lru_cache(maxsize=None)
def _row_states(name, b, end_scale):
    from oracle import waveglow_ref
    mel, z = row_inputs(ROWS_CASE_BY_NAME[name], b)
    _, inter = waveglow_ref.infer(mel.astype(np.float64), weights(end_scale), config(), z=z.astype(np.float64), sigma=1.0,
                                  dtype=np.float64, return_intermediates=True)
    return {k: inter[f'audio_after_flow_{k}'] for k in (11, 8, 4, 0)}


def row_states(case, b, end_scale=STATE_END_SCALE):
    """Oracle flow state of row b ALONE after flows 11, 8, 4 and 0 (float64), cached per (case, row)."""
    return _row_states(case.name, b, end_scale)


# ---- metrics -----------------------------------------------------------------------------------------------------------
def _rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def edge_mask(T, d):
    """Positions of one utterance within d of either end (all of them when the utterance is shorter than 2 d)."""
    l = np.arange(T * NPH)
    return (l < d) | (l >= T * NPH - d)


def act_errors(out, ref, T, d):
    err = np.asarray(out, np.float64) - ref
    m = edge_mask(T, d)
    return {'rel': _rms(err) / _rms(ref), 'abs': float(np.abs(err).max()),
            'edge': _rms(err[:, m]) / _rms(ref[:, m])}


def act_failures(e, precision, tag):
    out = []
    for k, bound in (('rel', ACTS_REL), ('abs', ACTS_ABS), ('edge', ACTS_EDGE_REL)):
        if not e[k] <= bound[precision]:
            out.append(f'{tag}: {k} {e[k]:.3e} > {bound[precision]:.1e}')
    if precision == 'f16' and not e['rel'] >= F16_FLOOR:
        out.append(f'{tag}: fp16 activations within {e["rel"]:.2e} of the fp32 oracle (< {F16_FLOOR:.0e}): flag ignored?')
    return out


def state_errors(out, ref):
    err = np.asarray(out, np.float64) - ref
    return {'rel': _rms(err) / _rms(ref), 'max_rel': float(np.abs(err).max() / np.abs(ref).max())}
