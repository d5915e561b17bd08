"""The frame-axis F(4,4) conditioning plane of the Winograd WN layers (csrc/wn_wino.hip: wino_cond_weights_kernel,
wino_cond_mel_planes_kernel, wino_cond_kernel), restated with exact rationals and in numpy / float64.

For every phase and layer the conditioning is a 4-tap FIR along frames, cond[t] = sum_q V_q mel[t - q]; four consecutive
frames share seven mel frames and need seven products instead of sixteen.  The transform constants are read from the HIP
source, so that a change there is checked here."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'text_to_speech_amd', 'csrc')
NMEL = 80
POINTS = [Fraction(0), Fraction(1), Fraction(-1), Fraction(2), Fraction(-2), Fraction(1, 2), Fraction(-1, 2)]


def _const_array(name):
    """A `__constant__ double NAME[r][c] = {...};` of wn_wino.hip as rows of Fractions (entries like -21. / 4)."""
    with open(os.path.join(CSRC, 'wn_wino.hip')) as f:
        m = re.search(r'__constant__ double ' + name + r'\[(\d+)\]\[(\d+)\] = (\{.*?\});', f.read(), re.S)
    assert m, name
    rows, cols = int(m.group(1)), int(m.group(2))
    vals = [Fraction(a.replace(' ', '').rstrip('.')) / (Fraction(b.rstrip('.')) if b else 1)
            for a, b in re.findall(r'(-?\s*[\d.]+)\s*(?:/\s*([\d.]+))?', m.group(3).replace('{', ' ').replace('}', ' '))]
    assert len(vals) == rows * cols, name
    return [vals[r * cols:(r + 1) * cols] for r in range(rows)]


G = _const_array('C44_G')              # 7 x 4
BT = _const_array('C44_BT')            # 7 x 7
AT = [[a ** j for a in POINTS] for j in range(4)]      # 4 x 7: written out in wino_cond_kernel's epilogue


def _evaluation(k):
    return [[a ** j for j in range(k)] for a in POINTS]


def _inverse(m):
    n = len(m)
    a = [row[:] + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(m)]
    for c in range(n):
        p = next(r for r in range(c, n) if a[r][c] != 0)
        a[c], a[p] = a[p], a[c]
        a[c] = [v / a[c][c] for v in a[c]]
        for r in range(n):
            if r != c and a[r][c] != 0:
                a[r] = [x - a[r][c] * y for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


def test_constants_are_the_evaluation_matrices_of_the_seven_points():
    assert G == _evaluation(4)
    e7_inv = _inverse(_evaluation(7))
    assert BT == [[e7_inv[j][i] for j in range(7)] for i in range(7)]         # (E_7^-1)^T


def test_f44_identity_is_exact():
    """y_j = sum_q' g_q' d_(j + q') = (AT [(G g) . (BT d)])_j, in exact rationals."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        g = [Fraction(int(v)) for v in rng.integers(-9, 10, 4)]
        d = [Fraction(int(v), 7) for v in rng.integers(-50, 51, 7)]
        gg = [sum(G[x][q] * g[q] for q in range(4)) for x in range(7)]
        bd = [sum(BT[x][i] * d[i] for i in range(7)) for x in range(7)]
        y = [sum(AT[j][x] * gg[x] * bd[x] for x in range(7)) for j in range(4)]
        assert y == [sum(g[q] * d[j + q] for q in range(4)) for j in range(4)]


def test_output_transform_rows_as_the_kernel_writes_them():
    """The epilogue's sums: y0 = P0 + s12 + s34 + s56, y1 = d12 + 2 d34 + d56 / 2, y2 = s12 + 4 s34 + s56 / 4,
    y3 = d12 + 8 d34 + d56 / 8 with s / d the sums / differences of the products of a point pair."""
    P = [Fraction(v) for v in (3, -5, 7, 11, -13, 17, 19)]
    s12, d12, s34, d34, s56, d56 = P[1] + P[2], P[1] - P[2], P[3] + P[4], P[3] - P[4], P[5] + P[6], P[5] - P[6]
    want = [sum(AT[j][x] * P[x] for x in range(7)) for j in range(4)]
    assert want == [P[0] + s12 + s34 + s56, d12 + 2 * d34 + d56 / 2, s12 + 4 * s34 + s56 / 4, d12 + 8 * d34 + d56 / 8]


def _f(m):
    return np.array([[float(v) for v in row] for row in m])


def direct(mel, V):
    """cond[t] = sum_q V_q mel[t - q] (zero before the utterance): mel [T][80], V [4][80][N] -> [T][N]."""
    out = np.zeros((mel.shape[0], V.shape[2]))
    for t in range(mel.shape[0]):
        for q in range(4):
            if t - q >= 0:
                out[t] += mel[t - q] @ V[q]
    return out


def wino_cond(mel, V):
    """The kernels' route: weight planes W_x = sum_q G[x][3 - q] V_q, one group per four frames with the mel planes
    Z_x = sum_i BT[x][i] mel[t0 - 3 + i] (frames outside the utterance read as zero), outputs past T not written."""
    T = mel.shape[0]
    Gf, BTf, ATf = _f(G), _f(BT), _f(AT)
    W = np.einsum('xq,qcn->xcn', Gf[:, ::-1], V)
    out = np.full((T, V.shape[2]), np.nan)
    for g in range((T + 3) // 4):
        t0 = 4 * g
        d = np.array([mel[t] if 0 <= t < T else np.zeros(NMEL) for t in range(t0 - 3, t0 + 4)])
        y = ATf @ np.einsum('xc,xcn->xn', BTf @ d, W)
        for j in range(4):
            if t0 + j < T:
                out[t0 + j] = y[j]
    return out


@pytest.mark.parametrize('lengths', [[1], [2], [3], [4], [5], [9], [16], [131], [3, 9, 40], [23, 16, 7, 61]])
def test_groups_reproduce_the_direct_conditioning(lengths):
    """Utterance starts, partial last groups, utterances shorter than one group, and batches of mixed lengths: every
    utterance is cut into its own groups of four frames, every frame is an output of exactly one group."""
    rng = np.random.default_rng(sum(lengths))
    V = rng.standard_normal((4, NMEL, 24)) / np.sqrt(4 * NMEL)
    for T in lengths:
        mel = rng.uniform(-11.5, 1.2, (T, NMEL))
        ref, got = direct(mel, V), wino_cond(mel, V)
        assert not np.isnan(got).any()
        assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max(), T


def test_fp32_model_of_the_rounding():
    """fp32 operands (planes formed in fp64, rounded once), fp32 products accumulated in fp64 -- the operand rounding alone:
    the relative RMS error of the F(4,4) route stays within a few 1e-7 (the issue's model, with fp32 accumulation: 4.4e-7)."""
    rng = np.random.default_rng(11)
    V = (rng.standard_normal((4, NMEL, 64)) / np.sqrt(4 * NMEL)).astype(np.float32).astype(np.float64)
    mel = rng.uniform(-11.5, 1.2, (64, NMEL)).astype(np.float32).astype(np.float64)
    ref = direct(mel, V)
    Gf, BTf, ATf = _f(G), _f(BT), _f(AT)
    W = np.einsum('xq,qcn->xcn', Gf[:, ::-1], V).astype(np.float32).astype(np.float64)
    got = np.zeros_like(ref)
    for g in range(16):
        d = np.array([mel[t] if t >= 0 else np.zeros(NMEL) for t in range(4 * g - 3, 4 * g + 4)])
        Z = (BTf @ d).astype(np.float32).astype(np.float64)
        got[4 * g:4 * g + 4] = ATf @ np.einsum('xc,xcn->xn', Z, W).astype(np.float32)
    rel = np.sqrt(np.mean((got - ref) ** 2) / np.mean(ref ** 2))
    print(f'fp32 operand model: relative RMS {rel:.2e}')
    assert rel < 1e-6
