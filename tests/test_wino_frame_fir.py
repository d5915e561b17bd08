"""The frame-axis F(4,2) conditioning of the dilation-32 / 64 WN layers (csrc/wn_wino.hip, frame groups with s = 1, 2),
restated in numpy / float64 and checked against the direct sum_q V_q mel[t - q].

The four outputs of a frame group are the frames t0 + j s of one phase and share its weights; the conditioning's four taps
split into two halves of two taps s frames apart, each an F(4, 2) problem whose five products are added into the tap
products at the points 0, 1, -1, 2, -2 and pass through the unchanged output transform.  The transform constants and the
chunk bookkeeping are read from the HIP source, so that a change there is checked here."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'text_to_speech_amd', 'csrc')
NMEL, KMEL, KF = 80, 320, 160
# output transform of the F(4,3) epilogue (products 0 .. 5 = points 0, 1, -1, 2, -2, infinity)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], float)


def _src():
    with open(os.path.join(CSRC, 'wn_wino.hip')) as f:
        return f.read()


def _const_array(name):
    """A `__constant__ double NAME[...] = {...};` of wn_wino.hip as a float array (entries like -5. / 4)."""
    m = re.search(r'__constant__ double ' + name + r'((?:\[\d+\])+) = (\{.*?\});', _src(), re.S)
    assert m, name
    shape = [int(n) for n in re.findall(r'\[(\d+)\]', m.group(1))]
    vals = [float(Fraction(a.strip().rstrip('.')) / Fraction(b.strip().rstrip('.')) if b else Fraction(a.strip().rstrip('.')))
            for a, b in re.findall(r'(-?\s*[\d.]+)\s*(?:/\s*([\d.]+))?', m.group(2).replace('{', ' ').replace('}', ' '))]
    return np.array(vals).reshape(shape)


X = _const_array('FIR_X')
FIR_BT = _const_array('FIR_BT')


def fir_qb(s, half):                      # the older tap of a half (fir_qb in wn_wino.hip); the newer one is qb - s
    return 2 * half + 1 if s == 1 else half + 2


def frame_groups_per_utt(T):
    return (T + 15) // 16 * 4


def groups(T, s):
    """(t0, frames t0 + j s < T) of the frame groups of one utterance (frame_group in wn_wino.hip; empty groups skipped)."""
    out = []
    for g in range(frame_groups_per_utt(T)):
        t0 = (g // s) * 4 * s + g % s
        if t0 < T:
            out.append(t0)
    return out


def direct(mel, V, s):
    """cond[t] = sum_q V_q mel[t - q] (zero before the utterance), per utterance: mel [T][80], V [4][80][N] -> [T][N]."""
    T = mel.shape[0]
    out = np.zeros((T, V.shape[2]))
    for t in range(T):
        for q in range(4):
            if t - q >= 0:
                out[t] += mel[t - q] @ V[q]
    return out


def weight_planes(V, s):
    """wino4_cond_weights_fir_kernel: product k, column half * 80 + c: V_qb + x_k V_qa -> [5][160][N]."""
    planes = np.zeros((5, KF, V.shape[2]))
    for k in range(5):
        for half in range(2):
            qb = fir_qb(s, half)
            planes[k, half * NMEL:(half + 1) * NMEL] = V[qb] + X[k] * V[qb - s]
    return planes


def mel_planes(mel, s, t0):
    """wino4_mel_planes_fir_kernel for one group: sum_i FIR_BT[k][i] z_i, z_i = mel[t0 - qb + i s] inside the utterance."""
    T = mel.shape[0]
    out = np.zeros((5, KF))
    for half in range(2):
        qb = fir_qb(s, half)
        z = np.array([mel[t] if 0 <= t < T else np.zeros(NMEL) for t in (t0 - qb + i * s for i in range(5))])
        out[:, half * NMEL:(half + 1) * NMEL] = FIR_BT @ z
    return out


def wino_cond(mel, V, s):
    """Conditioning of every frame of one utterance through the products and the F(4,3) output transform."""
    T = mel.shape[0]
    W = weight_planes(V, s)
    out = np.full((T, V.shape[2]), np.nan)
    for t0 in groups(T, s):
        m = mel_planes(mel, s, t0)
        P = np.zeros((6, V.shape[2]))
        P[:5] = np.einsum('kc,kcn->kn', m, W)              # product 5 (infinity) carries no conditioning
        y = AT @ P
        for j in range(4):
            if t0 + j * s < T:
                out[t0 + j * s] = y[j]
    return out


def test_transform_is_f42_at_points_0_pm1_pm2():
    """FIR_BT is the inverse transpose of the Vandermonde matrix at the five points, so that the output transform's columns
    [1, x, x^2, x^3] of products 0 .. 4 give back the 2-tap correlation y_j = h0 z_j + h1 z_{j+1}."""
    assert list(X) == [0, 1, -1, 2, -2]
    assert np.allclose(AT[:, :5], np.vander(X, 4, increasing=True).T)
    Vd = np.vander(X, 5, increasing=True)
    assert np.allclose(FIR_BT, np.linalg.inv(Vd).T, atol=1e-15)
    rng = np.random.default_rng(1)
    z, h0, h1 = rng.standard_normal(5), rng.standard_normal(), rng.standard_normal()
    y = AT[:, :5] @ ((h0 + X * h1) * (FIR_BT @ z))
    assert np.allclose(y, h0 * z[:4] + h1 * z[1:], atol=1e-13)


def test_halves_cover_the_four_taps_once():
    for s in (1, 2):
        taps = sorted(q for half in range(2) for q in (fir_qb(s, half), fir_qb(s, half) - s))
        assert taps == [0, 1, 2, 3], s


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('lengths', [[1], [2], [5], [16], [17], [31], [64], [3, 9, 40], [23, 16, 7, 61]])
def test_fir_products_reproduce_the_direct_conditioning(s, lengths):
    """Utterance starts (frames before t0 - 3), ends and partial groups (outputs past T not written, frames past T zero), and
    batches of mixed lengths: every utterance is cut into its own frame groups, so its conditioning is its own."""
    rng = np.random.default_rng(100 * s + sum(lengths))
    V = rng.standard_normal((4, NMEL, 24)) / np.sqrt(KMEL)
    for T in lengths:
        mel = rng.uniform(-11.5, 1.2, (T, NMEL))
        ref = direct(mel, V, s)
        got = wino_cond(mel, V, s)
        assert not np.isnan(got).any()                     # every frame is an output of exactly one group
        assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max(), (s, T)


def test_frames_past_the_end_do_not_reach_written_outputs():
    """Garbage in a frame past the utterance end (the next utterance's mel in the batched layout) changes no written output:
    the mel planes read those frames as zero, and in exact arithmetic only outputs past T would see them anyway."""
    rng = np.random.default_rng(5)
    V = rng.standard_normal((4, NMEL, 8))
    for s in (1, 2):
        for T in (5, 18, 33):
            mel = rng.standard_normal((T, NMEL))
            W = weight_planes(V, s)
            for t0 in groups(T, s):
                for half in range(2):
                    qb = fir_qb(s, half)
                    beyond = [i for i in range(5) if t0 - qb + i * s >= T]
                    # output j uses z_j and z_{j+1}: a frame past T serves only outputs j >= i - 1 with t0 + j s >= T
                    for i in beyond:
                        for j in (i - 1, i):
                            if 0 <= j < 4:
                                assert t0 + j * s >= T
            assert np.isfinite(wino_cond(mel, V, s)).all() and W.shape == (5, KF, 8)


def _frame_ccfg():
    """The ccfg words that waveglow_wino_layer sets for the frame groups: (s = 1, 2 branch, s = 4 branch), each [6] ints."""
    src = _src()
    consts = {n: int(v) for n, v in re.findall(r'\b(K4|SA|SB|SC|KF|KMEL)\s*=\s*(\d+)', src)}
    body = src[src.index('} else if (fir) {'):]
    fir_part = body[:body.index('} else {')]
    s4_part = body[body.index('} else {'):body.index('for (int p = 0; p < 6; ++p) (p < 4 ? a.cfg_lo')]

    def cc(n1, b1, n2=0, b2=0):
        assert 0 <= n1 < 32 and 0 <= b1 < 16 and 0 <= n2 < 8 and 0 <= b2 < 16      # the field widths of cfg
        return n1 | b1 << 5 | n2 << 9 | b2 << 12

    def run(part):
        ccfg = [0] * 6
        env = dict(consts, cc=cc, ccfg=ccfg)
        for stmt in re.findall(r'(?:for \(int p = (\d+); p < (\d+); \+\+p\) )?((?:ccfg\[\w+\] = )+cc\([^;]*\));', part):
            lo, hi, expr = stmt
            targets = re.findall(r'ccfg\[(\w+)\] = ', expr)
            value = eval(expr[expr.index('cc('):].replace('/', '//'), env)
            for p in (range(int(lo), int(hi)) if lo else [int(t) for t in targets]):
                ccfg[p] = value
        return ccfg

    return run(fir_part), run(s4_part), consts


def _chunks(c):
    return (c & 31) + ((c >> 9) & 7)


def test_chunk_bookkeeping_50_for_s1_s2_and_80_for_s4():
    fir, s4, k = _frame_ccfg()
    assert k['KF'] == KF and k['KMEL'] == KMEL
    assert [_chunks(c) for c in fir] == [10, 10, 10, 10, 10, 0] and sum(map(_chunks, fir)) == 50
    assert sum(map(_chunks, s4)) == 80
    # every weight chunk a product reads lies inside its plane's row (160 columns for s = 1, 2, cond_Bt's 320 for s = 4)
    for words, width in ((fir, KF), (s4, KMEL)):
        for c in words:
            n1, b1, n2, b2 = c & 31, (c >> 5) & 15, (c >> 9) & 7, c >> 12
            assert (b1 + n1) * 16 <= width and (n2 == 0 or (b2 + n2) * 16 <= width)
    # K steps per 64 x 128 tile of the fused kernel: 6 products x 32 tap chunks + the conditioning chunks
    assert 6 * 32 + sum(map(_chunks, s4)) == 272 and 6 * 32 + sum(map(_chunks, fir)) == 242
