"""Cases and float64 oracle pieces of the end-partial-sum tests (tests/test_wn_end_partials.py on the CPU, _gpu.py on an MI355X).

The fp32 path of a 512-channel model forms the folded skip / `end` conv of a flow in three parts: the residual GEMMs of
layers 0 .. 6 each add their layer's eight partial sums to endp [M][8] (csrc/gemm_f32.h, GemmArgs::end_sums), and
wn_end_last_kernel (csrc/waveglow.hip) adds layer 7 and the bias:

    end(sum_i skip_i) = sum_{i<7} acts_i @ (Ws_i @ We)  +  acts_7 @ (Ws_7 @ We)  +  ((sum_i bs_i) @ We + be)

The cases name one call per residual tile family and form; `state11` restates the split in float64 from the oracle's
gated activations of flow 11, which do not depend on the `end` scaling, so the cached `waveglow_cases.flow11_acts` serve.
"""
import numpy as np

import waveglow_cases as wc

C = 512
# (case, form, residual tile family, flows whose state is compared).  The oracle of all twelve flows is affordable for the
# two small cases only; the large ones compare the state after flow 11, whose input is z itself.
STATE_RUNS = (
    ('b5_t13', 'direct', '128x64', (11, 8, 4, 0)),        # 65 frames; h = 2, 3, 4 and 8 N tiles per M tile
    ('b16_t9', 'winograd', '64-row', (11, 8, 4, 0)),      # 144 frames; two wave columns split a block's outputs
    ('b1_t383', 'winograd', '128-row', (11,)),            # 128 x 128 tiles, three blocks per CU
    ('b1_t383', 'direct', '128-row', (11,)),
    ('b2_t128', 'winograd', '256-row', (11,)),            # the same residual kernel on 256-row phase blocks
)
ACTS_RUNS = (('b5_t13', 'direct'), ('b16_t9', 'winograd'))


def end_parts(acts, w, prefix='waveglow/block-11'):
    """(partials [7][B, L, n], layer 7's part [B, L, n], bias [n]) of the folded skip / `end` conv, float64: the three kinds
    of term the GPU adds up.  acts: the 8 layers' gated activations; w: float64 weights."""
    we, be = w[f'{prefix}/end_conv/kernel'][0], w[f'{prefix}/end_conv/bias']
    parts, bias = [], be.copy()
    for i in range(wc.N_LAYERS):
        k, b = w[f'{prefix}/res_skip_conv-{i}/kernel'][0], w[f'{prefix}/res_skip_conv-{i}/bias']
        ks, bs = (k[:, C:], b[C:]) if i < wc.N_LAYERS - 1 else (k, b)      # layer 7 has no residual half
        parts.append(np.asarray(acts[i], np.float64) @ (ks @ we))
        bias = bias + bs @ we
    return parts[:7], parts[7], bias


def coupling11(end_out, z, w):
    """The state after flow 11 from its `end` conv output [B, L, 4] and the call's z: affine coupling on the first four z
    channels, then the inverse 1x1 conv (oracle/waveglow_ref.py `infer`, k = 11: no early output)."""
    from oracle import waveglow_ref
    a = np.asarray(z, np.float64)[:, :, :4]
    a0, a1 = a[:, :, :2], a[:, :, 2:]
    a1 = (a1 - end_out[:, :, :2]) / np.exp(end_out[:, :, 2:])
    inv = waveglow_ref.inv1x1_reverse_matrix(w['waveglow/invertible_conv-11/conv/kernel'])
    return np.concatenate([a0, a1], axis=2) @ inv


def state11(case, drop=None):
    """Float64 state after flow 11 on the end_scale = 0.2 weights, as the sum of the three kinds of term; `drop`: leave out
    that layer's partial (the failure the state bound has to see)."""
    w = wc.weights64(wc.STATE_END_SCALE)
    _, z = wc.inputs(case)
    partials, last, bias = end_parts(wc.flow11_acts(case), w)
    total = sum(p for i, p in enumerate(partials) if i != drop)
    return coupling11(total + last + bias, z, w)
