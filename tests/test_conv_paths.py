"""CPU half of the encoder / postnet convolution tests (tests/conv_cases.py): the dispatch rule restated by
`pick_conv_path` still matches the source, the case table reaches both paths of every conv at the row counts where the
rule switches, and every case could fail -- oracle-only controls showing that the regression bounds of
test_conv_paths_gpu.py would catch a tap leaking across a sequence end, padded rows stored as act(BN(0)), conv 5's masked
rows stored as 0, the mask rule t < len and reversed taps."""
import os
import re

import numpy as np
import pytest

import conv_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
MARGIN = 100                # a defect must exceed the GPU bound by this factor


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- the rule against the source ---------------------------------------------------------------------------------------
def test_source_constants_of_the_rule():
    taco, gemm, plan = _src('tacotron2.hip'), _src('gemm_f32.h'), _src('taco_decode.h')
    body = taco[taco.index('int conv_gemm('):]
    body = body[:body.index('\n}\n')]
    assert 'const long long tiles = (long long)((M + 63) / 64) * ((cv.cout + 63) / 64);' in body
    assert 'const size_t need = (size_t)5 * M * cv.cout;' in body
    assert 'if (tiles < 512 && scratch && need <= scratch_floats && cv.cout % 4 == 0) {' in body
    assert body.count('gemm_small(') == 2
    # gemm_small is the 64 x 64 tile: BM = WR * RT * 32, BN = WC * CT * 32 with WR = WC = 2, RT = CT = 1
    assert re.search(r'inline hipError_t gemm_small\(const GemmArgs& g, int bz, hipStream_t s\) \{ '
                     r'return launch_gemm<2, 2, 1, 1, 32, 1, TAG_GENERIC>\(g, bz, s\); \}', gemm)
    assert 'constexpr int BM = WR * RT * 32;' in gemm and 'constexpr int BN = WC * CT * 32;' in gemm
    assert cc.TILE_M == 2 * 1 * 32 and cc.TILE_N == 2 * 1 * 32 and cc.SPLIT_BELOW_TILES == 512
    # the scratch every caller sizes: 5 x min(rows, 32768) x 512 floats, written in one function ...
    sizing = 'inline size_t conv_scratch_floats(long long rows) { return (size_t)5 * std::min<long long>(rows, 32768) * 512; }'
    assert plan.count(sizing) == 1 and plan.count('32768') == 1 and '32768' not in taco
    assert plan.count('conv_scratch_floats(') == 1
    # ... that sizes the conv scratch of all three plans: the encoder's over its R rows, and the postnet's over its RD rows,
    # which the decode plan and the postnet probe both take from postnet_layout
    assert taco.count('conv_scratch_floats(') == 2
    assert 't.convtmp_n = conv_scratch_floats(R);\n    t.convtmp = A.take<float>(t.convtmp_n);' in taco
    assert 'p.convtmp_n = conv_scratch_floats(RD);\n    p.convtmp = A.take<float>(p.convtmp_n);' in taco
    assert taco.count('postnet_layout(') == 3               # its definition, decoder_layout, the probe's plan
    assert 'w.post = postnet_layout(A, (long long)B * max_len);' in taco and 'pb = postnet_layout(A, RD);' in taco
    assert taco.count('encoder_tmp_layout(') == 2 and 'convtmp_n = 5' not in taco


def test_source_masks_and_activations_of_the_convs():
    taco = _src('tacotron2.hip')
    # encoder: relu, padded rows stored as 0 (mask_out 1); postnet: tanh + 0 on convs 1-4, no activation + BN(0) on conv 5
    assert 'conv_gemm(e, tc.enc_conv[i], xin, 512, xout, (int)R, Tin, out->mask, ACT_RELU, 1, t.convtmp, t.convtmp_n, i)' in taco
    assert 'last ? ACT_NONE : ACT_TANH' in taco and 'last ? 0 : 1, pb.convtmp, pb.convtmp_n, 3 + i' in taco
    assert 'const bool on = t <= lengths[b];' in taco                  # dec_mask_kernel
    assert cc.LAYERS['encoder'] == [(512, 'relu', 'zero')] * 3
    assert cc.LAYERS['postnet'] == [(512, 'tanh', 'zero')] * 4 + [(80, None, 'bn0')]


def test_pick_conv_path_at_its_edges():
    p = cc.pick_conv_path
    assert p(4032, 512) == 'split' and p(4033, 512) == 'single'         # 63 x 8 = 504 tiles, 64 x 8 = 512
    assert p(16320, 80) == 'split' and p(16321, 80) == 'single'         # 255 x 2 = 510 tiles, 256 x 2 = 512
    assert p(1, 512) == 'split' and p(1, 80) == 'split'
    for M in (1, 64, 4032, 16320):                                      # the scratch condition never binds
        for cout in (80, 512):
            if -(-M // 64) * -(-cout // 64) < 512:
                assert 5 * M * cout <= 5 * min(M, 32768) * 512


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_cases_reach_every_conv_on_both_paths_at_the_thresholds():
    got = set()
    for stage, cases in (('encoder', cc.ENCODER_CASES), ('postnet', cc.POSTNET_CASES)):
        for c in cases:
            for i, path in enumerate(cc.path_names(stage, c.rows)):
                got.add((stage, i, path))
    want = {(s, i, p) for s in ('encoder', 'postnet') for i in range(len(cc.LAYERS[s])) for p in ('split', 'single')}
    assert got == want, sorted(want - got)
    enc_rows = {c.rows for c in cc.ENCODER_CASES}
    post_rows = {c.rows for c in cc.POSTNET_CASES}
    assert {4032, 4033} <= enc_rows
    assert {4032, 4033, 16320, 16321} <= post_rows
    assert {8 * 800, 32 * 400} <= post_rows                             # config 3, config-4 job


def test_cases_put_sequence_ends_and_pads_where_kernels_go_wrong():
    encs = {c.name: c for c in cc.ENCODER_CASES}
    assert encs['b1_t4096'].Tin == 4096 and encs['b1024_t4'].B == 1024 and encs['cfg4_e768_b32_t256'].enc == 768
    assert min(cc.enc_lens(encs['cfg4_e768_b32_t256'])) == 50 and max(cc.enc_lens(encs['cfg4_e768_b32_t256'])) == 200
    assert {c.Tin for c in cc.ENCODER_CASES if c.B == 3} == {2, 3, 4, 5}
    for c in cc.ENCODER_CASES:
        lens = cc.enc_lens(c)
        assert len(lens) == c.B and min(lens) >= 1 and max(lens) <= c.Tin
        if c.B > 1:
            assert len(set(lens)) > 1, c.name                           # ragged
    assert any(c.mid_pad for c in cc.ENCODER_CASES if cc.path_names('encoder', c.rows)[0] == 'split')
    assert any(c.mid_pad for c in cc.ENCODER_CASES if cc.path_names('encoder', c.rows)[0] == 'single')
    for c in cc.POSTNET_CASES:
        L = cc.post_lengths(c)
        assert len(L) == c.B
        if c.B >= 5:
            assert 0 in L and c.T - 2 in L and L.max() >= c.T - 1 and ((L > 0) & (L < c.T - 2)).any()


# ---- controls: each defect against the bounds --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def enc_case():
    """b3_t5: three rows of 5, 2, 4 tokens with a pad at position 2 of row 0 -- every tap crosses a sequence end."""
    case = cc.ENC_BY_NAME['b3_t5']
    tok, _ = cc.enc_inputs(case)
    return case, tok, cc.encoder_reference(case.name)


@pytest.fixture(scope='module')
def post_case():
    """b800_t7 cut to its first 40 rows (lengths 0, 3, 5, 6, 10, 7, ...)."""
    case = cc.POST_BY_NAME['b800_t7']
    frames, lengths = cc.post_inputs(case)
    frames, lengths = frames[:40], lengths[:40]
    return frames, lengths, cc.postnet_of(frames, lengths, 512)


def _conv_bn(x, mask, w, conv, norm, act, mask_input=True, kernel=None):
    """masked_conv_bn with the input masking optional (the engine's conv reads its input as stored)."""
    from oracle import tacotron2_ref as R
    mf = mask[:, :, None].astype(np.float64)
    k = w[f'{conv}/kernel'] if kernel is None else kernel
    out = R.conv1d_same(x * mf if mask_input else x, k, w[f'{conv}/bias']) * mf
    out = R.batch_norm(out, w, norm, 1e-5)
    return np.maximum(out, 0) if act == 'relu' else np.tanh(out) if act == 'tanh' else out


def test_control_tap_leaking_across_a_sequence_end(enc_case, post_case):
    case, tok, ref = enc_case
    w = cc.weights64(512)
    p = 'tacotron2/encoder'
    mask = ref['mask']
    x = w[f'{p}/embeddings'][tok]
    B, T = tok.shape
    flat = _conv_bn(x.reshape(1, B * T, -1), mask.reshape(1, B * T), w, f'{p}/conv_1', f'{p}/norm_1', 'relu')
    e = cc.stage_error(flat.reshape(B, T, -1), ref['conv1'], mask)
    assert e > MARGIN * cc.bound_of('encoder', 'conv1'), e
    frames, lengths, pref = post_case
    B, T = frames.shape[:2]
    m = pref['mask']
    q = 'tacotron2/postnet'
    flat = _conv_bn(frames.reshape(1, B * T, -1).astype(np.float64), m.reshape(1, B * T), w, f'{q}/conv_1', f'{q}/norm_1',
                    'tanh')
    e = cc.stage_error(flat.reshape(B, T, -1), pref['conv1'], m)
    assert e > MARGIN * cc.bound_of('postnet', 'conv1'), e


def test_control_padded_rows_left_at_act_bn0(enc_case, post_case):
    case, tok, ref = enc_case
    w = cc.weights64(512)
    mask = ref['mask']
    # the GPU test requires padded rows of the intermediate convs to be exactly 0; act(BN(0)) is far from it
    assert float(np.abs(ref['conv1'][~mask]).max()) > 0.01
    # and the next conv, which reads its input as stored (no input mask), moves the valid rows next to a pad
    p = 'tacotron2/encoder'
    wrong = _conv_bn(ref['conv1'], mask, w, f'{p}/conv_2', f'{p}/norm_2', 'relu', mask_input=False)
    e = cc.stage_error(wrong, ref['conv2'], mask)
    assert e > MARGIN * cc.bound_of('encoder', 'conv2'), e
    frames, lengths, pref = post_case
    m = pref['mask']
    q = 'tacotron2/postnet'
    assert float(np.abs(pref['conv1'][~m]).max()) > 0.01
    wrong = _conv_bn(pref['conv1'], m, w, f'{q}/conv_2', f'{q}/norm_2', 'tanh', mask_input=False)
    e = cc.stage_error(wrong, pref['conv2'], m)
    assert e > MARGIN * cc.bound_of('postnet', 'conv2'), e


def test_control_conv5_masked_rows_as_zero(post_case):
    frames, lengths, pref = post_case
    m = pref['mask']
    wrong = np.where(m[:, :, None], pref['conv5'], 0.0)
    e = cc.stage_error(wrong, pref['conv5'])
    assert e > MARGIN * cc.bound_of('postnet', 'conv5'), e
    e = cc.stage_error(frames + wrong, pref['mel'])
    assert e > MARGIN * cc.bound_of('postnet', 'mel'), e


def test_control_mask_rule_t_below_len(post_case):
    frames, lengths, pref = post_case
    T = frames.shape[1]
    m = np.arange(T)[None, :] < lengths[:, None]
    wrong = cc.postnet_convs64(frames, m, cc.weights64(512), cc.config(512))
    e = cc.stage_error(frames + wrong[-1], pref['mel'])
    assert e > MARGIN * cc.bound_of('postnet', 'mel'), e
    e = cc.stage_error(wrong[0], pref['conv1'], pref['mask'])
    assert e > MARGIN * cc.bound_of('postnet', 'conv1'), e


def test_control_reversed_tap_order(enc_case, post_case):
    case, tok, ref = enc_case
    w = cc.weights64(512)
    p = 'tacotron2/encoder'
    x = w[f'{p}/embeddings'][tok]
    wrong = _conv_bn(x, ref['mask'], w, f'{p}/conv_1', f'{p}/norm_1', 'relu', kernel=w[f'{p}/conv_1/kernel'][::-1])
    e = cc.stage_error(wrong, ref['conv1'], ref['mask'])
    assert e > MARGIN * cc.bound_of('encoder', 'conv1'), e
    frames, lengths, pref = post_case
    wrong = cc.postnet_convs64(frames, pref['mask'], w, cc.config(512), kernel_map=lambda k: k[::-1])
    for i, what in enumerate(cc.POST_STAGES[:5]):
        e = cc.stage_error(wrong[i], pref[what], pref['mask'] if cc.valid_only('postnet', what) else None)
        assert e > MARGIN * cc.bound_of('postnet', what), (what, e)


def test_references_are_the_oracle(enc_case, post_case):
    """The float64 restatements agree with the oracle's own entry points (tacotron2_ref.encoder / postnet)."""
    from oracle import tacotron2_ref as R
    case, tok, ref = enc_case
    w, cfg = cc.weights64(512), cc.config(512)
    mem, mask = R.encoder(tok, w, cfg)
    assert np.array_equal(mem, ref['memory']) and np.array_equal(mask, ref['mask'])
    assert np.array_equal(ref['conv1'][mask] > 0, ref['conv1'][mask] != 0)             # relu outputs
    frames, lengths, pref = post_case
    post = R.postnet(frames.astype(np.float64), pref['mask'], w, cfg)
    assert np.array_equal(post, pref['conv5'])
    assert np.array_equal(pref['mel'], frames + post)
