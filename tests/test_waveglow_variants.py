"""CPU half of the WaveGlow-variant matrix (tests/waveglow_cases.py): the case table reaches every WN GEMM instantiation and
every Winograd kernel kind that `waveglow_run` can launch, `pick_variant` restates the dispatch rules at their edges, and
every bound of test_waveglow_variants_gpu.py could fail -- oracle-only controls showing that a tap leaking across an
utterance end, a conditioning frame off by one, an ignored fp16 flag and a small error in the `end` conv would be caught.
The same for calls with row lengths (RAGGED_CASES / PACKED_CASES, tests/test_waveglow_rows_gpu.py): the tables reach every
tile family and every MASK_LENS / MASK_FLAGS instantiation, and each mistake a mask can make -- x not zeroed somewhere, a mask
one frame too long, a gap one frame too short, an uncleared gap mel, an unmasked z or state tail -- would be caught."""
import os
import re

import numpy as np
import pytest

import waveglow_cases as wc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'text_to_speech_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _reached():
    """{kernel name} over every case x (precision, form) of the table."""
    got = set()
    for c in wc.CASES:
        for p, f in wc.runs(c):
            got |= wc.pick_variant(c.B, c.T, p, f).kernels
    return got


# ---- coverage ----------------------------------------------------------------------------------------------------------
def test_cases_reach_every_wn_gemm_wrapper_and_instantiation():
    """Every `gemm_wn_*` wrapper of gemm_f32.h (both values of a bool argument that picks the instantiation: split fp16's
    `small`, fp16's `t128`) is reached by some case, and every `gemm_wn_*` name in waveglow.hip (the `kWnKernels` table, where
    a bool is bound as `bound<wrapper, value>`) / wn_wino.hip (call sites) is one of them: a new wrapper, table entry or call
    site fails here until the case table covers it."""
    wrappers = re.findall(r'inline hipError_t (gemm_wn_\w+)\(const GemmArgs& \w+, (?:bool (\w+), )?(?:int \w+, )?hipStream_t',
                          _src('gemm_f32.h'))
    assert len(wrappers) >= 20, wrappers
    expected = set()
    for name, flag in wrappers:
        expected |= {f'{name}({flag}=True)', f'{name}({flag}=False)'} if flag else {name}
    got = {k.split('/')[0] for k in _reached()}
    assert expected <= got, sorted(expected - got)
    names = {n for n, _ in wrappers}
    for src in ('waveglow.hip', 'wn_wino.hip'):
        named = set(re.findall(r'\b(gemm_wn_\w+)\b', _src(src)))
        assert named and named <= names, sorted(named - names)
        assert named <= {k.split('(')[0] for k in got}, sorted(named - {k.split('(')[0] for k in got})
    # the table binds both values of every bool, and names a wrapper with a bool in no other way
    flags = dict(wrappers)
    table = _src('waveglow.hip')
    bound = {(n, v) for n, v in re.findall(r'\bbound<(gemm_wn_\w+), (true|false)>', table)}
    assert bound == {(n, v) for n in names if flags[n] for v in ('true', 'false')}, sorted(bound)
    assert not [n for n in re.findall(r'(?<!bound<)\b(gemm_wn_\w+)\b', table) if flags[n]]
    # every wrapper without a bool that the direct form launches is in the table (gemm_wn_wino*: wn_wino.hip's call sites)
    assert {n for n in names if not flags[n] and not n.startswith('gemm_wn_wino')} <= set(re.findall(r'\b(gemm_wn_\w+)\b', table))


def test_cases_reach_every_winograd_kernel_kind_and_end_fold_instantiation():
    got = _reached()
    wino = _src('wn_wino.hip')
    # the three in-layer kernels of the Winograd forms and the combine pass of form 2, launched in waveglow_wino_layer
    assert 'launch_wino_fused2(b, st)' in wino and 'launch_wino_fused<2, 2, 3, 2>(a, st)' in wino
    assert 'hipLaunchKernelGGL(wino4_combine_kernel' in wino
    for kernel in ('fused2', 'fused_prepass'):
        assert {f'{kernel}/{g}' for g in wc.WINO_KINDS} <= got, kernel
    assert {'gemm_wn_wino/phases', 'gemm_wn_wino_128/phases', 'gemm_wn_wino_128/mixed', 'gemm_wn_wino_128/frames',
            'combine'} <= got
    # launch_end_fold: one dispatch over <HALF, SPLIT, MASK>, launched through end_fold<..> and nowhere else
    src = _src('waveglow.hip')
    assert len(re.findall(r'hipLaunchKernelGGL\(\(wn_end_fold_kernel<', src)) == 1
    assert 'hipLaunchKernelGGL((wn_end_fold_kernel<HALF, SPLIT, MASK>)' in src
    combos = set(re.findall(r'\bend_fold<(true|false), (true|false), (MASK_\w+)>\(', src))
    assert combos == {(h, s, m) for h, s in (('false', 'false'), ('true', 'false'), ('true', 'true'))
                      for m in ('MASK_NONE', 'MASK_LENS', 'MASK_FLAGS')}, sorted(combos)
    folds = {f'wn_end_fold_kernel<{h}, {s}>' for h, s, _ in combos}
    assert len(folds) == 3 and folds <= got, sorted(folds - got)


def test_cases_reach_every_tile_family_in_every_form_and_the_edges():
    seen = {(p, f, v.tiles, v.wino) for c in wc.CASES for p, f in wc.runs(c) for v in [wc.pick_variant(c.B, c.T, p, f)]}
    for fam in ('64-row', '128x64', '128-row', '256-row'):
        assert ('f32', 'winograd', fam, False) in seen or fam != '128x64' and ('f32', 'direct', fam, False) in seen, fam
        assert ('f16', 'winograd', fam, False) in seen, fam
    for fam in ('64-row', '128-row', '256-row'):
        for form in ('winograd', 'winograd-prepass'):
            assert ('f32', form, fam, True) in seen, (form, fam)
    assert ('f32', 'winograd-3pass', '256-row', True) in seen and ('f32', 'winograd-3pass', '128-row', True) in seen
    assert ('f32', 'winograd-3pass', '64-row', False) in seen            # form 2 keeps 64-row tiles: the direct form
    assert {('f16x3', 'winograd', fam, False) for fam in ('64-row', '256-row')} <= seen
    bts = {c.BT for c in wc.CASES}
    assert {143, 144, 192, 193, 255, 256, 383, 384 + 1, 512, 513} <= bts
    assert {c.T for c in wc.CASES if c.B > 1} >= {1, 2, 3}
    assert any(c.T % 2 and c.T % 16 for c in wc.CASES if c.BT >= wc.WINO_MIN_FRAMES)
    pads = {(wc.pick_variant(c.B, c.T, p, f).PR - c.BT, wc.pick_variant(c.B, c.T, p, f).tiles)
            for c in wc.CASES for p, f in wc.runs(c)}
    assert {(1, '256-row'), (1, '128-row'), (63, '64-row'), (127, '128-row')} <= pads
    assert set(wc.LATER_FLOW_CASES) <= set(wc.CASE_BY_NAME) and set(wc.STATE_CASES) <= set(wc.CASE_BY_NAME)


# ---- dispatch edges ----------------------------------------------------------------------------------------------------
def _v(BT, precision='f32', form='winograd', T=None):
    T = BT if T is None else T
    return wc.pick_variant(BT // T, T, precision, form)


def test_pick_variant_restates_the_dispatch_rules_at_their_edges():
    # the Winograd start (fp32 only, forms >= 1)
    assert not _v(143).wino and _v(144).wino and not _v(144, form='direct').wino
    assert not _v(144, 'f16').wino and not _v(1024, 'f16x3').wino
    # fp32 64-row tiles: pr64 < pr_big and B*T <= 512
    assert _v(64).tiles == '64-row' and _v(65).tiles == '128x64' and _v(128).tiles == '128x64'
    assert _v(129).tiles == '64-row' and _v(192).tiles == '64-row' and _v(193).tiles == '256-row'
    assert _v(448).tiles == '64-row' and _v(449).tiles == '256-row'
    assert _v(512).tiles == '256-row' and _v(513).tiles == '128-row' and _v(513).PR == 640     # 576 < 640 but above the limit
    # 128-row tiles: pr128 * 1.05 < pr256
    assert _v(383).tiles == '128-row' and _v(256).tiles == '256-row' and _v(1024, T=128).tiles == '256-row'
    assert _v(2432, T=128).tiles == '128-row' and _v(2560 + 128, T=128).tiles == '256-row'    # 2688 * 1.05 > 2816
    # 128 x 64 tiles: (M / 128) * 8 < 768, i.e. fewer than 384 rows per phase
    assert _v(100).tiles == '128x64' and _v(100).PR == 128
    assert _v(383, form='direct').tiles == '128-row' and _v(383).PR * 32 // 128 * 8 == 768
    # fp16: the 64-row tiles pay from -25 % rows (pr64 * 4 <= pr_big * 3)
    assert _v(64, 'f16').tiles == '64-row' and _v(65, 'f16').tiles == '128x64'
    assert _v(192, 'f16').tiles == '64-row' and _v(193, 'f16').tiles == '256-row'              # 768 <= 768, 1024 > 768
    assert _v(257, 'f16').tiles == '128-row' and _v(257, 'f16').PR == 384                      # 1280 > 1152
    assert 'gemm_wn_in_h(t128=True)' in _v(257, 'f16').kernels
    assert 'gemm_wn_in_h(t128=False)' in _v(256, 'f16').kernels
    # split fp16: 64 x 128 while pr64 * 1.25 < pr256, 256 x 256 otherwise; no row-64 limit, no 128-row family
    assert _v(192, 'f16x3').tiles == '64-row' and _v(193, 'f16x3').tiles == '256-row'
    assert _v(384, 'f16x3').tiles == '64-row' and _v(385, 'f16x3').tiles == '256-row'
    assert _v(513, 'f16x3').tiles == '64-row' and _v(100, 'f16x3').tiles == '64-row'
    assert 'gemm_wn_in0_x3(small=False)' in _v(256, 'f16x3').kernels
    # form 2: PR % 256 picks the phase-group GEMM; the row-64 rescue (pr128 * 1120 * 1.35 < pr64 * 1856) or the direct form
    assert 'gemm_wn_wino/phases' in _v(256, form='winograd-3pass').kernels
    assert 'gemm_wn_wino_128/phases' in _v(513, form='winograd-3pass').kernels
    r = _v(300, form='winograd-3pass', T=75)
    assert r.wino and r.tiles == '128-row' and r.PR == 384 and 'gemm_wn_wino_128/phases' in r.kernels
    assert _v(300, form='winograd', T=75).tiles == '64-row'                                   # no rescue outside form 2
    d = _v(144, form='winograd-3pass', T=9)
    assert not d.wino and d.tiles == '64-row' and 'gemm_wn_in_r64' in d.kernels               # 256 / 192 > 1.2275
    # group rows: frame groups 4 ceil(T / 16) and mixed groups ceil(T / 2) per utterance, padded to 64 (form 2: 128)
    assert wc.group_rows(16, 9, 1) == (64, 128) and wc.group_rows(150, 1, 1) == (640, 192)
    assert wc.group_rows(4, 75, 2) == (128, 256) and wc.group_rows(3, 171, 1) == (192, 320)


# ---- oracle-only controls ----------------------------------------------------------------------------------------------
CTRL = wc.CASE_BY_NAME['t3_b4']


def _ctrl_inputs(case=CTRL):
    mel, z = wc.inputs(case)
    return mel, z, wc.spect_of(mel, wc.weights64())


@pytest.fixture(scope='module')
def ctrl_ref():
    return wc.flow11_acts(CTRL)


def test_control_a_tap_leaking_across_an_utterance_end_breaks_the_edge_bound(ctrl_ref, monkeypatch):
    """One position read across the start of every utterance (the previous utterance's last position instead of the zero
    padding), in one layer at a time: the edge-window error of that layer is at least 10x the bound of every precision
    but fp16, and still above fp16's (max abs error too)."""
    from oracle import waveglow_ref
    mel, z, spect = _ctrl_inputs()
    conv = waveglow_ref.conv1d_dilated_same
    L = CTRL.T * wc.NPH
    for leak in range(wc.N_LAYERS):
        d = 1 << leak
        if d > L:                           # no tap of a d > L layer reaches the position before an utterance
            continue

        def leaky(x, kernel, bias, dilation, _d=d):
            out = conv(x, kernel, bias, dilation)
            if dilation == _d:              # output position d - 1 reads x[-1] through its first tap
                prev = np.roll(x[:, -1], 1, axis=0)
                out[:, _d - 1] += prev @ kernel[0]
            return out

        monkeypatch.setattr(waveglow_ref, 'conv1d_dilated_same', leaky)
        acts = wc.flow_acts(z[:, :, :2], spect, 11, stop_after=leak)
        monkeypatch.setattr(waveglow_ref, 'conv1d_dilated_same', conv)
        e = wc.act_errors(acts[leak], ctrl_ref[leak], CTRL.T, d)
        print(f'leak at layer {leak}: edge {e["edge"]:.2e} rel {e["rel"]:.2e} abs {e["abs"]:.2e}')
        for p in ('f32', 'f16x3'):
            assert e['edge'] >= 10 * wc.ACTS_EDGE_REL[p] and e['abs'] >= 10 * wc.ACTS_ABS[p], (leak, p)
        assert e['edge'] > wc.ACTS_EDGE_REL['f16'] and e['abs'] > wc.ACTS_ABS['f16'], leak


def test_control_a_conditioning_frame_off_by_one_breaks_every_bound(ctrl_ref):
    """The mel frames shifted by one inside every utterance (frame t conditioned on t - 1, zeros before the start)."""
    mel, z, _ = _ctrl_inputs()
    shifted = np.zeros_like(mel)
    shifted[:, 1:] = mel[:, :-1]
    acts = wc.flow_acts(z[:, :, :2], wc.spect_of(shifted, wc.weights64()), 11)
    for i in range(wc.N_LAYERS):
        e = wc.act_errors(acts[i], ctrl_ref[i], CTRL.T, 1 << i)
        print(f'mel off by one, layer {i}: rel {e["rel"]:.2e} edge {e["edge"]:.2e} abs {e["abs"]:.2e}')
        for k, bound in (('rel', wc.ACTS_REL), ('edge', wc.ACTS_EDGE_REL), ('abs', wc.ACTS_ABS)):
            assert e[k] >= 10 * max(bound['f32'], bound['f16x3']) and e[k] > bound['f16'], (i, k)


def test_control_fp16_operands_are_far_from_fp32(ctrl_ref, monkeypatch):
    """Every GEMM operand rounded to fp16 (residual stream, first-layer input, weights, mel): the activations move at least
    3x F16_FLOOR from the fp32 oracle, and the fp32 bound sits 10x below that floor -- so an fp16 call that ignored its
    flag (fp32 arithmetic, within the fp32 bound) fails the floor of test_waveglow_variants_gpu.py."""
    from oracle import waveglow_ref
    assert 10 * max(wc.ACTS_REL['f32'], wc.ACTS_REL['f16x3']) <= wc.F16_FLOOR < wc.ACTS_REL['f16']
    r16 = lambda a: np.asarray(a).astype(np.float16).astype(np.float64)
    mel, z, _ = _ctrl_inputs()
    w16 = {k: (r16(v) if '/kernel' in k else v) for k, v in wc.weights64().items()}
    conv = waveglow_ref.conv1d_dilated_same
    monkeypatch.setattr(waveglow_ref, 'conv1d_dilated_same', lambda x, k, b, d: conv(r16(x), k, b, d))
    acts = wc.flow_acts(r16(z[:, :, :2]), r16(wc.spect_of(r16(mel), wc.weights64())), 11, w=w16)
    for i in range(wc.N_LAYERS):
        e = wc.act_errors(acts[i], ctrl_ref[i], CTRL.T, 1 << i)
        print(f'fp16 operands, layer {i}: rel {e["rel"]:.2e} edge {e["edge"]:.2e} abs {e["abs"]:.2e}')
        assert e['rel'] >= 3 * wc.F16_FLOOR, i


def test_control_an_end_conv_error_of_1e4_moves_the_post_flow_state_beyond_its_bound():
    """Every `end` conv output scaled by 1 + 1e-4 (weights with end_scale 0.2): the flow state after flows 11, 8, 4 and 0
    moves beyond the fp32 / f16x3 bounds."""
    from oracle import waveglow_ref
    case = wc.CASE_BY_NAME[wc.STATE_CASES[0]]
    ref = wc.states(case)
    w = dict(wc.weights(wc.STATE_END_SCALE))
    for k in range(12):
        for part in ('kernel', 'bias'):
            name = f'waveglow/block-{k}/end_conv/{part}'
            w[name] = np.asarray(w[name], np.float64) * (1 + 1e-4)
    mel, z = wc.inputs(case)
    _, inter = waveglow_ref.infer(mel.astype(np.float64), w, wc.config(), z=z.astype(np.float64), sigma=1.0,
                                  dtype=np.float64, return_intermediates=True)
    for k in (11, 8, 4, 0):
        e = wc.state_errors(inter[f'audio_after_flow_{k}'], ref[k])
        print(f'end conv x (1 + 1e-4): state after flow {k}: rel {e["rel"]:.2e} max_rel {e["max_rel"]:.2e}')
        for p in ('f32', 'f16x3'):
            assert e['rel'] > wc.STATE_REL[p] and e['max_rel'] > wc.STATE_MAX_REL[p], (k, p)


# ---- calls with row lengths: coverage ------------------------------------------------------------------------------------
def _rows_seen(cases):
    return {(p, f, v.tiles, v.wino) for c in cases for p, f in wc.runs(c) for v in [wc.rows_variant(c, p, f)]}


@pytest.mark.parametrize('table', ['ragged', 'packed'])
def test_rows_cases_reach_every_tile_family_and_the_winograd_form_on_each(table):
    cases = wc.RAGGED_CASES if table == 'ragged' else wc.PACKED_CASES
    seen = _rows_seen(cases)
    for fam in ('64-row', '128x64', '128-row', '256-row'):
        assert any(s[0] == 'f32' and s[2] == fam and not s[3] for s in seen), fam
        assert ('f16', 'winograd', fam, False) in seen, fam
    assert {('f16x3', 'winograd', fam, False) for fam in ('64-row', '256-row')} <= seen
    for fam in ('64-row', '128-row', '256-row'):
        assert ('f32', 'winograd', fam, True) in seen, fam
    if table == 'packed':
        assert all(set(c.forms) == {'winograd', 'direct'} and c.packed and c.frames == sum(c.lengths) + wc.GAP * (
            sum(n > 0 for n in c.lengths) - 1) for c in cases)
        assert any(c.T > 10 * max(c.lengths) for c in cases)        # the gather's source index is not the packed index
    else:
        assert ('f32', 'winograd-3pass', '256-row', True) in seen and ('f32', 'winograd-3pass', '128-row', True) in seen
        assert {'gemm_wn_wino/phases', 'gemm_wn_wino_128/phases'} <= {
            k for c in cases for f in c.forms for k in wc.rows_variant(c, 'f32', f).kernels}
    # every table: a row of length 0, 1, T and T - 1 (T > 1: not the same row as the one of length 0), an odd length
    for want in ('zero', 'one', 'T', 'T-1', 'odd'):
        assert any({'zero': n == 0, 'one': n == 1, 'T': n == c.T, 'T-1': n == c.T - 1 and c.T > 2, 'odd': n % 2 == 1}[want]
                   for c in cases for n in c.lengths), (table, want)
    pads = {(wc.rows_variant(c, p, f).PR - c.frames, wc.rows_variant(c, p, f).tiles) for c in cases for p, f in wc.runs(c)}
    assert (127, '128-row') in pads and (63, '64-row') in pads or table == 'packed' and (1, '128-row') in pads


def test_rows_cases_reach_every_masked_instantiation_named_in_the_source():
    """init_audio_kernel<MASK_*>, wn_end_last_kernel<MASK_*> and end_fold<HALF, SPLIT, MASK_*> for MASK_LENS and MASK_FLAGS:
    every one that waveglow.hip names is launched by some case of the tables (fp32 end_fold: the 256-channel cases), and the
    tables name none that the source does not have."""
    src = _src('waveglow.hip')
    named = {f'{k}<{m}>' for k, m in re.findall(r'\b(init_audio_kernel|wn_end_last_kernel)<(MASK_LENS|MASK_FLAGS)>', src)}
    named |= {f'end_fold<{h}, {s}, {m}>' for h, s, m in
              re.findall(r'\bend_fold<(true|false), (true|false), (MASK_LENS|MASK_FLAGS)>\(', src)}
    assert len(named) == 2 + 2 + 6, sorted(named)
    got = set()
    for c in wc.ROWS_CASES:
        for p in wc.PRECISIONS:
            got |= wc.mask_kernels(c, p)
    for name in wc.ROWS_256_CASES:
        got |= wc.mask_kernels(wc.ROWS_CASE_BY_NAME[name], 'f32', channels=256)
    assert got == named, (sorted(named - got), sorted(got - named))
    # one launch site per kind, picked by the run's mask alone: a packed run takes MASK_FLAGS, a ragged one MASK_LENS
    assert 'const int mask = d_flags ? MASK_FLAGS : d_lens ? MASK_LENS : MASK_NONE;' in src
    assert 'c.endp = (precision == 0 && C == 512) ? wg.endp.f() : nullptr;' in src
    for names in (wc.ROWS_LATER_FLOW_CASES, wc.ROWS_STATE_CASES, wc.ROWS_COND_CASES, wc.ROWS_256_CASES):
        assert set(names) <= set(wc.ROWS_CASE_BY_NAME)
    assert all(wc.rows_variant(wc.ROWS_CASE_BY_NAME[n], 'f32').wino for n in wc.ROWS_COND_CASES)
    from waveglow_packed_ref import header_gap_frames
    assert wc.GAP == header_gap_frames()


# ---- calls with row lengths: oracle-only controls --------------------------------------------------------------------------
CTRL_ROWS = wc.RowsCase('ctrl_r3x13', 3, 13, (13, 5, 9))
CTRL_PACKED = CTRL_ROWS._replace(name='ctrl_p35', packed=True)


_SOLO = {}


def _solo_acts(case, mel, z):
    """Per row: the oracle's flow-11 activations on the row's own frames (one computation per set of rows)."""
    key = (case.B, case.T, case.lengths, case.packed)          # (what seeds rows_inputs)
    if key not in _SOLO:
        _SOLO[key] = _solo_acts_of(case, mel, z)
    return _SOLO[key]


def _solo_acts_of(case, mel, z):
    return [wc.flow_acts(z[b:b + 1, :n * wc.NPH, :2], wc.spect_of(mel[b:b + 1, :n], wc.weights64()), 11)
            for b, n in enumerate(case.lengths)]


def _run_layout(case, mel, z, gap=wc.GAP, fill=None):
    """(mel [R, F, 80], z [R, F*32, 8], real [R, F]) of the one run: the padded batch, or the packed row with `gap` frames
    between two rows; gap frames hold `fill`'s values (a generator: the engine gathers nothing there, the control puts numbers)."""
    if not case.packed:
        return mel, z, np.arange(case.T)[None, :] < np.asarray(case.lengths)[:, None]
    from waveglow_packed_ref import packing_plan
    plan = packing_plan(case.lengths, case.T, gap)
    F = plan['F']
    pm, pz = fill.uniform(-11.5, 1.2, (1, F, 80)), fill.standard_normal((1, F * wc.NPH, 8))
    for b, n in enumerate(case.lengths):
        at = plan['starts'][b]
        pm[0, at:at + n], pz[0, at * wc.NPH:(at + n) * wc.NPH] = mel[b, :n], z[b, :n * wc.NPH]
    return pm, pz, (np.asarray(plan['flags']) != 0)[None, :]


def _masked_acts(mel, z, real, unmasked=(), clear_mel=True, mask_z=True):
    """Flow 11's activations of the masked oracle on one run (float64)."""
    from waveglow_packed_ref import wn_block_masked
    keep = real.astype(np.float64)
    mel = np.asarray(mel, np.float64) * (keep[:, :, None] if clear_mel else 1.0)
    pos = np.repeat(keep, wc.NPH, axis=1)[:, :, None]
    a0 = np.asarray(z, np.float64)[:, :, :2] * (pos if mask_z else 1.0)
    acts = []
    wn_block_masked(a0, wc.spect_of(mel, wc.weights64()), wc.weights64(), 'waveglow/block-11', pos, collect=acts,
                    unmasked=unmasked)
    return acts


def _worst_per_row(case, acts, solo, starts=None):
    """Worst of every metric over rows and layers, each row against the oracle on its own frames."""
    worst = {'rel': 0.0, 'edge': 0.0, 'abs': 0.0}
    case = case if starts is None else _Starts(case, starts)
    for b, n in enumerate(case.lengths):
        if n:
            for layer in range(wc.N_LAYERS):
                out = acts[layer][0] if case.packed else acts[layer]
                e = wc.act_errors(wc.row_of(case, out, b), solo[b][layer], n, 1 << layer)
                worst = {k: max(worst[k], e[k]) for k in worst}
    return worst


class _Starts:
    """A packed case whose rows start elsewhere (the 3-gap-frame control)."""

    def __init__(self, case, starts):
        self.packed, self.lengths, self.starts = case.packed, case.lengths, starts


def _exceeds(e, factor, precisions):
    return all(any(e[k] >= factor * bound[p] for k, bound in (('rel', wc.ACTS_REL), ('edge', wc.ACTS_EDGE_REL),
                                                              ('abs', wc.ACTS_ABS))) for p in precisions)


@pytest.mark.parametrize('case', [CTRL_ROWS, CTRL_PACKED], ids=lambda c: c.name)
def test_control_masked_oracle_on_the_run_is_the_solo_oracle_per_row(case):
    """Lengths (13, 5, 9): x zeroed after the start conv and after every residual sum -- and nothing else, neither the mel
    tail cleared nor the z tail masked -- gives every row what it computes alone, to float64 rounding (measured: no bit
    differs).  So the activations cannot see those two mistakes: the state controls below do.  A packed row is different
    in one respect: the transposed-conv upsampling looks three frames BACK, so what the mel holds on a gap frame reaches the
    first frames of the row behind it -- there an uncleared mel is a planted mistake of the next test, not of this one."""
    mel, z = wc.rows_inputs(case, nan=False)
    solo = _solo_acts(case, mel, z)
    rm, rz, real = _run_layout(case, mel, z, fill=np.random.default_rng(3))
    for kw in ({}, dict(mask_z=False)) + (() if case.packed else (dict(clear_mel=False),)):
        e = _worst_per_row(case, _masked_acts(rm, rz, real, **kw), solo)
        print(f'{case.name} masked oracle {kw}: rel {e["rel"]:.1e} edge {e["edge"]:.1e} abs {e["abs"]:.1e}')
        assert e['rel'] <= 1e-13 and e['edge'] <= 1e-13 and e['abs'] <= 1e-12


PLANTED = [('start', dict(unmasked=('start',))), ('res0', dict(unmasked=(0,))), ('res3', dict(unmasked=(3,))),
           ('res6', dict(unmasked=(6,))), ('long', dict(longer=1)), ('gap_mel', dict(clear_mel=False))]


# (behind a row's length nothing looks at the mel -- the upsampling is causal -- so 'gap_mel' is a mistake of the packed row only)
PLANTED_RUNS = [(c, n, m) for c in (CTRL_ROWS, CTRL_PACKED) for n, m in PLANTED if n != 'gap_mel' or c.packed]


@pytest.mark.parametrize('case,name,mistake', PLANTED_RUNS, ids=[f'{c.name}-{n}' for c, n, _ in PLANTED_RUNS])
def test_control_a_planted_mask_mistake_breaks_the_per_row_bounds(case, name, mistake):
    """One mistake at a time in the masked oracle -- x not zeroed after the start conv, or after residual sum 0 / 3 / 6, or a
    mask one frame too long -- moves some row beyond the bounds of waveglow_cases in at least one metric, by a factor 100 for
    f32 and f16x3 and by 3 for f16.  Measured worst over rows and layers, lengths (13, 5, 9) in a [3, 13] batch with this
    module's inputs (rel / edge / abs): start 1.8e-3 / 1.7e-2 / 1.1e-1; res0 1.6e-2 / 1.0e-1 / 0.83; res3 4.1e-2 / 9.3e-2 /
    1.1; res6 1.0e-1 / 1.0e-1 / 1.1; one frame too long 2.0e-1 / 3.2e-1 / 1.9.  The same rows packed with 4 gap frames (gap
    frames holding numbers): start 2.9e-3 / 2.6e-2 / 1.4e-1; res0 2.0e-2 / 1.3e-1 / 0.95; res3 4.3e-2 / 9.7e-2 / 0.91; res6
    1.6e-1 / 1.6e-1 / 1.3; too long 2.9e-1 / 3.0e-1 / 1.9; and, packed only, the mel not cleared on the gap frames 8.0e-1 /
    9.1e-1 / 2.0.  The smallest ratio to a bound is the start conv's: edge 1.7e-2 = 680 x the fp32 bound, 1100 x f16x3's,
    8.5 x fp16's (abs 1.1e-1 = 3.7 x fp16's)."""
    mel, z = wc.rows_inputs(case, nan=False)
    solo = _solo_acts(case, mel, z)
    rm, rz, real = _run_layout(case, mel, z, fill=np.random.default_rng(3))
    kw = dict(mistake)
    if kw.pop('longer', 0):
        grown = real.copy()
        grown[:, 1:] |= real[:, :-1]                                # every row one frame longer (into its tail or its gap)
        real = grown
    e = _worst_per_row(case, _masked_acts(rm, rz, real, **kw), solo)
    print(f'{case.name} {name}: rel {e["rel"]:.1e} edge {e["edge"]:.1e} abs {e["abs"]:.1e}')
    assert _exceeds(e, 100, ('f32', 'f16x3')) and _exceeds(e, 3, ('f16',)), e


def test_control_three_gap_frames_break_the_per_row_bounds():
    """The packed row built with 3 gap frames instead of 4 and otherwise correct: the d = 128 taps of layer 7 reach 4 frames,
    across the gap into the neighbouring row.  Measured (lengths (13, 5, 9)): rel 2.6e-1 / edge 2.6e-1 / abs 1.9 (130 x fp16's
    edge bound); with 4 frames the control above holds bit for bit."""
    from waveglow_packed_ref import packing_plan
    case = CTRL_PACKED
    mel, z = wc.rows_inputs(case, nan=False)
    solo = _solo_acts(case, mel, z)
    rm, rz, real = _run_layout(case, mel, z, gap=3, fill=np.random.default_rng(3))
    e = _worst_per_row(case, _masked_acts(rm, rz, real), solo, starts=packing_plan(case.lengths, case.T, 3)['starts'])
    print(f'3 gap frames: rel {e["rel"]:.1e} edge {e["edge"]:.1e} abs {e["abs"]:.1e}')
    assert _exceeds(e, 100, ('f32', 'f16x3')) and _exceeds(e, 3, ('f16',)), e


# (twelve flows in float64, three times over: the smallest rows that have a tail, a gap and a row that fills its T)
CTRL_STATE = wc.RowsCase('ctrl_r3x3', 3, 3, (3, 1, 2))


@pytest.mark.parametrize('case', [CTRL_STATE, CTRL_STATE._replace(name='ctrl_p14', packed=True)], ids=lambda c: c.name)
def test_control_an_unmasked_tail_leaves_state_behind_a_length(case):
    """The state checks: with z masked in the init step and the state cleared by every flow's end kernel, the state after
    flows 11, 8, 4 and 0 is exactly 0 on every frame that is not real and the row's own state on the others; z not masked,
    or the end kernel not clearing, leaves non-zero state there -- which the activations above cannot show."""
    from oracle import waveglow_ref
    from waveglow_packed_ref import infer_packed
    mel, z = wc.rows_inputs(case, nan=False)
    rm, rz, real = _run_layout(case, mel, z, fill=np.random.default_rng(3))
    w = wc.weights64(wc.STATE_END_SCALE)
    good, no_z, no_end = {}, {}, {}
    infer_packed(rm, rz, real, w, wc.config(), dtype=np.float64, states=good)
    infer_packed(rm, rz, real, w, wc.config(), dtype=np.float64, states=no_z, mask_z=False)
    infer_packed(rm, rz, real, w, wc.config(), dtype=np.float64, states=no_end, mask_state=False)
    for k in (11, 8, 4, 0):
        layout = lambda s: s[k][0] if case.packed else s[k]
        assert not wc.not_real(case, layout(good)).any(), k
        assert wc.not_real(case, layout(no_end)).any(), k
        # the early outputs that flows 8 and 4 prepend are z's: they show an unmasked z even where the state was cleared
        assert wc.not_real(case, layout(no_z)).any() == (k in (8, 4)), k
    # the real positions: every row against the same arithmetic on its own frames (no frame masked), and the last row --
    # behind a tail, or behind a gap -- against the oracle's own intermediates as well
    for b, n in enumerate(case.lengths):
        own_mel, own_z = mel[b:b + 1, :n].astype(np.float64), z[b:b + 1, :n * wc.NPH].astype(np.float64)
        alone = {}
        infer_packed(own_mel, own_z, np.ones((1, n)), w, wc.config(), dtype=np.float64, states=alone)
        if b == case.B - 1:
            _, inter = waveglow_ref.infer(own_mel, wc.weights(wc.STATE_END_SCALE), wc.config(), z=own_z, sigma=1.0,
                                          dtype=np.float64, return_intermediates=True)
        for k in (11, 8, 4, 0):
            got = wc.row_of(case, good[k][0] if case.packed else good[k], b)
            for ref in (alone[k],) + ((inter[f'audio_after_flow_{k}'],) if b == case.B - 1 else ()):
                e = wc.state_errors(got, ref)                       # (float64 rounding: the matrix products block by shape)
                assert e['rel'] <= 1e-12 and e['max_rel'] <= 1e-12, (b, k, e)


def test_edge_windows_and_state_widths():
    m = wc.edge_mask(3, 64)
    assert m.sum() == 96 and wc.edge_mask(3, 1).sum() == 2 and wc.edge_mask(3, 4)[[0, 3, 4, 91, 92, 95]].tolist() == \
        [True, True, False, False, True, True]
    ref = wc.states(wc.CASE_BY_NAME[wc.STATE_CASES[0]])
    assert {k: v.shape[2] for k, v in ref.items()} == {11: 4, 8: 6, 4: 8, 0: 8}
