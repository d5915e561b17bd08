"""CPU half of the decoder-variant matrix (tests/decoder_cases.py): the case table reaches every instantiation of the three
decoder machines, and every case could fail -- oracle-only controls showing that the regression bounds of
test_decoder_variants_gpu.py would catch a wrong frame, a wrong chunk edge, a dropped long-input half, a lost speaker
embedding or an ignored fp16 flag.  For the attention-window cases: the oracle's arg max is decided by a margin far above any
machine's error, the window changes the frames, both clamps and the free range occur, and the window keeps moving."""
import numpy as np
import pytest

import decoder_cases as dc

PRECISIONS = ('f32', 'f16')

# ---- expected instantiations, read off the switch statements ------------------------------------------------------------
# taco_persist.hip dispatch_persist: (NBT, KT) cases of `switch (NBT * 16 + KT)`; HW = fp16 weights; enc is a run-time
# argument of the kernel, listed because the PM fold differs
PERSIST_SWITCH = [(1, 2), (1, 4), (1, 8), (2, 2), (2, 4), (4, 2)]
PERSIST_EXPECTED = {(n, k, enc, hw) for n, k in PERSIST_SWITCH for enc in (512, 768) for hw in (False, True)}
# taco_fused.hip fused_enqueue_chunk: chunk_t<NBT, ENC, HW> for key 0..7, each with launch_y_kt's KT 1 / 2
FUSED_SWITCH = [(4, 512, False), (4, 512, True), (4, 768, False), (4, 768, True),
                (8, 512, False), (8, 512, True), (8, 768, False), (8, 768, True)]
FUSED_EXPECTED = {(n, enc, kt, hw) for n, enc, hw in FUSED_SWITCH for kt in (1, 2)}
# tacotron2.hip lstm_dispatch_p: KS 7 / 8 / 10 / 11; lstm_by_batch: NBT 1 / 2 / 4 / 8; lstm_dispatch: HW false / true
GRAPH_EXPECTED = {(ks, n, hw) for ks in (7, 8, 10, 11) for n in (1, 2, 4, 8) for hw in (False, True)}


def _all_variants():
    for c in dc.CASES:
        for p in PRECISIONS:
            for m, v in dc.machines(c, p):
                yield c, p, m, v


def test_cases_reach_every_persistent_instantiation():
    got = {v.inst for _, _, m, v in _all_variants() if m == 'persistent'}
    assert got == PERSIST_EXPECTED, sorted(PERSIST_EXPECTED - got)


def test_cases_reach_every_fused_instantiation_and_the_two_pairs_branch():
    got = {v.inst for _, _, m, v in _all_variants() if m == 'fused'}
    assert got == FUSED_EXPECTED, sorted(FUSED_EXPECTED - got)
    rows = {c.B for c, _, m, v in _all_variants() if m == 'fused' and v.two_pairs}
    assert 8 in rows and rows & {5, 6, 7}, rows                 # full and partially filled 8-row tiles
    encs = {c.enc for c, _, m, v in _all_variants() if m == 'fused' and v.two_pairs}
    assert encs == {512, 768}


def test_cases_reach_every_graph_instantiation_and_more_than_8_rows():
    got = set()
    for _, _, m, v in _all_variants():
        if m == 'graph':
            got |= set(v.inst)
    assert got == GRAPH_EXPECTED, sorted(GRAPH_EXPECTED - got)
    big = {(c.enc, p) for c, p, m, _ in _all_variants() if m == 'graph' and c.B > 8}
    assert big == {(e, p) for e in (512, 768) for p in PRECISIONS}


def test_pick_variant_restates_the_dispatch_rules_at_their_edges():
    pv = dc.pick_variant
    assert pv('persistent', 1, 128, 512, 'f32').inst == (1, 2, 512, False)
    assert pv('persistent', 1, 129, 512, 'f32').inst == (1, 4, 512, False)
    assert pv('persistent', 1, 257, 512, 'f16').inst == (1, 8, 512, True)
    assert pv('persistent', 1, 513, 512, 'f32') is None
    assert pv('persistent', 2, 257, 512, 'f32') is None                 # NBT 2 stops at KT 4
    assert pv('persistent', 3, 129, 512, 'f32') is None                 # NBT 4 stops at KT 2
    assert pv('persistent', 5, 10, 512, 'f32') is None
    assert pv('fused', 1, 256, 768, 'f32').inst == (4, 768, 2, False)
    assert pv('fused', 5, 1, 512, 'f32') is None and pv('fused', 5, 257, 512, 'f32') is None
    assert pv('fused', 9, 10, 512, 'f32') is None
    assert not pv('fused', 8, 128, 512, 'f16').two_pairs                # KT 1: one pair per wave
    assert not pv('fused', 8, 129, 512, 'f32').two_pairs                # fp32 weights
    assert pv('fused', 8, 129, 512, 'f16').two_pairs                    # 1032 > 1024 pairs
    assert not pv('fused', 5, 200, 512, 'f16').two_pairs                # 1000 pairs
    assert pv('graph', 11, 40, 768, 'f16').inst == ((8, 4, True), (8, 8, True), (11, 4, True), (11, 8, True))
    assert pv('auto', 2, 100, 512, 'f32').machine == 'persistent'
    assert pv('auto', 3, 100, 512, 'f32').machine == 'fused'
    assert pv('auto', 3, 200, 512, 'f32').machine == 'fused'            # persistent does not apply
    assert pv('auto', 1, 300, 512, 'f32').machine == 'persistent'       # fused does not apply
    assert pv('auto', 2, 300, 512, 'f32').machine == 'graph'
    assert pv('auto', 11, 40, 512, 'f32').machine == 'graph'


def test_required_shapes_are_in_the_table():
    shapes = {(c.B, c.Tin, c.enc) for c in dc.CASES}
    lens = {(c.B, c.max_len) for c in dc.CASES}
    assert {(3, 63), (3, 64), (3, 65), (3, 129), (8, 63), (8, 64), (8, 65), (8, 129)} <= lens
    assert {128, 129, 256, 257, 512, 513} <= {t for b, t, e in shapes if b == 1}
    assert {(b, t) for b in (2, 4, 5, 8) for t in (100, 200)} <= {(b, t) for b, t, e in shapes if e == 768}
    assert {(5, 250, 512), (7, 150, 512), (8, 256, 512)} <= shapes
    assert {(11, 512), (11, 768)} <= {(b, e) for b, t, e in shapes}
    edges = {(max(c.targets) + 1) for c in dc.CASES if c.early_stopping}
    assert {33, 64, 65} <= edges                                         # loop ends just past / on a chunk edge


# ---- sensitivity controls ------------------------------------------------------------------------------------------------
CASE_IDS = [c.name for c in dc.CASES]


def _steps(case, ref):
    return min(case.max_len, int(ref.lengths.max()) + 1) if case.early_stopping else case.max_len


@pytest.mark.parametrize('name', CASE_IDS)
def test_consecutive_frames_differ_far_beyond_the_bound(name):
    """A machine that repeated the previous frame or state -- at a chunk edge (32/33, 64/65, 128/129) or anywhere else --
    must fail the frame bound: every pair of consecutive reference frames differs by >= 20x MEL_REG (the prenet masks
    keep late frames moving)."""
    case = dc.CASE_BY_NAME[name]
    ref = dc.reference(case)
    T = _steps(case, ref)
    d = np.abs(np.diff(ref.decoder_output[:, :T], axis=1)).max(-1)          # [B, T - 1]: frame t + 1 vs frame t
    for e in dc.chunk_edges(case, T):
        print(f'{name}: chunk edge {e}/{e + 1}: smallest consecutive-frame change {d[:, e - 1].min():.2e}')
    assert d.min() >= 20 * dc.MEL_REG, (d.min(), np.unravel_index(d.argmin(), d.shape))


@pytest.mark.parametrize('name', [c.name for c in dc.CASES if c.Tin > 128 and c.win is None])     # (a window confines the mass)
def test_long_inputs_put_attention_past_position_128(name):
    """In rows longer than 128 tokens, the positions >= 128 carry at least 10 % of the attention mass (for 129 - 150
    tokens: at least half of what uniform attention would put there), and dropping them would move the attention far
    beyond its RMS bound."""
    case = dc.CASE_BY_NAME[name]
    ref = dc.reference(case)
    a = ref.attention_weights[:, :_steps(case, ref)].astype(np.float64)
    long_rows = [b for b, n in enumerate(dc.lens_of(case)) if n > 128]
    assert long_rows
    for b in long_rows:
        n = dc.lens_of(case)[b]
        frac = a[b, :, 128:].sum() / a[b].sum()
        assert frac >= min(0.1, 0.5 * (n - 128) / n), (b, frac)
    cut = a.copy()
    cut[:, :, 128:] = 0
    assert dc.attention_rms_rel(cut, a) >= 20 * dc.ATT_REG


@pytest.mark.parametrize('name', [c.name for c in dc.CASES if c.enc == 768])
def test_speaker_embedding_moves_the_frames(name):
    """enc 768: the speaker part of the context matters -- a zero embedding changes the first frames by >> MEL_REG."""
    case = dc.CASE_BY_NAME[name]
    T = min(8, case.max_len)
    ref, zero = dc.reference(case), dc.reference(case, zero_speaker=True, max_len=T)
    d = float(np.abs(zero.decoder_output - ref.decoder_output[:, :T]).max())
    assert d >= 100 * dc.MEL_REG, d


@pytest.mark.parametrize('name', CASE_IDS)
def test_fp16_references_are_far_from_fp32(name):
    """The rounded-weight reference of every machine that runs the case in fp16 differs from the fp32 oracle by >= 5x
    MEL_REG, so a machine that ignored the fp16 flag (or rounded other tensors) fails the bound."""
    case = dc.CASE_BY_NAME[name]
    ref = dc.reference(case)
    for kind in {dc.reference_kind(m, 'f16') for m, _ in dc.machines(case, 'f16')}:
        d = float(np.abs(dc.reference(case, kind).mel - ref.mel).max())
        print(f'{name}: {kind} reference vs fp32: mel {d:.2e}')
        assert d >= 5 * dc.MEL_REG, (kind, d)


def test_persistent_fp16_reference_differs_from_the_fully_rounded_one():
    """The persistent kernel keeps the context rows in fp32 (PM fold): its reference is a different computation, further
    from the fully rounded one than the bound -- comparing it with the wrong one would fail."""
    case = dc.CASE_BY_NAME['b3_len64']
    d = float(np.abs(dc.reference(case, 'f16').mel - dc.reference(case, 'f16_ctx32').mel).max())
    assert d >= 2 * dc.MEL_REG, d


def test_round_lstm_f16_touches_exactly_the_four_tensors():
    w = dc.base_weights(768)
    r = dc.round_lstm_f16(w, 768)
    changed = {k for k in w if not np.array_equal(w[k], r[k])}
    assert changed == set(dc.F16_TENSORS)
    for k in dc.F16_TENSORS:
        assert np.array_equal(r[k], w[k].astype(np.float16).astype(np.float32))
    rc = dc.round_lstm_f16(w, 768, keep_ctx=True)
    a = f'{dc.D}/attention_rnn/kernel'
    k = f'{dc.D}/decoder_rnn/cell_0/kernel'
    assert np.array_equal(rc[a][256:1024], w[a][256:1024]) and np.array_equal(rc[a][:256], r[a][:256])
    assert np.array_equal(rc[k][1024:1792], w[k][1024:1792]) and np.array_equal(rc[k][:1024], r[k][:1024])


@pytest.mark.parametrize('name', [c.name for c in dc.CASES if c.early_stopping])
def test_scripted_stops_are_realisable(name):
    """The fitted gate separates every decision with margin >= 0.4 * slope (asserted inside script_stop_tokens), and the
    fp32 oracle and every rounded-weight oracle give exactly the target lengths."""
    case = dc.CASE_BY_NAME[name]
    _, sens, margin = dc.scripted(name)
    print(f'{name}: gate norm {sens:.1f}, logit margin {margin:.2f}')
    assert margin >= 0.8
    for kind in ('f32', 'f16', 'f16_ctx32'):
        ref = dc.reference(case, kind)
        assert ref.lengths.tolist() == list(case.targets), (kind, ref.lengths)
    assert max(case.targets) + 1 < case.max_len                          # the loop ends by the stop tokens


# ---- the attention window ------------------------------------------------------------------------------------------------------
WINDOW_IDS = [c.name for c in dc.WINDOW_CASES]
ARGMAX_GAP = 5e-6               # about 30x the worst attention max-abs error measured on an MI355X (1.8e-7, decoder_cases.ATT_REG)
# the instantiations each window case is there for: machine -> `Variant.inst` without its HW flag, (NBT, KT, enc) persistent /
# (NBT, ENC, KT) fused; 'graph': the rows of the call
WINDOW_REACHES = {
    'win_b3_len66': {'persistent': (4, 2, 512), 'fused': (4, 512, 1), 'graph': 3},
    'win_b8_tin256': {'fused': (8, 512, 2), 'graph': 8},
    'win_b1_tin512': {'persistent': (1, 8, 512), 'graph': 1},
    'win_b2_tin200': {'persistent': (2, 4, 512), 'fused': (4, 512, 2), 'graph': 2},
    'win_b1_tin513': {'graph': 1},
    'win_b11_tin40': {'graph': 11},
    'win_e768_b4_tin100': {'persistent': (4, 2, 768), 'fused': (4, 768, 1), 'graph': 4},
    'win_e768_b1_tin300': {'persistent': (1, 8, 768), 'graph': 1},
    'win_b5_tin129': {'fused': (8, 512, 2), 'graph': 5},
    'win_stop_b3_64': {'persistent': (4, 2, 512), 'fused': (4, 512, 1), 'graph': 3},
}


def _window(name, kind='f32'):
    """(case, ref, steps, prev, lo, hi) of a window case on the oracle with weights rounded as `kind`."""
    case = dc.CASE_BY_NAME[name]
    ref = dc.reference(case, kind)
    T = _steps(case, ref)
    return (case, ref, T, *dc.window_bounds(case, ref.attention_weights[:, :T]))


def test_window_cases_reach_their_machines():
    assert set(WINDOW_REACHES) == set(WINDOW_IDS)
    for name, want in WINDOW_REACHES.items():
        case = dc.CASE_BY_NAME[name]
        for precision in PRECISIONS:
            got = dict(dc.machines(case, precision))
            assert set(got) == set(want), (name, precision, sorted(got))        # exactly these machines accept the shape
            for m, inst in want.items():
                if m == 'graph':
                    assert case.B == inst
                else:
                    assert got[m].inst == (*inst, precision == 'f16'), (name, m, got[m])
    assert dc.pick_variant('fused', 8, 256, 512, 'f16').two_pairs                    # the two-positions-per-wave branch
    assert len(dc.pick_variant('graph', 11, 40, 512, 'f32').inst) == 4               # two LSTM launches (8 + 3 rows) per step
    assert dc.CASE_BY_NAME['win_b11_tin40'].max_len > dc.GRAPH_CHUNK
    for name in ('win_b3_len66', 'win_e768_b4_tin100'):
        assert dc.CASE_BY_NAME[name].max_len > dc.FUSED_CHUNK + 1                    # steps 64 and 65 run in the second chunk


@pytest.mark.parametrize('name', WINDOW_IDS)
def test_window_arg_max_is_decided_with_margin(name):
    """The arg max, and with it the next window, is discontinuous in the weights: on every reference a machine is compared
    with, the two largest weights of every (row, step) differ by >= ARGMAX_GAP, so a correct kernel cannot land in another
    window than the oracle."""
    for kind in ('f32', 'f16', 'f16_ctx32'):
        case, ref, T, prev, lo, hi = _window(name, kind)
        a = np.sort(ref.attention_weights[:, :T].astype(np.float64), axis=-1)
        gap = float((a[..., -1] - a[..., -2]).min())
        print(f'{name}: {kind}: smallest arg-max gap {gap:.2e}')
        assert gap >= ARGMAX_GAP, (kind, gap)
        # the oracle itself keeps to the window it is asked for
        tau = np.arange(case.Tin)
        outside = (tau < lo[..., None]) | (tau > hi[..., None])
        assert np.all(ref.attention_weights[:, :T][outside] == 0)


@pytest.mark.parametrize('name', WINDOW_IDS)
def test_window_bites(name):
    """A machine that ignored the window would give the frames of the call without one: >= 1000x MEL_REG away."""
    case = dc.CASE_BY_NAME[name]
    d = float(np.abs(dc.reference(case).mel - dc.reference(case, windowed=False).mel).max())
    print(f'{name}: mel with the window vs without: {d:.2e}')
    assert d >= 1000 * dc.MEL_REG, d


def test_window_cases_cover_both_clamps_and_keep_moving():
    lower = upper = free = short_rows = 0
    for name in WINDOW_IDS:
        case, ref, T, prev, lo, hi = _window(name)
        win_len, win_off = case.win
        enc_len = np.asarray(dc.lens_of(case))[:, None]
        lo_clamp, hi_clamp = prev < win_off, prev > enc_len - win_len + win_off
        n = (int(lo_clamp.sum()), int(hi_clamp.sum()), int((~lo_clamp & ~hi_clamp).sum()))
        distinct = [len(set(lo[b])) for b in range(case.B)]
        print(f'{name}: row-steps on the lower clamp {n[0]}, on the upper {n[1]}, free {n[2]}; distinct window starts per row '
              f'{distinct}' + ''.join(f'; starts at step {e} {lo[:, e].tolist()}' for e in (32, 64) if e < T))
        lower, upper, free = lower + n[0], upper + n[1], free + n[2]
        short_rows += int((enc_len < win_len).sum())
        if name in ('win_b3_len66', 'win_b8_tin256', 'win_b2_tin200', 'win_b11_tin40'):
            long_rows = [b for b in range(case.B) if enc_len[b, 0] >= 2 * win_len]
            assert long_rows and all(distinct[b] >= 3 for b in long_rows), (name, distinct)
        if name in ('win_b3_len66', 'win_e768_b4_tin100'):
            assert T > 64 and np.any(lo[:, 64] != lo[:, 0]), (name, lo[:, 0], lo[:, 64])    # still moving in the second fused chunk
        if name == 'win_b11_tin40':
            assert np.any(lo[:, 32] != lo[:, 0])                                            # ... and in the second graph chunk
    assert lower and upper and free and short_rows, (lower, upper, free, short_rows)
