"""GPU: properties of the decoder's attention window (`attn_mask_win_len` / `attn_mask_offset`) that need no oracle, on each
of the three decoder machines (tests/decoder_cases.py restates which shapes each accepts) and in both precisions.  Every call
asserts the machine that ran.  Bit equalities only: both sides of every comparison run on the same machine and precision.

- a window wider than every row only ANDs ones into the mask: the call equals the one without a window;
- no window state survives a call: the arg max of the last call, the parity of its ping-pong buffer and the cached chunk
  graphs (keyed by the window) leave no trace in the next one, nor in the next sentence encoded into the same batch;
- masks drawn on the device and the window meet in one call as they do apart;
- the runtime resolves a fractional offset as the reference does.

The accuracy of the windowed decoder against the oracle is tests/test_decoder_variants_gpu.py."""
import numpy as np
import pytest

import decoder_cases as dc

pytestmark = pytest.mark.gpu

OUTPUTS = ('decoder_output', 'mel', 'stop_tokens', 'attention_weights', 'lengths')
MODES = ('persistent', 'fused', 'graph')
PRECISIONS = ('f32', 'f16')


def _inputs(B, Tin, T, seed):
    """Tokens [B, Tin] with the ragged rows of the case table, and prenet masks [B, T, 2, 256]."""
    case = dc.Case('adhoc', B, Tin, T, seed=seed)
    tok, _, masks = dc.inputs(case)
    return tok, masks, dc.lens_of(case)


def _modes(B, Tin):
    """Decoder modes whose machine accepts the shape (the others would fall back to the graph)."""
    return [m for m in MODES if dc.pick_variant(m, B, Tin, 512, 'f32') is not None]


class _mode:
    """`with _mode(eng, m) as ran:` -- decoder mode m for the block, 'auto' after it; `ran(what)` asserts that m ran."""

    def __init__(self, eng, mode):
        self.eng, self.mode = eng, mode

    def __enter__(self):
        self.eng.set_decoder_mode(self.mode)

        def ran(what):
            assert self.eng.last_decoder_mode == self.mode, f'{what}: asked for {self.mode}, ran {self.eng.last_decoder_mode}'
        return ran

    def __exit__(self, *exc):
        self.eng.set_decoder_mode('auto')


def _same(a, b, what):
    for name, u, v in zip(OUTPUTS, a, b):
        assert u.shape == v.shape and np.array_equal(u, v), \
            f'{what}: {name} differs at {np.argwhere(np.asarray(u) != np.asarray(v))[:3].tolist()}'
    assert np.isfinite(a.mel).all() and a.mel.any()


@pytest.mark.parametrize('B,Tin', [(3, 60), (2, 200), (8, 129)])
def test_a_window_wider_than_every_row_is_no_window(gpu_engine, B, Tin):
    T = 34
    tok, masks, _ = _inputs(B, Tin, T, seed=11)
    win = Tin + 5
    modes = _modes(B, Tin)
    assert {(3, 60): 3, (2, 200): 3, (8, 129): 2}[B, Tin] == len(modes)
    for mode in modes:
        for prec in PRECISIONS:
            kw = dict(max_len=T, early_stopping=False, prenet_masks=masks, precision=prec)
            with _mode(gpu_engine, mode) as ran:
                plain = gpu_engine.tacotron2_infer(tok, **kw)
                ran(f'{prec} no window')
                for off in (0, win // 2):
                    wide = gpu_engine.tacotron2_infer(tok, attn_mask_win_len=win, attn_mask_offset=off, **kw)
                    ran(f'{prec} window {win} offset {off}')
                    _same(wide, plain, f'{mode} {prec}: window {win} offset {off} against no window')


WIN_A, WIN_B = (12, 6), (8, 2)


@pytest.mark.parametrize('prec', PRECISIONS)
@pytest.mark.parametrize('mode,T', [('graph', 34), ('fused', 66), ('persistent', 34)])
def test_no_window_state_survives_a_call(gpu_engine, mode, T, prec):
    """34 steps replay the graph's second chunk from the cache, 66 steps run the fused step's second chunk."""
    B, Tin = 3, 60
    assert mode in _modes(B, Tin)
    tok, masks, _ = _inputs(B, Tin, T, seed=12)
    other, _, _ = _inputs(B, Tin, T, seed=13)
    assert not np.array_equal(tok, other)
    kw = dict(max_len=T, early_stopping=False, prenet_masks=masks, precision=prec)
    win = lambda w: {} if w is None else dict(attn_mask_win_len=w[0], attn_mask_offset=w[1])
    with _mode(gpu_engine, mode) as ran:
        enc = gpu_engine.tacotron2_encode(tok)
        try:
            outs = []
            for w in (WIN_A, WIN_A, WIN_B, None, WIN_A):
                outs.append(gpu_engine.tacotron2_decode(enc, **kw, **win(w)))
                ran(f'{prec} window {w}')
            a1, a2, b, none, a3 = outs
            _same(a2, a1, f'{mode} {prec}: window A twice')
            _same(a3, a1, f'{mode} {prec}: window A after window B and no window')
            for what, x in (('window B', b), ('no window', none)):
                assert not np.array_equal(x.mel, a1.mel) and not np.array_equal(x.attention_weights, a1.attention_weights), what
            assert not np.array_equal(b.mel, none.mel)
            gpu_engine.tacotron2_encode(other, into=enc)
            again = gpu_engine.tacotron2_decode(enc, **kw, **win(WIN_A))
            ran(f'{prec} the next sentence')
        finally:
            enc.close()
        fresh = gpu_engine.tacotron2_infer(other, **kw, **win(WIN_A))
        ran(f'{prec} the next sentence, fresh')
        _same(again, fresh, f'{mode} {prec}: the next sentence in the same batch against a fresh call')
        assert not np.array_equal(fresh.mel, a1.mel)


@pytest.mark.parametrize('mode,B,Tin', [('persistent', 2, 40), ('fused', 5, 40), ('graph', 11, 24)])
def test_seeded_masks_with_a_window(gpu_engine, mode, B, Tin):
    from oracle import philox_ref
    T, seed, offset = 20, 41, 6
    assert mode in _modes(B, Tin)
    tok, _, _ = _inputs(B, Tin, T, seed=14)
    keys, offs = [1000 + 17 * b for b in range(B)], [3 * b for b in range(B)]
    whole = philox_ref.prenet_masks(B * T * 512, seed, offset).reshape(B, T, 2, 256)
    rows = np.stack([philox_ref.prenet_masks(T * 512, k, o) for k, o in zip(keys, offs)]).reshape(B, T, 2, 256)
    for prec in PRECISIONS:
        kw = dict(max_len=T, early_stopping=False, precision=prec, attn_mask_win_len=8, attn_mask_offset=2)
        with _mode(gpu_engine, mode) as ran:
            enc = gpu_engine.tacotron2_encode(tok)
            try:
                explicit = gpu_engine.tacotron2_decode(enc, prenet_masks=whole, **kw)
                seeded = gpu_engine.tacotron2_decode(enc, mask_seed=(seed, offset), **kw)
                ran(f'{prec} mask_seed')
                _same(seeded, explicit, f'{mode} {prec}: mask_seed with a window')
                explicit_rows = gpu_engine.tacotron2_decode(enc, prenet_masks=rows, **kw)
                by_row = gpu_engine.tacotron2_decode(enc, row_mask_seeds=(keys, offs), **kw)
                ran(f'{prec} row_mask_seeds')
                _same(by_row, explicit_rows, f'{mode} {prec}: row_mask_seeds with a window')
                assert not np.array_equal(by_row.mel, seeded.mel)
                unwindowed = gpu_engine.tacotron2_decode(enc, mask_seed=(seed, offset), max_len=T, early_stopping=False, precision=prec)
                assert not np.array_equal(unwindowed.mel, seeded.mel)                    # the window was applied
            finally:
                enc.close()


@pytest.mark.parametrize('win,fraction,positions', [(13, 0.5, 6), (7, 0.3, 2)])
def test_runtime_resolves_a_fractional_offset(gpu_engine, win, fraction, positions):
    """int(float32(win_len) * float32(offset)), tacotron2_arch.py:894-897."""
    from text_to_speech_amd.runtime import HipRuntime
    T = 20
    tok, masks, _ = _inputs(3, 60, T, seed=15)
    rt = HipRuntime('unused', engine=gpu_engine, model='tacotron2')
    for mode in _modes(3, 60):
        with _mode(gpu_engine, mode) as ran:
            got = rt(tok, max_length=T, early_stopping=False, prenet_masks=masks, attn_mask_win_len=win, attn_mask_offset=fraction)
            ran('the runtime')
            kw = dict(max_len=T, early_stopping=False, prenet_masks=masks, attn_mask_win_len=win)
            _same(got, gpu_engine.tacotron2_infer(tok, attn_mask_offset=positions, **kw), f'{mode}: {win} x {fraction}')
            near = gpu_engine.tacotron2_infer(tok, attn_mask_offset=positions + 1, **kw)
            assert not np.array_equal(near.attention_weights, got.attention_weights)    # one position further is another call
