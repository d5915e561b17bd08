"""Shared case table of the decoder-variant tests (tests/test_decoder_variants.py on the CPU, _gpu.py on an MI355X).

The three decoder machines -- the persistent kernel (csrc/taco_persist.hip), the fused two-kernel step replayed in 64-step
chunks (csrc/taco_fused.hip) and the 7-kernel per-step graph replayed in 32-step chunks (csrc/tacotron2.hip) -- are each
compiled into many template instantiations.  `pick_variant` restates their dispatch rules, so a test can say which
instantiation a call must take and check that the case table reaches every one of them.  `WINDOW_CASES` run the attention
window (`Case.win`), which each machine implements on its own, on every machine and precision their shapes allow.

References come from the numpy oracle, once per case and weight rounding (`reference`):
- 'f32': the oracle as it is;
- 'f16': the four decoder-LSTM tensors (attention / decoder LSTM kernel and recurrent_kernel) rounded to fp16 with RNE, as
  `cvt_w16_kernel` does -- the exact-arithmetic reference of the fp16 mode of the fused step and the per-step graph;
- 'f16_ctx32': the same, but the context rows of both LSTM kernels stay fp32.  The persistent kernel folds those rows
  into the per-utterance PM table from the fp32 weights (tacotron2.hip, `parts` of run_persistent) and streams
  only the prenet / h_att / h_dec rows in fp16.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

# ---- bounds ------------------------------------------------------------------------------------------------------------
MEL_TOL = 1e-3              # north star (BASELINE.json): mel, decoder frames and attention weights, max abs
# Regression bounds: about 10x the worst error measured on an MI355X over every case x machine x precision of
# test_decoder_variants_gpu.py (fp16 calls against the rounded-weight reference, fp32 calls against the fp32 oracle).
MEL_REG = 3e-5              # frames (decoder_output, mel) and fixed-step stop tokens, max abs: measured 2.71e-6 (mel, b8_len63,
                            # fp16, graph; fp32 worst 2.68e-6, b8_tin256, graph); stop tokens 6.7e-8
                            # window cases: mel 2.62e-6 (win_stop_b3_64, fp16, fused), frames 1.79e-6 (win_stop_b3_64, fp32,
                            # persistent), stop tokens 6.7e-8 (win_b3_len66, fp16, persistent)
ATT_REG = 2.5e-6            # attention weights, RMS of the error / RMS of the reference: measured 2.24e-7 (e768_b1_tin100,
                            # fp16, persistent); max abs 1.64e-7
                            # window cases: 2.18e-7 (win_stop_b3_64, fp32, persistent); max abs 1.79e-7 (win_b5_tin129, fp32,
                            # fused: two positions share the mass, so the weights are large)
STOP_REG = 4e-6             # scripted-stop cases: stop-token bound per unit of the fitted gate's norm (`sensitivity`):
                            # measured 3.62e-7 (stop_b2_33, fp16, persistent); window case 2.30e-7 (win_stop_b3_64, fp16, fused)

GRAPH_CHUNK, FUSED_CHUNK = 32, 64       # tacotron2.hip CHUNK, taco_fused.h FUSED_CHUNK
N_CU = 256                              # MI355X; both whole-GPU machines need 256 resident blocks

D = 'tacotron2/decoder'
F16_TENSORS = (f'{D}/attention_rnn/kernel', f'{D}/attention_rnn/recurrent_kernel',
               f'{D}/decoder_rnn/cell_0/kernel', f'{D}/decoder_rnn/cell_0/recurrent_kernel')


# ---- dispatch rules ----------------------------------------------------------------------------------------------------
class Variant(NamedTuple):
    machine: str                # 'persistent' | 'fused' | 'graph'
    inst: tuple                 # persistent (NBT, KT, enc, HW); fused (NBT, ENC, KT, HW); graph ((KS, NBT, HW), ...)
    two_pairs: bool = False     # fused: the fp16 two-positions-per-wave branch of fused_y_kernel


def _persist_lds_bytes(NBT, KT, Tin):
    # taco_persist.hip persist_lds_bytes: RNN 1024, PRE 256, LOCK 31, ATT 128, PMW 36
    TP = KT * 64
    WS = TP + 32
    return (NBT * (2 * 1024 + 256 + TP + 2 * WS) + 2 * 31 * 128 + NBT * Tin * 36 + 4) * 4


def _persist(B, Tin, enc, hw):
    # taco_persist.hip pick_shape, persist_applicable and the dispatch_persist switch above them
    if B < 1 or B > 4 or Tin < 1 or Tin > 512:
        return None
    NBT = 1 if B <= 1 else 2 if B <= 2 else 4
    KT = 2 if Tin <= 128 else 4 if Tin <= 256 else 8
    if (NBT == 2 and KT > 4) or (NBT == 4 and KT > 2):
        return None
    if _persist_lds_bytes(NBT, KT, Tin) > 160 * 1024:
        return None
    return Variant('persistent', (NBT, KT, enc, hw))


def _fused(B, Tin, enc, hw):
    # taco_fused.hip pick_shape, fused_applicable, lds_x / lds_y, and the chunk_t switch of fused_enqueue_chunk
    if B < 1 or B > 8 or Tin < 2 or Tin > 256 or enc not in (512, 768):
        return None
    NBT = 4 if B <= 4 else 8
    KT = 1 if Tin <= 128 else 2
    lds_x = (NBT * (2 * 1024 + enc) + NBT * 256 + 8) * 4
    lds_y = (NBT * (2 * 1024 + enc) + 2 * 31 * 128 + 4 * KT * 128 * 9 + 16) * 4
    if lds_x > 160 * 1024 or lds_y > 160 * 1024:
        return None
    # taco_fused.hip fused_y_kernel: NPOS = (NBT * KT * 128 + 1023) / 1024 and two_pairs = NPOS > 1 && HW && B * Tin > 4 * NBLK
    npos = (NBT * KT * 128 + 1023) // 1024
    return Variant('fused', (NBT, enc, KT, hw), two_pairs=npos > 1 and hw and B * Tin > 4 * N_CU)


def _graph(B, enc, hw):
    # tacotron2.hip lstm_dispatch_p switches on KS = (n0 + n1 + units) / 256 -- attention LSTM
    # [p2 256 | ctx enc | h_att 1024], decoder LSTM [h_att 1024 | ctx enc | h_dec 1024] -- and lstm_by_batch launches
    # one kernel per chunk of <= 8 rows, NBT 1 / 2 / 4 / 8 by the chunk's row count
    ks = ((256 + enc + 1024) // 256, (1024 + enc + 1024) // 256)
    nbts = set()
    for b0 in range(0, B, 8):
        nb = min(8, B - b0)
        nbts.add(1 if nb == 1 else 2 if nb == 2 else 4 if nb <= 4 else 8)
    return Variant('graph', tuple(sorted((k, n, hw) for k in ks for n in nbts)))


def pick_variant(machine, B, Tin, enc, precision) -> Optional[Variant]:
    """The instantiation a call takes under decoder mode `machine`, or None when that machine does not accept the call
    (it then falls back to the graph).  'auto' restates choose_decoder_machine (tacotron2.hip): persistent for 1 - 2 rows,
    fused above, whichever applies otherwise, the graph when neither does."""
    hw = precision == 'f16'
    if machine == 'persistent':
        return _persist(B, Tin, enc, hw)
    if machine == 'fused':
        return _fused(B, Tin, enc, hw)
    if machine == 'graph':
        return _graph(B, enc, hw)
    if machine == 'auto':
        p, f = _persist(B, Tin, enc, hw), _fused(B, Tin, enc, hw)
        if p and f:
            return p if B <= 2 else f
        return p or f or _graph(B, enc, hw)
    raise ValueError(machine)


def reference_kind(machine, precision):
    """Which oracle reference a machine's output is compared with."""
    if precision == 'f32':
        return 'f32'
    return 'f16_ctx32' if machine == 'persistent' else 'f16'


def round_lstm_f16(weights, enc=None, keep_ctx=False):
    """The four decoder-LSTM tensors rounded to fp16 (RNE) and back; everything else unchanged.  `keep_ctx` leaves the
    context rows of both kernels (rows 256 : 256 + enc of the attention LSTM, 1024 : 1024 + enc of the decoder LSTM)
    in fp32, as the persistent kernel's PM fold does."""
    out = dict(weights)
    for name in F16_TENSORS:
        w = np.asarray(weights[name], np.float32)
        r = w.astype(np.float16).astype(np.float32)
        if keep_ctx and name.endswith('/kernel'):
            lo = 256 if 'attention_rnn' in name else 1024
            r[lo:lo + enc] = w[lo:lo + enc]
        out[name] = r
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    B: int
    Tin: int
    max_len: int
    enc: int = 512
    targets: Optional[tuple] = None     # scripted stops (tests/stop_script.py): early stopping with these `lengths`
    seed: int = 0
    win: Optional[tuple] = None         # attention window (win_len, win_off), integers as the C API takes them

    @property
    def early_stopping(self):
        return self.targets is not None

    @property
    def win_kwargs(self):
        """The window as keyword arguments of `tacotron2_ref.infer` and of `HipEngine.tacotron2_infer` alike."""
        return {} if self.win is None else dict(attn_mask_win_len=self.win[0], attn_mask_offset=self.win[1])


_C = Case
CASES = (
    # max_len around the fused chunk (64) and past two of them, batches 3 (4-row kernels) and 8 (8-row kernels)
    _C('b3_len63', 3, 60, 63), _C('b3_len64', 3, 60, 64), _C('b3_len65', 3, 60, 65), _C('b3_len129', 3, 128, 129),
    _C('b8_len63', 8, 90, 63), _C('b8_len64', 8, 90, 64), _C('b8_len65', 8, 90, 65), _C('b8_len129', 8, 129, 129),
    # token counts at the KT switches: 128 / 129 (persistent 2 -> 4, fused 1 -> 2), 256 / 257 (persistent 4 -> 8; the
    # fused step stops applying), 512 / 513 (the persistent kernel stops applying)
    _C('b1_tin128', 1, 128, 40), _C('b1_tin129', 1, 129, 40), _C('b1_tin256', 1, 256, 70), _C('b1_tin257', 1, 257, 40),
    _C('b1_tin512', 1, 512, 70), _C('b1_tin513', 1, 513, 40),
    _C('b2_tin40', 2, 40, 33), _C('b2_tin200', 2, 200, 40),
    # the fp16 two-positions-per-wave branch of the fused step, partially filled and full 8-row tiles
    _C('b5_tin250', 5, 250, 40), _C('b7_tin150', 7, 150, 40), _C('b8_tin256', 8, 256, 66),
    # enc 768 (256-d speaker embedding)
    _C('e768_b1_tin100', 1, 100, 40, 768), _C('e768_b1_tin200', 1, 200, 40, 768), _C('e768_b1_tin300', 1, 300, 40, 768),
    _C('e768_b2_tin100', 2, 100, 40, 768), _C('e768_b2_tin200', 2, 200, 40, 768),
    _C('e768_b4_tin100', 4, 100, 66, 768), _C('e768_b4_tin200', 4, 200, 40, 768),
    _C('e768_b5_tin100', 5, 100, 40, 768), _C('e768_b5_tin200', 5, 200, 40, 768),
    _C('e768_b8_tin100', 8, 100, 40, 768), _C('e768_b8_tin200', 8, 200, 70, 768),
    # more than 8 rows: two LSTM launches per step on the graph (8 + 3 rows)
    _C('b11_tin40', 11, 40, 33), _C('e768_b11_tin40', 11, 40, 40, 768),
    # scripted stops at the chunk edges: the loop ends one step into the fused step's second chunk (65 steps), on the
    # last step of the first fused chunk (64 steps: the stop is seen through n_fin) and one step into the second graph
    # chunk (33 steps); max_len leaves chunks in flight that must do nothing
    _C('stop_b8_65', 8, 256, 200, targets=(63, 20, 64, 10, 5, 3, 12, 2), seed=1),
    _C('stop_b3_64', 3, 100, 129, targets=(31, 63, 33), seed=2),
    _C('stop_b2_33', 2, 150, 100, targets=(32, 31), seed=3),
)
# The attention window (win_len, win_off): the arg max of step t's alignment, an integer, decides which energies step t + 1
# masks -- implemented once per machine.  Seeds and windows are chosen so that the conditions of test_decoder_variants.py
# hold on the oracle alone: arg-max gap, the window bites, both clamps and the free range occur, the window keeps moving.
WINDOW_CASES = (
    # fused NBT 4 / KT 1 and persistent NBT 4; the window still moves across the graph (32) and fused (64) chunk edges; the
    # row of 20 tokens sits on the upper clamp
    _C('win_b3_len66', 3, 60, 66, win=(12, 6)),
    # fused NBT 8 / KT 2 and its fp16 two-positions-per-wave branch; rows of 5 and 11 tokens are shorter than the window (lo < 0)
    _C('win_b8_tin256', 8, 256, 40, win=(16, 8), seed=1),
    _C('win_b1_tin512', 1, 512, 40, win=(40, 20), seed=3),                  # persistent KT 8
    _C('win_b2_tin200', 2, 200, 40, win=(24, 0)),                           # persistent NBT 2 / KT 4, fused KT 2; offset 0
    _C('win_b1_tin513', 1, 513, 40, win=(24, 8)),                           # graph only: stride-256 loops and their tail
    _C('win_b11_tin40', 11, 40, 34, win=(8, 2)),                            # graph, two LSTM launches, past its 32-step chunk
    _C('win_e768_b4_tin100', 4, 100, 66, 768, win=(12, 2)),                 # enc 768: fused ENC 768 and persistent
    _C('win_e768_b1_tin300', 1, 300, 40, 768, win=(2, 1)),                  # three positions; graph and persistent KT 8
    _C('win_b5_tin129', 5, 129, 40, win=(1, 0)),                            # two positions (inclusive upper bound); fused NBT 8 / KT 2
    # scripted stops with the window: finished rows keep moving their arg max until every row has fired
    _C('win_stop_b3_64', 3, 100, 129, targets=(31, 63, 33), seed=2, win=(12, 6)),
)
CASES += WINDOW_CASES
CASE_BY_NAME = {c.name: c for c in CASES}


def lens_of(case):
    """Real token counts: the first row fills Tin, the others are ragged (padded positions must get zero attention)."""
    T = case.Tin
    pattern = [T, T - 7, max(3, T // 3), T - 1, max(2, T // 2), T - 20, 5, T - 3, 11, T // 4, T - 2]
    return [max(1, min(T, n)) for n in pattern[:case.B]]


def inputs(case):
    """(tokens [B, Tin], speaker [B, 256] or None, prenet masks [B, max_len, 2, 256]).  Every case runs with prenet
    dropout masks: without them the decoder settles and late frames barely change (see the chunk-edge control)."""
    rng = np.random.default_rng(1000 + 7 * case.B + case.Tin + case.seed)
    tok = rng.integers(1, 148, (case.B, case.Tin)).astype(np.int32)
    for b, n in enumerate(lens_of(case)):
        tok[b, n:] = 0
    masks = (rng.random((case.B, case.max_len, 2, 256)) >= 0.5).astype(np.float32) * 2.0
    spk = None
    if case.enc == 768:
        spk = rng.standard_normal((case.B, 256)).astype(np.float32)
        spk /= np.linalg.norm(spk, axis=1, keepdims=True)
    return tok, spk, masks


@functools.lru_cache(maxsize=None)
def config(enc):
    from text_to_speech_amd.config import Tacotron2Config
    return Tacotron2Config() if enc == 512 else Tacotron2Config(speaker_embedding_dim=enc - 512)


@functools.lru_cache(maxsize=None)
def base_weights(enc):
    from text_to_speech_amd import weights
    return weights.synth_tacotron2(config(enc), seed=1234 if enc == 512 else 99)


@functools.lru_cache(maxsize=None)
def scripted(name):
    """(weights, sensitivity, margin) of a scripted-stop case: the base weights with a fitted gate."""
    from stop_script import script_stop_tokens
    case = CASE_BY_NAME[name]
    tok, spk, masks = inputs(case)
    return script_stop_tokens(base_weights(case.enc), config(case.enc), tok, list(case.targets), speaker_embedding=spk,
                              prenet_masks=masks, **case.win_kwargs)


def weights_key(case):
    """Cases sharing a key share the weights (and, on the GPU, one engine)."""
    return case.name if case.early_stopping else f'enc{case.enc}'


def weights_of(case):
    return scripted(case.name)[0] if case.early_stopping else base_weights(case.enc)


@functools.lru_cache(maxsize=None)
def _weights_rounded(key, enc, kind):
    case = next(c for c in CASES if weights_key(c) == key)
    w = weights_of(case)
    return w if kind == 'f32' else round_lstm_f16(w, enc, keep_ctx=kind == 'f16_ctx32')


@functools.lru_cache(maxsize=None)
def _reference(name, kind, zero_speaker=False, max_len=None, windowed=True):
    from oracle import tacotron2_ref
    case = CASE_BY_NAME[name]
    tok, spk, masks = inputs(case)
    if zero_speaker:
        spk = np.zeros_like(spk)
    T = case.max_len if max_len is None else max_len
    return tacotron2_ref.infer(tok, _weights_rounded(weights_key(case), case.enc, kind), config(case.enc),
                               speaker_embedding=spk, max_length=T, early_stopping=case.early_stopping,
                               prenet_masks=masks[:, :T], **(case.win_kwargs if windowed else {}))


def reference(case, kind='f32', zero_speaker=False, max_len=None, windowed=True):
    """Oracle output of `case` with the weights rounded as `kind` says (module docstring); cached per process.
    `windowed=False` drops the case's attention window."""
    return _reference(case.name, kind, zero_speaker, max_len, windowed)


def window_bounds(case, attention):
    """(prev, lo, hi), int [B, steps] each, of a window case, from alignments [B, steps, Tin] (tacotron2_arch.py:630-638):
    `prev` is the arg max of the step before (0 at step 0); the step keeps positions lo <= tau <= hi."""
    win_len, win_off = case.win
    am = np.asarray(attention).argmax(-1)
    prev = np.concatenate([np.zeros((case.B, 1), np.int64), am[:, :-1]], 1)
    enc_len = np.asarray(lens_of(case))[:, None]
    center = np.minimum(np.maximum(prev, win_off), enc_len - win_len + win_off)
    return prev, center - win_off, center - win_off + win_len


def machines(case, precision):
    """[(machine, Variant)] of every machine that accepts the case."""
    out = []
    for m in ('persistent', 'fused', 'graph'):
        v = pick_variant(m, case.B, case.Tin, case.enc, precision)
        if v is not None:
            out.append((m, v))
    return out


def chunk_edges(case, steps):
    """Chunk edges inside the loop, as frame indices e: frame e is the first of a new graph (32) or fused (64) chunk."""
    return [e for e in range(GRAPH_CHUNK, steps, GRAPH_CHUNK)]


def attention_rms_rel(a, r):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64) - r))) / np.sqrt(np.mean(np.square(np.asarray(r, np.float64)))))
