"""Shared case table of the encoder / postnet convolution tests (tests/test_conv_paths.py on the CPU, _gpu.py on an MI355X).

Every k = 5 conv + folded batch-norm of Tacotron2 -- encoder convs 1-3 and postnet convs 1-5 -- goes through `conv_gemm`
(csrc/tacotron2.hip), which runs it one of two ways:
- 'split': `gemm_small` with blockIdx.z = tap into a scratch buffer [5][M][cout], then `conv_reduce_kernel` adds the
  slices, the bias, the row mask (0 or BN(0)) and the activation;
- 'single': one `gemm_small` over five shifted segments; bias, row mask and activation run in the GEMM epilogue.
`pick_conv_path` restates the rule, so a test can say which path a call must take and that the table reaches both paths
of every conv at the row counts where the rule switches.

References are float64 restatements built from oracle/tacotron2_ref.py (`masked_conv_bn`, `encoder`, `memory @
memory_layer`, the postnet loop), computed once per case.  Errors are max abs over the compared rows divided by the
reference's max abs over the same rows (`stage_error`); padded rows of the convs whose masked rows the engine stores as 0
(encoder convs, postnet convs 1-4) are compared on valid rows only and must be exactly 0 on the GPU.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

# ---- bounds ------------------------------------------------------------------------------------------------------------
MEL_TOL = 1e-3              # north star (BASELINE.json)
# Regression bounds: about 10x the worst error measured on an MI355X over every case of test_conv_paths_gpu.py, as
# stage_error (max abs error / max abs of the reference over the compared rows), fp32 throughout.  The errors grow with
# the layer (each conv carries the rounding of the ones before it) and not with the path: split and single pass measure
# alike.
BOUNDS = {
    'enc_conv': 2.5e-5,         # encoder convs 1-3 (relu), valid rows: measured 2.29e-6 (b37_t109, conv 1); a single-pass
                                # batch's rows against their one-row split calls 2.51e-6 (b37_t109 row 4, conv 1)
    'memory': 3e-5,             # BiLSTM output + speaker columns, every row: measured 2.81e-6 (b37_t109)
    'processed_memory': 1.5e-5, # measured 1.58e-6 (cfg4_e768_b32_t256)
    'post_conv': 6e-5,          # postnet convs 1-4 (tanh), valid rows: measured 5.73e-6 (b16_t1020, conv 4)
    'post_residual': 3e-5,      # postnet conv 5 (no activation, masked rows BN(0)), every row: measured 2.28e-6 (b19_t859);
                                # mel - decoder_output of a real call 2.75e-6 (config 3, 8 x 800, fp16 decoder weights)
    'mel': 1.2e-5,              # frames + residual, every row: measured 1.16e-6 (b19_t859)
}

# ---- the dispatch rule -------------------------------------------------------------------------------------------------
TILE_M, TILE_N = 64, 64     # gemm_small = launch_gemm<2, 2, 1, 1, 32, ...>: BM = WR * RT * 32, BN = WC * CT * 32 (gemm_f32.h)
SPLIT_BELOW_TILES = 512     # conv_gemm: `tiles < 512` -> split
SCRATCH_ROWS = 32768        # taco_decode.h conv_scratch_floats: 5 * min(rows, 32768) * 512 floats


def pick_conv_path(M, cout):
    """'split' or 'single', as conv_gemm (csrc/tacotron2.hip) decides for M rows and `cout` output channels:
    tiles = ceil(M / 64) * ceil(cout / 64); split when tiles < 512, the per-tap scratch 5 * M * cout fits the workspace's
    5 * min(M, 32768) * 512 floats (the encoder and decode size it so; it never binds: a split conv has at most 16320 rows)
    and cout % 4 == 0 (the reduction pass is vectorised by 4)."""
    tiles = -(-M // TILE_M) * -(-cout // TILE_N)
    scratch = 5 * min(M, SCRATCH_ROWS) * 512
    return 'split' if tiles < SPLIT_BELOW_TILES and 5 * M * cout <= scratch and cout % 4 == 0 else 'single'


# (cout, activation, masked rows stored as) per conv of each stage; bit of tts_hip_last_conv_paths = offset + index
LAYERS = {
    'encoder': [(512, 'relu', 'zero')] * 3,
    'postnet': [(512, 'tanh', 'zero')] * 4 + [(80, None, 'bn0')],
}
BIT0 = {'encoder': 0, 'postnet': 3}


def expected_paths(stage, M, upto=None):
    """(bits, mask) of tts_hip_last_conv_paths after `stage` ran convs 0 .. upto (default: all) on M rows."""
    layers = LAYERS[stage]
    n = len(layers) if upto is None else upto + 1
    bits = mask = 0
    for i in range(n):
        b = 1 << (BIT0[stage] + i)
        mask |= b
        if pick_conv_path(M, layers[i][0]) == 'single':
            bits |= b
    return bits, mask


def path_names(stage, M):
    return [pick_conv_path(M, c) for c, _, _ in LAYERS[stage]]


# ---- cases -------------------------------------------------------------------------------------------------------------
class EncCase(NamedTuple):
    name: str
    B: int
    Tin: int
    enc: int = 512
    lens: Optional[tuple] = None        # real tokens per row; None: `_ragged`
    mid_pad: Optional[tuple] = None     # (row, position) of a pad token inside the row's real tokens
    seed: int = 0

    @property
    def rows(self):
        return self.B * self.Tin


class PostCase(NamedTuple):
    name: str
    B: int
    T: int
    seed: int = 0

    @property
    def rows(self):
        return self.B * self.T


def _ragged(B, T, seed):
    """Row lengths that put sequence ends everywhere: full, T - 1, T - 2, 1, the middle, then random."""
    rng = np.random.default_rng(seed)
    head = [T, max(1, T - 1), max(1, T - 2), 1, max(1, T // 2)]
    out = head[:B] + [int(v) for v in rng.integers(1, T + 1, max(0, B - len(head)))]
    return tuple(out)


_E = EncCase
ENCODER_CASES = (
    # split path: one row of one token; three rows of 2 - 5 tokens (every tap of a row crosses its ends);
    # 4032 rows (63 row tiles x 8 column tiles = 504 tiles, the last split row count)
    _E('b1_t1', 1, 1),
    _E('b3_t2', 3, 2), _E('b3_t3', 3, 3), _E('b3_t4', 3, 4), _E('b3_t5', 3, 5, lens=(5, 2, 4), mid_pad=(0, 2)),
    _E('b16_t252', 16, 252, mid_pad=(4, 60)),
    # single pass: 4033 rows (the last row tile holds one row), 4096 rows
    _E('b37_t109', 37, 109, mid_pad=(4, 27)), _E('b16_t256', 16, 256),
    # the encode limits: Tin 4096 (4096 BiLSTM steps) and B 1024 (16 sequences per row tile)
    _E('b1_t4096', 1, 4096, lens=(4000,)), _E('b1024_t4', 1024, 4),
    # the BASELINE config-4 job: 32 utterances, 256-d speaker embeddings (enc 768), 50 - 200 real tokens padded to 256
    _E('cfg4_e768_b32_t256', 32, 256, enc=768, lens=tuple(int(v) for v in np.linspace(50, 200, 32).round())),
)

_P = PostCase
POSTNET_CASES = (
    _P('b16_t252', 16, 252), _P('b37_t109', 37, 109),         # 4032 / 4033 rows: convs 1-4 switch
    _P('b1024_t4', 1024, 4), _P('b800_t7', 800, 7),           # single pass with a sequence end every 4 / 7 rows
    _P('b8_t800', 8, 800), _P('b32_t400', 32, 400),           # BASELINE config 3 and the config-4 job
    _P('b16_t1020', 16, 1020), _P('b19_t859', 19, 859),       # 16320 / 16321 rows: conv 5 (80 channels) switches
)
ENC_BY_NAME = {c.name: c for c in ENCODER_CASES}
POST_BY_NAME = {c.name: c for c in POSTNET_CASES}


def enc_lens(case):
    return case.lens if case.lens is not None else _ragged(case.B, case.Tin, case.seed + 11)


def post_lengths(case):
    """Decoder lengths of the rows; the mask is t <= lengths[b]: 0 (one valid frame), the middle, T - 2, T - 1 and beyond
    (every frame valid), then random in [0, T + 2]."""
    T = case.T
    head = [0, T // 2, max(0, T - 2), T - 1, T + 3, T]
    rng = np.random.default_rng(case.seed + 23)
    return np.array(head[:case.B] + [int(v) for v in rng.integers(0, T + 3, max(0, case.B - len(head)))], np.int32)


def enc_inputs(case):
    """(tokens [B, Tin], speaker [B, 256] or None)."""
    rng = np.random.default_rng(500 + case.B + 3 * case.Tin + case.seed)
    tok = rng.integers(1, 148, (case.B, case.Tin)).astype(np.int32)
    for b, n in enumerate(enc_lens(case)):
        tok[b, n:] = 0
    if case.mid_pad is not None:
        b, t = case.mid_pad
        assert 0 < t < enc_lens(case)[b] - 1, case
        tok[b, t] = 0
    spk = None
    if case.enc == 768:
        spk = rng.standard_normal((case.B, 256)).astype(np.float32)
        spk /= np.linalg.norm(spk, axis=1, keepdims=True)
    return tok, spk


def post_inputs(case):
    """(frames [B, T, 80], lengths [B]): frames ~ N(0, 1), the scale of the synthetic decoder's output."""
    rng = np.random.default_rng(700 + case.B + 3 * case.T + case.seed)
    return rng.standard_normal((case.B, case.T, 80)).astype(np.float32), post_lengths(case)


def post_mask(lengths, T):
    return np.arange(T)[None, :] <= np.asarray(lengths)[:, None]       # dec_mask_kernel / tacotron2_ref.decode


# ---- references --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def config(enc):
    from text_to_speech_amd.config import Tacotron2Config
    return Tacotron2Config() if enc == 512 else Tacotron2Config(speaker_embedding_dim=enc - 512)


@functools.lru_cache(maxsize=None)
def weights(enc):
    """The weights of the engines: conftest's taco_weights for enc 512, the config-4 job's seed for enc 768."""
    from text_to_speech_amd import weights as W
    return W.synth_tacotron2(config(enc), seed=1234)


@functools.lru_cache(maxsize=None)
def weights64(enc):
    return {k: v.astype(np.float64) for k, v in weights(enc).items() if k.startswith('tacotron2/')}


def encoder_convs64(tok, w, cfg):
    """[conv 1, conv 2, conv 3] outputs of the encoder in float64 (padded rows: act(BN(0)), as the reference has them)."""
    from oracle import tacotron2_ref as R
    p = 'tacotron2/encoder'
    mask = tok != cfg.pad_token
    x = w[f'{p}/embeddings'][tok]
    outs = []
    for i in range(cfg.encoder_n_conv):
        x = R.masked_conv_bn(x, mask, w, f'{p}/conv_{i + 1}', f'{p}/norm_{i + 1}', cfg.bn_epsilon, 'relu')
        outs.append(x)
    return outs


def postnet_convs64(frames, mask, w, cfg, kernel_map=None):
    """[conv 1 .. conv 5] outputs of the postnet in float64 (tacotron2_ref.postnet, every layer kept).  `kernel_map`
    (controls only) replaces each conv's kernel."""
    from oracle import tacotron2_ref as R
    x = np.asarray(frames, np.float64)
    n = cfg.postnet_n_conv
    outs = []
    for i in range(n):
        conv = f'tacotron2/postnet/conv_{i + 1}'
        wi = w if kernel_map is None else {**w, f'{conv}/kernel': kernel_map(w[f'{conv}/kernel'])}
        x = R.masked_conv_bn(x, mask, wi, conv, f'tacotron2/postnet/norm_{i + 1}', cfg.bn_epsilon,
                             'tanh' if i < n - 1 else None)
        outs.append(x)
    return outs


@functools.lru_cache(maxsize=None)
def encoder_reference(name):
    """{'mask', 'conv1'..'conv3', 'memory', 'processed_memory'} of an encoder case, float64."""
    from oracle import tacotron2_ref as R
    case = ENC_BY_NAME[name]
    tok, spk = enc_inputs(case)
    w, cfg = weights64(case.enc), config(case.enc)
    convs = encoder_convs64(tok, w, cfg)
    memory, mask = R.encoder(tok, w, cfg, None if spk is None else spk.astype(np.float64))
    pm = memory @ w['tacotron2/decoder/lsa/memory_layer/kernel']
    out = {'mask': mask, 'memory': memory, 'processed_memory': pm}
    out.update({f'conv{i + 1}': c for i, c in enumerate(convs)})
    return out


@functools.lru_cache(maxsize=None)
def postnet_reference(name):
    """{'mask', 'conv1'..'conv5', 'mel'} of a postnet case, float64."""
    case = POST_BY_NAME[name]
    frames, lengths = post_inputs(case)
    return postnet_of(frames, lengths, 512)


def postnet_of(frames, lengths, enc):
    mask = post_mask(lengths, frames.shape[1])
    convs = postnet_convs64(frames, mask, weights64(enc), config(enc))
    out = {'mask': mask, 'mel': np.asarray(frames, np.float64) + convs[-1]}
    out.update({f'conv{i + 1}': c for i, c in enumerate(convs)})
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------
ENC_STAGES = ('conv1', 'conv2', 'conv3', 'memory', 'processed_memory')
POST_STAGES = ('conv1', 'conv2', 'conv3', 'conv4', 'conv5', 'mel')


def bound_of(stage, what):
    if stage == 'encoder':
        return BOUNDS['enc_conv' if what.startswith('conv') else what]
    return BOUNDS['post_conv' if what in ('conv1', 'conv2', 'conv3', 'conv4') else
                  'post_residual' if what == 'conv5' else 'mel']


def valid_only(stage, what):
    """Outputs whose masked rows the engine stores as 0 (compared on valid rows; their padded rows must be exactly 0)."""
    return what.startswith('conv') and not (stage == 'postnet' and what == 'conv5')


def stage_error(got, ref, rows=None):
    """max |got - ref| / max |ref| over `rows` (a [B, T] bool mask; None = every row)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return float(np.abs(got - ref).max()) / scale if scale > 0 else float(np.abs(got - ref).max()) if got.size else 0.0
