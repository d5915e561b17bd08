// wg_plan.h -- which WN GEMM tile family and which form one WaveGlow call takes: pure host arithmetic on the frame count,
// the precision and the form (no HIP include; also built with plain g++ by csrc/host_check.cpp, and compared there with
// the restatement in tests/waveglow_cases.py::pick_variant).
#pragma once

// fp32: the Winograd form (wn_wino.hip) executes K ~910 per output instead of 1 856 (taps 768 in one kernel per layer on 64-row
// tiles, conditioning 140 in a kernel of its own ahead of it).
// It pays from about 150 frames per call (one sentence, measured on one box, Winograd / direct: 100 frames 16.9 / 15.0 ms,
// 150: 18.3 / 20.9, 200: 19.4 / 26.0, 350: 32.2 / 37.6, 513: 48.5 / 61.2, 800: 64.0 / 84.9; the three-pass form of round 3
// only paid from 384 frames: its two HBM-bound passes and six-slice launches cost 40 % at 100 frames)
#ifndef TTS_WINO_MIN_FRAMES
#define TTS_WINO_MIN_FRAMES 144
#endif

// WN GEMM tile family; the values are the codes of tts_hip_last_waveglow_tiles (include/tts_hip.h)
enum WgTiles { WG_T256 = 0, WG_T128 = 1, WG_T128x64 = 2, WG_ROW64 = 3 };

struct WgPlan {
    int BT;             // frames of the call
    int PR;             // rows per phase block: BT padded to the M tile
    long long M;        // phase-major rows, 32 * PR (incl. padding)
    int NP;             // fp16 planes per operand (2 in split fp16)
    WgTiles tiles;
    bool wino_wanted;   // layers 1 .. 7 in their Winograd form, if the device can hold its operands (the driver asks)
};

// precision 0 fp32, 1 fp16, 2 split fp16; form_mode as tts_hip_set_waveglow_form sets it (only fp32 has forms)
inline WgPlan wg_plan(int BT, int precision, int form_mode) {
    const bool half = precision == 1, x3 = precision == 2;
    // rows per phase block, padded to the M tile: 256-row tiles unless 128-row tiles save at least 5 % of the rows
    const int pr256 = (BT + 255) / 256 * 256, pr128 = (BT + 127) / 128 * 128, pr64 = (BT + 63) / 64 * 64;
    const bool tile128 = pr128 * 1.05 < pr256;
    // short utterances (a sentence at batch 1): 64-row tiles when they save padding
    const int pr_big = tile128 ? pr128 : pr256;
    bool row64 = x3 ? pr64 * 1.25 < pr256      // split fp16 has two tile shapes: 64 x 128 (about 25 % more time per row) and 256 x 256
                    : BT <= 512 &&
                      (half ? pr64 * 4 <= pr_big * 3 : pr64 < pr_big);   // fp16: the smaller tile only pays from -25 % rows
    const bool wino_size = precision == 0 && form_mode >= 1 && BT >= TTS_WINO_MIN_FRAMES;
    // the three-pass form (measurement form 2) needs 128-row phase blocks; the fused kernels run on 64-row tiles
    if (wino_size && form_mode == 2 && row64 && (double)pr128 * 1120.0 * 1.35 < (double)pr64 * 1856.0) row64 = false;
    WgPlan p;
    p.BT = BT;
    p.PR = row64 ? pr64 : (tile128 && !x3) ? pr128 : pr256;      // split fp16 never takes the 128-row family
    p.M = 32ll * p.PR;
    p.NP = x3 ? 2 : 1;
    // 128 x 128 tiles would leave block slots (3 per CU) empty -> 128 x 64 tiles, twice the blocks
    const bool tile64 = !row64 && tile128 && (p.M / 128) * 8 < 768;
    p.tiles = row64 ? WG_ROW64 : x3 ? WG_T256 : tile64 ? WG_T128x64 : tile128 ? WG_T128 : WG_T256;
    p.wino_wanted = wino_size && (!row64 || form_mode != 2);     // form 2 never runs on 64-row blocks (PR: a multiple of 128)
    return p;
}

// First WN layer of a flow in the Winograd form (wn_wino.hip, wino_layer0_kernel): its three taps act on the neighbouring
// POSITIONS n - 1, n, n + 1 (n = 32 t + p), i.e. on the phase blocks p - 1, p, p + 1 of the phase-major layout, carried into
// frame t - 1 / t + 1 at p = 0 / p = 31.  Row of a0p that tap s (-1, 0, +1) of position (phase p, frame row f = b T + t) reads,
// or -1 when that position lies outside the utterance (or f is a padding row >= BT): the bounds test of the direct form's
// SEG_PHASE_TAP segments.  Tail frames of a ragged row and gap frames of a packed row need no test: their a0p rows are zero.
#ifdef __HIPCC__
#define WG_HOST_DEVICE __host__ __device__
#else
#define WG_HOST_DEVICE
#endif
WG_HOST_DEVICE inline long long wn_tap_row(int p, int f, int s, int PR, int BT, int T) {
    if (f >= BT) return -1;
    const int ps = p + s;
    const int carry = ps < 0 ? -1 : ps > 31 ? 1 : 0;
    const int t = f % T + carry;
    if (t < 0 || t >= T) return -1;
    return (long long)(ps - 32 * carry) * PR + f + carry;
}
// Column k of the 16-float tap operand row for a flow with h coupling channels: [tap -1: a[0..h), v | tap 0 | tap +1 | 0 ..]
// (v: a0p's constant-1 column, the indicator that carries the start conv's bias) -> tap index 0 .. 2 and a0p column, or
// tap 3 for the zero columns behind the 3 (h + 1) used ones.
WG_HOST_DEVICE inline int wn_tap_of_col(int k, int h) { return k < 3 * (h + 1) ? k / (h + 1) : 3; }
WG_HOST_DEVICE inline int wn_tap_src_col(int k, int h) { return k % (h + 1); }
