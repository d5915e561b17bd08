// mel_dtw_call.h -- what one MCD / DTW call (tts_hip_mel_dtw, tts_hip_mel_dtw_probe; mel_dtw.hip) is, why it may be refused and
// how its workspace is laid out: pure host code on the caller's arguments (no HIP include; also built with plain g++ under
// ASan / UBSan by csrc/host_check.cpp, --mel-dtw, and compared there with a Python restatement, tests/test_mel_dtw.py).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "taco_call.h"      // taco_refuse, taco_bad_mem

constexpr int kDtwMinMel = 2, kDtwMaxMel = 128;      // channels of a frame
constexpr int kDtwMaxFrames = 8192;                  // Ta and Tb: the sweep keeps one strip edge of a row's frames in LDS (32 KiB)
// B * Ta * Tb.  The aligned programme keeps, per cell, at most 2 distances (float) and 2 step codes (a byte) in the skewed
// layout below: 10 bytes, 320 MiB at this limit (a probe of the cost matrix adds 8 more, and 4 for a host caller's result).
constexpr long long kDtwMaxCells = 1ll << 25;
// B * (Ta + Tb): what the cells do not bound in a thin call (many rows, or one side of a frame or two).  The cepstra are up to
// 128 floats a frame and a host caller's staged mels another 128: at most 256 MiB each at this limit.  So the workspace of an
// accepted call is below 320 + 256 + 256 MiB plus 8 MiB of path, tables and padding (a probe: + 256 + 128 MiB), whatever its shape.
constexpr long long kDtwMaxRowFrames = 1ll << 19;
constexpr int kDtwStages = 5;                        // TTS_HIP_DTW_CEPSTRA_A .. TTS_HIP_DTW_STEP

struct MelDtwCall {
    const char* who;                 // the entry point, as messages name it
    const float *a, *b;              // [B, Ta, n_mel], [B, Tb, n_mel]
    int B, Ta, Tb, n_mel;
    const int32_t *len_a, *len_b;    // host int32 [B] or NULL (every row full)
    int n_cep, flags;                // TTS_HIP_DTW_*
    float* stats;                    // [3, B]                       (the call)
    int32_t* path;                   // NULL or [B, Ta + Tb - 1, 2]  (the call)
    bool probe;                      // tts_hip_mel_dtw_probe: `what` and `out` stand for `stats` and `path`
    int what;                        // the stage the probe returns (the call: -1)
    float* out;                      // the probe's dense result
    int mem;
    void* stream;                    // NULL = the handle's
};

inline bool dtw_probing(const MelDtwCall& c) { return c.probe; }
inline int dtw_coeffs(const MelDtwCall& c) { return c.n_cep + ((c.flags & TTS_HIP_DTW_C0) ? 1 : 0); }

// Every reason a call is refused, first match wins, in this order: a NULL pointer (a, b, then stats | out), B / Ta / Tb below
// 1, n_mel outside 2 .. 128, n_cep outside 1 .. n_mel - 1, unknown flag bits, mem kind, (probe) an unknown stage, a length
// outside its range (len_a first, rows in order), Ta or Tb above kDtwMaxFrames, B * Ta * Tb above kDtwMaxCells, B * (Ta + Tb)
// above kDtwMaxRowFrames.  The kernels
// load single floats: no alignment is asked of device pointers.  Reads host memory only (the two length tables); TTS_HIP_OK
// or TTS_HIP_EINVAL with the reason in `msg`.  Nothing is copied or launched before it has passed.
inline int mel_dtw_check(const MelDtwCall& c, char* msg, size_t n) {
    const struct { const void* p; const char* name; } ptrs[] = {
        {c.a, "a"}, {c.b, "b"}, {dtw_probing(c) ? (const void*)c.out : (const void*)c.stats, dtw_probing(c) ? "out" : "stats"}};
    for (const auto& p : ptrs)
        if (!p.p) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%s is NULL", p.name);
    if (c.B < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B = %d must be at least 1", c.B);
    if (c.Ta < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "Ta = %d must be at least 1", c.Ta);
    if (c.Tb < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "Tb = %d must be at least 1", c.Tb);
    if (c.n_mel < kDtwMinMel || c.n_mel > kDtwMaxMel)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "n_mel = %d is outside [%d, %d]", c.n_mel, kDtwMinMel, kDtwMaxMel);
    if (c.n_cep < 1 || c.n_cep > c.n_mel - 1)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "n_cep = %d is outside [1, n_mel - 1 = %d]", c.n_cep, c.n_mel - 1);
    if (c.flags & ~(TTS_HIP_DTW_ALIGN | TTS_HIP_DTW_C0))
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "flags = %d holds unknown bits (1 align, 2 c0)", c.flags);
    if (taco_bad_mem(c.mem)) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad mem kind %d", c.mem);
    if (c.probe && (c.what < 0 || c.what >= kDtwStages))
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL,
                           "what = %d is no stage (0 cepstra_a, 1 cepstra_b, 2 distance, 3 cost, 4 step)", c.what);
    const struct { const int32_t* p; const char* name; int T; } lens[] = {{c.len_a, "len_a", c.Ta}, {c.len_b, "len_b", c.Tb}};
    for (const auto& l : lens)
        for (int b = 0; l.p && b < c.B; ++b)
            if (l.p[b] < 1 || l.p[b] > l.T)
                return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%s[%d] = %d is outside [1, T%c = %d]", l.name, b, (int)l.p[b],
                                   l.name[4], l.T);
    if (c.Ta > kDtwMaxFrames || c.Tb > kDtwMaxFrames)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "Ta = %d, Tb = %d: above %d frames", c.Ta, c.Tb, kDtwMaxFrames);
    if ((long long)c.B * c.Ta * c.Tb > kDtwMaxCells)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B*Ta*Tb too large (B = %d, Ta = %d, Tb = %d: above %lld cells); split the batch",
                           c.B, c.Ta, c.Tb, kDtwMaxCells);
    if ((long long)c.B * ((long long)c.Ta + c.Tb) > kDtwMaxRowFrames)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B*(Ta+Tb) too large (B = %d, Ta = %d, Tb = %d: above %lld frames); split the batch",
                           c.B, c.Ta, c.Tb, kDtwMaxRowFrames);
    return TTS_HIP_OK;
}

// Where the call's buffers start in the handle's DTW workspace, in bytes (each 256-aligned), and its size.  The matrices of
// the aligned programme are kept skewed (diagonal-major): cell (i, j) of a pair lies at (i + j) * W + (Ta < Tb ? i : j),
// W = min(Ta, Tb), K = Ta + Tb - 1 diagonals -- what the lanes of one sweep step touch is consecutive in memory.
struct MelDtwLayout {
    int R;                           // coefficients per frame: n_cep, + 1 with c0
    int W, K;                        // width and number of the skewed diagonals
    bool skew_i;                     // a diagonal is indexed by i (Ta < Tb), else by j
    bool aligned;                    // the dynamic programme runs (TTS_HIP_DTW_ALIGN, or a probe of its stages)
    size_t in_a, in_b;               // staged inputs of a TTS_HIP_MEM_HOST call (else 0 bytes)
    size_t lens;                     // int32 [2][B]: len_a, len_b
    size_t cep_a, cep_b;             // float [B][Ta][R], [B][Tb][R]
    size_t dist;                     // float [B][K][W]     (aligned)
    size_t step;                     // uint8 [B][K][W]     (aligned)
    size_t cost;                     // float [B][K][W]     (probe of cost only)
    size_t final_cost;               // float [B]           (aligned)
    size_t stats;                    // float [3][B]        (host call)
    size_t path;                     // int32 [B][K][2]     (host call that asks for it)
    size_t out;                      // the probe's dense result (host probe)
    size_t out_elems;                // ... and its floats, whatever `mem` says
    size_t bytes;
};

// (arguments already passed mel_dtw_check)
inline MelDtwLayout mel_dtw_layout(const MelDtwCall& c) {
    MelDtwLayout l{};
    l.R = dtw_coeffs(c);
    l.W = c.Ta < c.Tb ? c.Ta : c.Tb;
    l.K = c.Ta + c.Tb - 1;
    l.skew_i = c.Ta < c.Tb;
    l.aligned = dtw_probing(c) ? c.what >= TTS_HIP_DTW_DISTANCE : (c.flags & TTS_HIP_DTW_ALIGN) != 0;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const bool host = c.mem == TTS_HIP_MEM_HOST;
    const size_t B = (size_t)c.B, skewed = B * l.K * l.W;
    l.in_a = take(host ? B * c.Ta * c.n_mel * sizeof(float) : 0);
    l.in_b = take(host ? B * c.Tb * c.n_mel * sizeof(float) : 0);
    l.lens = take(2 * B * sizeof(int32_t));
    l.cep_a = take(B * c.Ta * l.R * sizeof(float));
    l.cep_b = take(B * c.Tb * l.R * sizeof(float));
    l.dist = take(l.aligned ? skewed * sizeof(float) : 0);
    l.step = take(l.aligned ? skewed : 0);
    l.cost = take(c.probe && c.what == TTS_HIP_DTW_COST ? skewed * sizeof(float) : 0);
    l.final_cost = take(l.aligned ? B * sizeof(float) : 0);
    l.stats = take(host && !dtw_probing(c) ? 3 * B * sizeof(float) : 0);
    l.path = take(host && !dtw_probing(c) && c.path ? B * l.K * 2 * sizeof(int32_t) : 0);
    l.out_elems = !dtw_probing(c)                 ? 0
                  : c.what == TTS_HIP_DTW_CEPSTRA_A ? B * c.Ta * l.R
                  : c.what == TTS_HIP_DTW_CEPSTRA_B ? B * c.Tb * l.R
                                                    : B * c.Ta * c.Tb;
    l.out = take(host ? l.out_elems * sizeof(float) : 0);
    l.bytes = at;
    return l;
}

// The orthonormal DCT-II rows the cepstra use, [R][n_mel]: D[r][k] = sqrt(2 / n_mel) cos(pi (k + 1/2) r / n_mel), row 0 divided
// by sqrt 2; rows 1 .. n_cep, or 0 .. n_cep with c0.  Computed in float64 and rounded once to float32.
inline std::vector<float> mel_dtw_dct(int n_mel, int n_cep, bool c0) {
    const int R = n_cep + (c0 ? 1 : 0), r0 = c0 ? 0 : 1;
    std::vector<float> D((size_t)R * n_mel);
    const double pi = 3.14159265358979323846, scale = std::sqrt(2.0 / n_mel);
    for (int r = 0; r < R; ++r)
        for (int k = 0; k < n_mel; ++k) {
            const double v = scale * std::cos(pi * (k + 0.5) * (r + r0) / n_mel);
            D[(size_t)r * n_mel + k] = (float)(r + r0 == 0 ? v / std::sqrt(2.0) : v);
        }
    return D;
}
