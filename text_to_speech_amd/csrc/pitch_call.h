// pitch_call.h -- what a pitch call (tts_hip_pitch, tts_hip_pitch_probe), a probabilistic-YIN call (tts_hip_pyin,
// tts_hip_pyin_probe) and an F0 comparison (tts_hip_f0_error; pitch.hip) are, why they may be refused and how their workspaces
// are laid out: pure host code on the caller's arguments (no HIP include; also built with plain g++ under ASan / UBSan by
// csrc/host_check.cpp, --pitch and --pyin, and compared there with a Python restatement, tests/test_pitch.py and
// tests/test_pyin.py).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstddef>

#include "mel_dtw_call.h"   // kDtwMaxFrames, kDtwMaxRowFrames: an F0 comparison takes the frames and the path a mel_dtw call can return
#include "taco_call.h"      // taco_refuse, taco_bad_mem

constexpr int kPitchMinWin = 2, kPitchMaxWin = 2048;      // W: samples a difference sums
constexpr int kPitchMaxLag = 1024;                        // tau_max: W + tau_max samples of a frame lie in LDS, 12 KiB here
constexpr int kPitchMaxSamples = 1 << 24;                 // N: a sample index and a frame count stay exact in float32 and far from int32
constexpr long long kPitchMaxBytes = 1ll << 31;           // every buffer of a call stays below this many bytes
constexpr int kPitchStages = 3;                           // TTS_HIP_PITCH_DIFF .. TTS_HIP_PITCH_PICK
constexpr int kPitchLagsPerThread = 4;                    // a thread of the kernel owns four consecutive lags

struct PitchCall {
    const char* who;                 // the entry point, as messages name it
    const float* audio;              // [B, N]
    int B, N;
    const int32_t* lengths;          // host int32 [B] or NULL (every row full)
    int rate, hop, win, tau_min, tau_max;
    float threshold;
    bool probe;                      // tts_hip_pitch_probe
    int what;                        // the stage the probe returns (the call: -1)
    float* out;                      // [3, B, F], or the probe's dense result
    int mem;
    void* stream;                    // NULL = the handle's
};

inline int pitch_frames(int n, int hop) { return 1 + n / hop; }

// the floats of `out`: [3, B, F]; a probe: [B, F, tau_max + 1] for the difference and its normalised form, [2, B, F] for the pick
inline long long pitch_out_elems(const PitchCall& c) {
    const long long BF = (long long)c.B * pitch_frames(c.N, c.hop);
    return !c.probe ? 3 * BF : c.what == TTS_HIP_PITCH_PICK ? 2 * BF : BF * (c.tau_max + 1);
}

// Every reason a call is refused, first match wins, in this order: a NULL audio or out, B or N below 1, rate below 1, hop
// outside 1 .. win, win outside 2 .. 2048, tau_min below 1 or not below tau_max or tau_max above 1024, a threshold outside
// (0, 1] (a NaN is), mem kind, (probe) an unknown stage, a length outside 1 .. N (rows in order), N above 2^24, a buffer of the
// call (audio, out -- the probe's [B, F, tau_max + 1] floats included) at or above 2^31 bytes.  The kernel loads single
// floats: no alignment is asked of device pointers.  Reads host memory only (the length table); TTS_HIP_OK or TTS_HIP_EINVAL
// with the reason in `msg`.  Nothing is copied or launched before it has passed.
inline int pitch_check(const PitchCall& c, char* msg, size_t n) {
    if (!c.audio) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "audio is NULL");
    if (!c.out) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "out is NULL");
    if (c.B < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B = %d must be at least 1", c.B);
    if (c.N < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "N = %d must be at least 1", c.N);
    if (c.rate < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "rate = %d must be at least 1", c.rate);
    if (c.hop < 1 || c.hop > c.win) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "hop = %d is outside [1, win = %d]", c.hop, c.win);
    if (c.win < kPitchMinWin || c.win > kPitchMaxWin)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "win = %d is outside [%d, %d]", c.win, kPitchMinWin, kPitchMaxWin);
    if (c.tau_min < 1 || c.tau_min >= c.tau_max || c.tau_max > kPitchMaxLag)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "lags [%d, %d] must satisfy 1 <= tau_min < tau_max <= %d", c.tau_min, c.tau_max,
                           kPitchMaxLag);
    if (!(c.threshold > 0.f && c.threshold <= 1.f))
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "threshold = %g is outside (0, 1]", (double)c.threshold);
    if (taco_bad_mem(c.mem)) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad mem kind %d", c.mem);
    if (c.probe && (c.what < 0 || c.what >= kPitchStages))
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "what = %d is no stage (0 difference, 1 normalised difference, 2 pick)", c.what);
    for (int b = 0; c.lengths && b < c.B; ++b)
        if (c.lengths[b] < 1 || c.lengths[b] > c.N)
            return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "lengths[%d] = %d is outside [1, N = %d]", b, (int)c.lengths[b], c.N);
    if (c.N > kPitchMaxSamples) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "N = %d: above %d samples", c.N, kPitchMaxSamples);
    if ((long long)c.B * c.N * (long long)sizeof(float) >= kPitchMaxBytes)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "audio too large (B = %d, N = %d: 2^31 bytes or more); split the batch", c.B, c.N);
    if (pitch_out_elems(c) * (long long)sizeof(float) >= kPitchMaxBytes)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "out too large (%lld floats: 2^31 bytes or more); split the batch", pitch_out_elems(c));
    return TTS_HIP_OK;
}

// Where the call's buffers start in the handle's pitch workspace, in bytes (each 256-aligned), its size, and the launch
struct PitchLayout {
    int F;                           // frames of a full row
    int threads;                     // of a workgroup: four lags each, whole waves
    size_t lens;                     // int32 [B]
    size_t in;                       // staged audio of a TTS_HIP_MEM_HOST call (else 0 bytes)
    size_t out;                      // staged result of a TTS_HIP_MEM_HOST call (else 0 bytes)
    size_t out_elems;
    size_t bytes;
};

// (arguments already passed pitch_check)
inline PitchLayout pitch_layout(const PitchCall& c) {
    PitchLayout l{};
    l.F = pitch_frames(c.N, c.hop);
    const int owners = (c.tau_max + 1 + kPitchLagsPerThread - 1) / kPitchLagsPerThread;      // lags 0 .. tau_max
    l.threads = (owners + 63) / 64 * 64;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const bool host = c.mem == TTS_HIP_MEM_HOST;
    l.out_elems = (size_t)pitch_out_elems(c);
    l.lens = take((size_t)c.B * sizeof(int32_t));
    l.in = take(host ? (size_t)c.B * c.N * sizeof(float) : 0);
    l.out = take(host ? l.out_elems * sizeof(float) : 0);
    l.bytes = at;
    return l;
}

// ---- probabilistic YIN (tts_hip_pyin, tts_hip_pyin_probe)
constexpr int kPyinMaxBins = 1024;                        // n_bins: a thread of the decode owns a bin, a workgroup a row
constexpr int kPyinMaxBps = 100;                          // bins per semitone
constexpr int kPyinMaxThresh = 1024;                      // n_thresh: the cumulative prior lies in LDS
constexpr int kPyinStages = 5;                            // TTS_HIP_PYIN_TROUGH .. TTS_HIP_PYIN_PATH

struct PyinCall {
    PitchCall p;                     // who, audio, B, N, lengths, rate, hop, win, tau_min, tau_max, out, mem, stream (threshold, probe
                                     // and what of a plain call: pitch_check sees nothing of the new arguments)
    const float* prior;              // host float [n_thresh]
    int n_thresh;
    float no_trough_prob;
    double fmin;
    int bps, n_bins, max_step;
    float switch_prob;
    bool probe;                      // tts_hip_pyin_probe
    int what;                        // the stage the probe returns (the call: -1)
};

// the floats of `out`: [3, B, F]; a probe: TROUGH [B, F, tau_max + 1], OBS [2, B, F, n_bins], DELTA and BACK [B, F, 2 n_bins],
// PATH [B, F]
inline long long pyin_out_elems(const PyinCall& c) {
    const long long BF = (long long)c.p.B * pitch_frames(c.p.N, c.p.hop);
    if (!c.probe) return 3 * BF;
    switch (c.what) {
        case TTS_HIP_PYIN_TROUGH: return BF * (c.p.tau_max + 1);
        case TTS_HIP_PYIN_PATH: return BF;
        default: return BF * 2 * c.n_bins;
    }
}

// Every reason a pYIN call is refused, first match wins: everything pitch_check refuses, in its order (the call seen as a plain
// pitch call with a threshold of 1/2); then n_bins outside 1 .. 1024, bps outside 1 .. 100, max_step outside 1 .. n_bins, n_thresh
// outside 1 .. 1024, a NULL prior, a prior entry that is not finite or is negative (entries in order), switch_prob outside (0, 1),
// no_trough_prob outside [0, 1], an fmin that is not finite and positive (a NaN fails each of the three), (probe) an unknown
// stage, a buffer of the call -- out, the probe's result included; the observations [B, F, n_bins] floats; the backpointers
// [B, F, 2 n_bins] uint16 -- at or above 2^31 bytes.  Reads host memory only (the length table, the prior).
inline int pyin_check(const PyinCall& c, char* msg, size_t n) {
    if (const int rc = pitch_check(c.p, msg, n)) return rc;
    const char* who = c.p.who;
    if (c.n_bins < 1 || c.n_bins > kPyinMaxBins)
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "n_bins = %d is outside [1, %d]", c.n_bins, kPyinMaxBins);
    if (c.bps < 1 || c.bps > kPyinMaxBps)
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "bins_per_semitone = %d is outside [1, %d]", c.bps, kPyinMaxBps);
    if (c.max_step < 1 || c.max_step > c.n_bins)
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "max_step = %d is outside [1, n_bins = %d]", c.max_step, c.n_bins);
    if (c.n_thresh < 1 || c.n_thresh > kPyinMaxThresh)
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "n_thresh = %d is outside [1, %d]", c.n_thresh, kPyinMaxThresh);
    if (!c.prior) return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "prior is NULL");
    for (int i = 0; i < c.n_thresh; ++i)
        if (!(std::isfinite(c.prior[i]) && c.prior[i] >= 0.f))
            return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "prior[%d] = %g must be finite and not negative", i, (double)c.prior[i]);
    if (!(c.switch_prob > 0.f && c.switch_prob < 1.f))
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "switch_prob = %g is outside (0, 1)", (double)c.switch_prob);
    if (!(c.no_trough_prob >= 0.f && c.no_trough_prob <= 1.f))
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "no_trough_prob = %g is outside [0, 1]", (double)c.no_trough_prob);
    if (!(std::isfinite(c.fmin) && c.fmin > 0.0)) return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "fmin = %g must be finite and positive", c.fmin);
    if (c.probe && (c.what < 0 || c.what >= kPyinStages))
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "what = %d is no stage (0 trough, 1 observation, 2 delta, 3 back, 4 path)", c.what);
    const long long BF = (long long)c.p.B * pitch_frames(c.p.N, c.p.hop);
    if (pyin_out_elems(c) * (long long)sizeof(float) >= kPitchMaxBytes)
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "out too large (%lld floats: 2^31 bytes or more); split the batch", pyin_out_elems(c));
    if (BF * c.n_bins * (long long)sizeof(float) >= kPitchMaxBytes)
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "observations too large (%lld floats: 2^31 bytes or more); split the batch", BF * c.n_bins);
    if (BF * 2 * c.n_bins * (long long)sizeof(uint16_t) >= kPitchMaxBytes)
        return taco_refuse(msg, n, who, TTS_HIP_EINVAL, "backpointers too large (%lld states: 2^31 bytes or more); split the batch",
                           BF * 2 * c.n_bins);
    return TTS_HIP_OK;
}

// Where a pYIN call's buffers start in the handle's pitch workspace, in bytes (each 256-aligned), its size, and the launches
struct PyinLayout {
    int F;                           // frames of a full row
    int threads;                     // of a workgroup of the observation kernel: four lags each, whole waves
    int vit_threads;                 // of a workgroup of the decode: a bin each, whole waves
    size_t lens;                     // int32 [B]
    size_t in;                       // staged audio of a TTS_HIP_MEM_HOST call (else 0 bytes)
    size_t out;                      // staged result of a TTS_HIP_MEM_HOST call (else 0 bytes)
    size_t cum;                      // float [n_thresh + 1]: the cumulative prior
    size_t tables;                   // float [max_step + 1 + n_bins + 2]: log triangle, log norm, log(1 - switch), log switch
    size_t obs, cand;                // float [B, F, n_bins] each
    size_t vprob;                    // float [B, F]
    size_t back;                     // uint16 [B, F, 2 n_bins]
    size_t path;                     // int32 [B, F]
    size_t out_elems;
    size_t bytes;
};

// (arguments already passed pyin_check)
inline PyinLayout pyin_layout(const PyinCall& c) {
    PyinLayout l{};
    l.F = pitch_frames(c.p.N, c.p.hop);
    const int owners = (c.p.tau_max + 1 + kPitchLagsPerThread - 1) / kPitchLagsPerThread;
    l.threads = (owners + 63) / 64 * 64;
    l.vit_threads = (c.n_bins + 63) / 64 * 64;
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const bool host = c.p.mem == TTS_HIP_MEM_HOST;
    const size_t BF = (size_t)c.p.B * l.F;
    l.out_elems = (size_t)pyin_out_elems(c);
    l.lens = take((size_t)c.p.B * sizeof(int32_t));
    l.in = take(host ? (size_t)c.p.B * c.p.N * sizeof(float) : 0);
    l.out = take(host ? l.out_elems * sizeof(float) : 0);
    l.cum = take((size_t)(c.n_thresh + 1) * sizeof(float));
    l.tables = take((size_t)(c.max_step + 1 + c.n_bins + 2) * sizeof(float));
    l.obs = take(BF * c.n_bins * sizeof(float));
    l.cand = take(BF * c.n_bins * sizeof(float));
    l.vprob = take(BF * sizeof(float));
    l.back = take(BF * 2 * c.n_bins * sizeof(uint16_t));
    l.path = take(BF * sizeof(int32_t));
    l.bytes = at;
    return l;
}

// The host tables of a call, in double, rounded once: cum[k] = prior[0] + ... + prior[k - 1]; then log(max_step + 1 - k),
// k = 0 .. max_step; log norm(i), norm(i) = the sum of the triangle over the bins j of [0, n_bins) within max_step of i; log(1 -
// switch_prob); log(switch_prob).
inline void pyin_tables(const PyinCall& c, float* cum, float* tables) {
    double run = 0.0;
    cum[0] = 0.f;
    for (int k = 0; k < c.n_thresh; ++k) cum[k + 1] = (float)(run += (double)c.prior[k]);
    for (int k = 0; k <= c.max_step; ++k) tables[k] = (float)std::log((double)(c.max_step + 1 - k));
    float* norm = tables + c.max_step + 1;
    for (int i = 0; i < c.n_bins; ++i) {
        const int lo = i - c.max_step < 0 ? 0 : i - c.max_step, hi = i + c.max_step > c.n_bins - 1 ? c.n_bins - 1 : i + c.max_step;
        long long s = 0;
        for (int j = lo; j <= hi; ++j) s += c.max_step + 1 - (j < i ? i - j : j - i);
        norm[i] = (float)std::log((double)s);
    }
    norm[c.n_bins] = (float)std::log(1.0 - (double)c.switch_prob);
    norm[c.n_bins + 1] = (float)std::log((double)c.switch_prob);
}

constexpr int kF0Stats = 6;        // pairs, voiced_pairs, rmse_cents, mean_cents, vuv_errors, gross_errors

struct F0ErrorCall {
    const char* who;
    const float *f0_a, *f0_b;        // [B, Fa], [B, Fb]
    int B, Fa, Fb;
    const int32_t *len_a, *len_b;    // host int32 [B] or NULL (every row full)
    const int32_t* path;             // NULL (the diagonal) or int32 [B, P, 2], where `mem` says
    int P;
    float gross_cents;
    float* stats;                    // [6, B]
    int mem;
    void* stream;
};

// Every reason an F0 comparison is refused, first match wins, in this order: a NULL f0_a, f0_b or stats; B, Fa or Fb below 1;
// with a path, P below 1; a gross_cents that is not finite and positive; mem kind; a length outside its range (len_a first, rows
// in order); Fa or Fb above kDtwMaxFrames; with a path, P above Fa + Fb (a warping path has at most Fa + Fb - 1 pairs); B * (Fa +
// Fb) above kDtwMaxRowFrames.  Reads host memory only (the two length tables).
inline int f0_error_check(const F0ErrorCall& c, char* msg, size_t n) {
    const struct { const void* p; const char* name; } ptrs[] = {{c.f0_a, "f0_a"}, {c.f0_b, "f0_b"}, {c.stats, "stats"}};
    for (const auto& p : ptrs)
        if (!p.p) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%s is NULL", p.name);
    if (c.B < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B = %d must be at least 1", c.B);
    if (c.Fa < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "Fa = %d must be at least 1", c.Fa);
    if (c.Fb < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "Fb = %d must be at least 1", c.Fb);
    if (c.path && c.P < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "P = %d must be at least 1", c.P);
    if (!(std::isfinite(c.gross_cents) && c.gross_cents > 0.f))
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "gross_cents = %g must be finite and positive", (double)c.gross_cents);
    if (taco_bad_mem(c.mem)) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad mem kind %d", c.mem);
    const struct { const int32_t* p; const char* name; int T; } lens[] = {{c.len_a, "len_a", c.Fa}, {c.len_b, "len_b", c.Fb}};
    for (const auto& l : lens)
        for (int b = 0; l.p && b < c.B; ++b)
            if (l.p[b] < 1 || l.p[b] > l.T)
                return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%s[%d] = %d is outside [1, F%c = %d]", l.name, b, (int)l.p[b], l.name[4], l.T);
    if (c.Fa > kDtwMaxFrames || c.Fb > kDtwMaxFrames)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "Fa = %d, Fb = %d: above %d frames", c.Fa, c.Fb, kDtwMaxFrames);
    if (c.path && c.P > c.Fa + c.Fb)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "P = %d: above Fa + Fb = %d pairs", c.P, c.Fa + c.Fb);
    if ((long long)c.B * ((long long)c.Fa + c.Fb) > kDtwMaxRowFrames)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B*(Fa+Fb) too large (B = %d, Fa = %d, Fb = %d: above %lld frames); split the batch",
                           c.B, c.Fa, c.Fb, kDtwMaxRowFrames);
    return TTS_HIP_OK;
}

struct F0ErrorLayout {
    size_t lens;                     // int32 [2][B]
    size_t in_a, in_b, path;         // staged operands of a TTS_HIP_MEM_HOST call (else 0 bytes)
    size_t stats;                    // float [6][B] (host call)
    size_t bytes;
};

// (arguments already passed f0_error_check)
inline F0ErrorLayout f0_error_layout(const F0ErrorCall& c) {
    F0ErrorLayout l{};
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const bool host = c.mem == TTS_HIP_MEM_HOST;
    const size_t B = (size_t)c.B;
    l.lens = take(2 * B * sizeof(int32_t));
    l.in_a = take(host ? B * c.Fa * sizeof(float) : 0);
    l.in_b = take(host ? B * c.Fb * sizeof(float) : 0);
    l.path = take(host && c.path ? B * c.P * 2 * sizeof(int32_t) : 0);
    l.stats = take(host ? kF0Stats * B * sizeof(float) : 0);
    l.bytes = at;
    return l;
}
