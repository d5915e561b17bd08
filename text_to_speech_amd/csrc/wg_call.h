// wg_call.h -- what one WaveGlow call is, why it may be refused and the int table it stages: pure host code on the caller's
// arguments (no HIP include; also built with plain g++ under ASan / UBSan by csrc/host_check.cpp, --wg-call, and compared
// there with tests/waveglow_packed_ref.py::packing_plan and a numpy restatement, tests/test_wg_call.py).  Every
// tts_hip_waveglow_infer* entry point fills a WgCall and hands it to waveglow_call (engine.hip); the inverse direction's test
// hooks fill a WgCall and a WgProbe (wg_probe_check; --wg-call with flow= / what= / layer=); the forward flow's two entry
// points fill a WgEncode (--wg-encode, tests/test_waveglow_encode.py).
#pragma once
#include <stdint.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../include/tts_hip.h"

constexpr int kMaxFramesPerRun = 31744;             // one waveglow_run addresses its activations with 31-bit byte offsets
constexpr long long kMaxGroups = 1ll << 30;         // B * T * 32 groups of 8 samples: what the batch buffers are indexed with

enum WgNoise {
    WG_NOISE_Z = 0,      // the caller's z (NULL: zeros, the reference's deterministic = True)
    WG_NOISE_SEED = 1,   // drawn into wg.io_zgen from one stream (seed, offset), batch layout
    WG_NOISE_ROWS = 2    // drawn into wg.io_zgen from one stream (keys[b], offsets[b]) per row, a row's real frames only
};

struct WgCall {
    const char* who;                 // the entry point, as messages name it
    const float* mel;                // [B, T, 80]
    int B, T;
    const int32_t* lengths;          // NULL or host int32 [B]
    bool packed;                     // one packed row instead of runs of whole rows (needs lengths)
    WgNoise noise;
    const float* z;                  // WG_NOISE_Z
    uint64_t seed, offset;           // WG_NOISE_SEED
    const uint64_t *keys, *offsets;  // WG_NOISE_ROWS: host uint64 [B]
    float sigma;
    float* audio;                    // [B, T * 256]
    int precision;                   // 0 f32, 1 f16, 2 f16x3
    bool async;                      // false: `mem` says where mel / z / audio live, runs on the handle's stream, returns drained
    int mem;                         // true: device pointers, enqueued on `stream` (NULL = the handle's), returns at once
    void* stream;
};

// Frames of the packed row: the rows that hold frames one after another, TTS_HIP_WG_GAP_FRAMES gap frames between two of
// them; rows of length 0 take no space and no gap.  (lengths already checked.)
inline long long wg_packed_frames(int B, const int32_t* lengths, int* rows_out) {
    long long F = 0;
    int rows = 0;
    for (int b = 0; b < B; ++b)
        if (lengths[b] > 0) {
            F += lengths[b];
            ++rows;
        }
    *rows_out = rows;
    return F + (rows > 1 ? (long long)TTS_HIP_WG_GAP_FRAMES * (rows - 1) : 0);
}

inline int wg_refuse(char* msg, size_t n, const char* who, const char* fmt, ...) {
    const int at = snprintf(msg, n, "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (at >= 0 && (size_t)at < n) vsnprintf(msg + at, n - (size_t)at, fmt, ap);
    va_end(ap);
    return TTS_HIP_EINVAL;
}

// Every reason a call is refused for what it asks (a handle without finalized weights is waveglow_call's business), first
// match wins, in this order: precision, mem kind, keys / offsets, B, mel / audio / T, B * T, packed without lengths,
// lengths[b], then the one-run limit (F of a packed call, T of any other).  Reads host memory only (lengths); TTS_HIP_OK or
// TTS_HIP_EINVAL with the reason in `msg`.  Nothing is copied or launched before it has passed.
// (audio = false: the probe below, which has its own one output, skips the test of c.audio.)
inline int wg_call_check(const WgCall& c, char* msg, size_t n, bool audio = true) {
    if (c.precision < 0 || c.precision > 2)
        return wg_refuse(msg, n, c.who, "precision must be 0 (f32), 1 (f16) or 2 (f16x3), got %d", c.precision);
    if (!c.async && c.mem != TTS_HIP_MEM_HOST && c.mem != TTS_HIP_MEM_DEVICE)
        return wg_refuse(msg, n, c.who, "bad mem kind %d", c.mem);
    if (c.noise == WG_NOISE_ROWS && (!c.keys || !c.offsets)) return wg_refuse(msg, n, c.who, "keys / offsets is NULL");
    if (c.B <= 0) return wg_refuse(msg, n, c.who, "bad argument: B = %d must be positive", c.B);
    if (!c.mel || (audio && !c.audio) || c.T <= 0) return wg_refuse(msg, n, c.who, "bad argument (mel or audio is NULL, or T = %d <= 0)", c.T);
    if ((long long)c.B * c.T * 32 > kMaxGroups)
        return wg_refuse(msg, n, c.who, "B*T too large (B = %d, T = %d: above 2^25 frames)", c.B, c.T);
    if (c.packed && !c.lengths) return wg_refuse(msg, n, c.who, "packed needs lengths, got NULL");
    if (c.lengths)
        for (int b = 0; b < c.B; ++b)
            if (c.lengths[b] < 0 || c.lengths[b] > c.T)
                return wg_refuse(msg, n, c.who, "lengths[%d] = %d is outside [0, T = %d]", b, (int)c.lengths[b], c.T);
    // One run addresses its activations with 31-bit byte offsets.  Rows are independent, so a larger batch runs in slices of
    // whole rows, but a single row above the limit is refused (the Python wrapper's windowed inference is the answer to long
    // mels); a packed row is ONE run: no slicing, and no silent fall-back to the ragged path.
    if (c.packed) {
        int rows = 0;
        const long long F = wg_packed_frames(c.B, c.lengths, &rows);
        if (F > kMaxFramesPerRun)
            return wg_refuse(msg, n, c.who,
                             "the packed row holds F = %lld frames (%d rows with frames, %d gap frames between two), above one "
                             "run's limit (%d); split the batch or use the ragged call",
                             F, rows, TTS_HIP_WG_GAP_FRAMES, kMaxFramesPerRun);
    } else if (c.T > kMaxFramesPerRun) {
        return wg_refuse(msg, n, c.who, "T = %d frames exceeds one run's limit (%d); use windowed inference", c.T,
                         kMaxFramesPerRun);
    }
    return TTS_HIP_OK;
}

// Where the inverse direction's test hook (tts_hip_waveglow_probe_rows and the two older symbols that call it) stops and what
// it copies to `out`: what 0 the gated activations of WN layer `layer` of flow `flow`, 1 the flow state after flow `flow`,
// 2 that layer's conditioning plane (fp32 only).
struct WgProbe {
    int flow, what, layer;
    float* out;
};
// Refused: whatever wg_call_check refuses of the same mel / B / T / lengths / packed / precision / mem (c.audio is not looked
// at), then flow outside 0 .. 11, what outside 0 .. 2, layer outside 0 .. 7, what 2 in another precision than fp32, more
// frames than one run holds (B * T; a packed row's F was wg_call_check's last reason already: the probe is one run, it does
// not slice), out NULL.
inline int wg_probe_check(const WgCall& c, const WgProbe& p, char* msg, size_t n) {
    if (int rc = wg_call_check(c, msg, n, false)) return rc;
    if (p.flow < 0 || p.flow > 11) return wg_refuse(msg, n, c.who, "flow = %d is outside [0, 11]", p.flow);
    if (p.what < 0 || p.what > 2) return wg_refuse(msg, n, c.who, "what = %d must be 0 (acts), 1 (state) or 2 (cond)", p.what);
    if (p.layer < 0 || p.layer > 7) return wg_refuse(msg, n, c.who, "layer = %d is outside [0, 7]", p.layer);
    if (p.what == 2 && c.precision != 0)
        return wg_refuse(msg, n, c.who, "what = 2 (cond) needs precision 0 (f32), got %d: only fp32 builds the plane", c.precision);
    if (!c.packed && (long long)c.B * c.T > kMaxFramesPerRun)
        return wg_refuse(msg, n, c.who, "B * T = %lld frames exceeds one run's limit (%d); the probe is one run",
                         (long long)c.B * c.T, kMaxFramesPerRun);
    if (!p.out) return wg_refuse(msg, n, c.who, "bad argument: out is NULL");
    return TTS_HIP_OK;
}

// One forward-flow call (tts_hip_waveglow_encode[_async], fp32): audio [B, T*256] and mel [B, T, 80] in, z [B, T*32, 8] and
// stats [3, B] out, either of which may be NULL.
struct WgEncode {
    const char* who;                 // the entry point, as messages name it
    const float *audio, *mel;
    int B, T;
    const int32_t* lengths;          // NULL or host int32 [B]
    float *z, *stats;
    bool async;                      // as WgCall::async / mem / stream
    int mem;
    void* stream;
};

// Every reason a forward-flow call is refused for what it asks, first match wins, in this order: mem kind, B, audio / mel / T,
// both outputs NULL, lengths[b], then B * T above one run (the call is one run: no slicing).  Reads host memory only
// (lengths); nothing is copied or launched before it has passed.
// (outputs = false: the probe below, which has its own one output, skips the check of z / stats.)
inline int wg_encode_check(const WgEncode& c, char* msg, size_t n, bool outputs = true) {
    if (!c.async && c.mem != TTS_HIP_MEM_HOST && c.mem != TTS_HIP_MEM_DEVICE)
        return wg_refuse(msg, n, c.who, "bad mem kind %d", c.mem);
    if (c.B <= 0) return wg_refuse(msg, n, c.who, "bad argument: B = %d must be positive", c.B);
    if (!c.audio || !c.mel || c.T <= 0) return wg_refuse(msg, n, c.who, "bad argument (audio or mel is NULL, or T = %d <= 0)", c.T);
    if (outputs && !c.z && !c.stats) return wg_refuse(msg, n, c.who, "bad argument: z and stats are both NULL, nothing to compute");
    if (c.lengths)
        for (int b = 0; b < c.B; ++b)
            if (c.lengths[b] < 0 || c.lengths[b] > c.T)
                return wg_refuse(msg, n, c.who, "lengths[%d] = %d is outside [0, T = %d]", b, (int)c.lengths[b], c.T);
    if ((long long)c.B * c.T > kMaxFramesPerRun)
        return wg_refuse(msg, n, c.who, "B * T = %lld frames exceeds one run's limit (%d); encode the batch in slices of rows",
                         (long long)c.B * c.T, kMaxFramesPerRun);
    return TTS_HIP_OK;
}

// Where the forward direction's test hook (tts_hip_waveglow_encode_probe) stops and what it copies: after flow `flow`
// (-1: after the init step) the flow state as stored (what 0) or the running per-position sum of s (what 1), to `out`.
struct WgEncodeProbe {
    int flow, what;
    float* out;
};
// Refused: whatever wg_encode_check refuses of the same audio / mel / B / T / lengths / mem (c.z and c.stats are not looked
// at), then flow outside -1 .. 11, what outside 0 .. 1, what 1 with flow -1 (no s has been summed yet), out NULL.
inline int wg_encode_probe_check(const WgEncode& c, const WgEncodeProbe& p, char* msg, size_t n) {
    if (int rc = wg_encode_check(c, msg, n, false)) return rc;
    if (p.flow < -1 || p.flow > 11) return wg_refuse(msg, n, c.who, "flow = %d is outside [-1, 11]", p.flow);
    if (p.what < 0 || p.what > 1) return wg_refuse(msg, n, c.who, "what = %d must be 0 (state) or 1 (slog)", p.what);
    if (p.what == 1 && p.flow < 0) return wg_refuse(msg, n, c.who, "what = 1 (slog) needs flow >= 0: no s is summed before flow 0");
    if (!p.out) return wg_refuse(msg, n, c.who, "bad argument: out is NULL");
    return TTS_HIP_OK;
}

// What a call with lengths stages to the device, once, as one int32 table:
//   ragged: [lengths[B] | tail frames], the tail frames (b - b0) * T + t, t >= lengths[b], listed run by run (b0 = first row
//           of the run of chunkB rows that holds row b), so that run r finds its own run_tails[r] as one contiguous slice;
//   packed: [start[B] | len[B] | flags[F] | gap frames[n_gap]], flags[f] = 1 + b * T + t on the packed frame that holds frame
//           t of row b (non-zero = real, and the gather's source index), 0 on a gap frame; start of an empty row stays 0
//           (the scatter reads nothing of such a row).
// counts[b] = noise values row b needs (lengths[b] * 256; T * 256 without lengths, where `info` stays empty).
struct WgTable {
    std::vector<int> info;
    std::vector<int> run_tails;
    std::vector<long long> counts;
    int F = 0, n_gap = 0;
};

// (arguments already passed wg_call_check; chunkB: rows per run, not used by a packed call)
inline void wg_call_table(int B, int T, const int32_t* lengths, bool packed, int chunkB, WgTable* t) {
    t->F = t->n_gap = 0;
    t->info.clear();
    t->run_tails.clear();
    t->counts.assign((size_t)B, (long long)T * 256);
    if (!lengths) return;
    for (int b = 0; b < B; ++b) t->counts[b] = (long long)lengths[b] * 256;
    if (packed) {
        int rows = 0;
        const long long F = wg_packed_frames(B, lengths, &rows);
        const long long n_gap = rows > 1 ? (long long)TTS_HIP_WG_GAP_FRAMES * (rows - 1) : 0;
        t->info.assign((size_t)2 * B + (size_t)F + (size_t)n_gap, 0);
        int* start = t->info.data();
        int* len = start + B;
        int* flags = len + B;
        int* gaps = flags + F;
        int pos = 0, g = 0;
        bool first = true;
        for (int b = 0; b < B; ++b) {
            len[b] = lengths[b];
            if (lengths[b] == 0) continue;
            if (!first)
                for (int j = 0; j < TTS_HIP_WG_GAP_FRAMES; ++j) gaps[g++] = pos++;
            first = false;
            start[b] = pos;
            for (int i = 0; i < lengths[b]; ++i) flags[pos++] = 1 + b * T + i;
        }
        t->F = (int)F;
        t->n_gap = (int)n_gap;
        return;
    }
    long long n_tail = 0;
    for (int b = 0; b < B; ++b) n_tail += T - lengths[b];
    t->info.resize((size_t)B + (size_t)n_tail);
    t->run_tails.assign((size_t)((B + chunkB - 1) / chunkB), 0);
    size_t at = (size_t)B;
    for (int b = 0; b < B; ++b) {
        t->info[b] = lengths[b];
        t->run_tails[b / chunkB] += T - lengths[b];
        for (int i = lengths[b]; i < T; ++i) t->info[at++] = (b % chunkB) * T + i;
    }
}
