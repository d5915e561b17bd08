// taco_call.h -- what one Tacotron2 call is, why it may be refused and how large the teacher-forced pass's buffers are: pure
// host code on the caller's arguments (no HIP include; also built with plain g++ under ASan / UBSan by csrc/host_check.cpp,
// --taco-call, and compared there with a Python restatement, tests/test_taco_call.py).  Every tts_hip_tacotron2_* entry point
// fills a TacoEncode, a TacoRun or both (infer = encode + decode) and hands them to one driver (tacotron2.hip).
#pragma once
#include <stdint.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "../../include/tts_hip.h"

constexpr int kMaxEncodeRows = 1024, kMaxEncodeTokens = 4096;      // B and Tin of one encoder run
constexpr long long kMaxForwardFrames = 65536;      // B * T: the hoisted gate term is 16 KiB per frame, 1 GiB here
constexpr int kForwardGateCols = 4096;              // 4 gates x 1024 units of the attention LSTM
constexpr int kForwardPrenet = 256, kForwardMel = 80, kForwardRnn = 1024;

// The encoder on a token batch (encode, reencode, probe_encoder, the first half of infer)
struct TacoEncode {
    const char* who;                 // the entry point, as messages name it
    bool model_ready;                // the handle holds finalized Tacotron2 weights ...
    int spk_dim;                     // ... which expect a speaker embedding of this width (0: none)
    const int32_t* tokens;           // [B, Tin], 0 = pad
    int B, Tin;
    const float* speaker;            // NULL or [B, spk_dim]
    int mem;
    void* stream;                    // NULL = the handle's
};

enum TacoKind { TACO_DECODE = 0, TACO_FORWARD = 1 };      // the free-running loop | the teacher-forced pass

enum TacoMasks {
    TACO_MASKS_NONE = 0,     // deterministic prenet
    TACO_MASKS_TENSOR = 1,   // the caller's prenet_masks [B, len, 2, 256]
    TACO_MASKS_SEED = 2,     // drawn into the workspace from one stream (seed, offset), batch layout
    TACO_MASKS_ROWS = 3      // drawn into the workspace from one stream (keys[b], offsets[b]) per row
};

// A run on an encoded batch (decode*, forward, the second half of infer)
struct TacoRun {
    const char* who;
    TacoKind kind;
    bool model_ready;                // the handle holds finalized Tacotron2 weights
    bool has_encoded;                // the encoded batch is non-NULL and holds a buffer (infer: the one it is about to fill)
    int B, Tin, enc;                 // the encoded batch's rows, tokens per row and width (512 or 768)
    int model_enc;                   // the width the handle's weights expect
    int len;                         // decode: max_len, the steps allocated; forward: T, the steps run
    int early_stop, win_len, win_offset;      // decode
    int precision;                   // 0 f32, 1 fp16 LSTM weights
    TacoMasks masks;
    const float* prenet_masks;       // TACO_MASKS_TENSOR
    uint64_t seed, offset;           // TACO_MASKS_SEED
    const uint64_t *keys, *offsets;  // TACO_MASKS_ROWS: host uint64 [B]
    const float* mel_input;          // forward: [B, T, 80], already shifted
    const int32_t* mel_lengths;      // forward: host int32 [B], each in 1 .. T
    float *mel, *decoder_output, *stop_tokens, *attention;      // any may be NULL
    int32_t *lengths, *steps_run;    // decode; any may be NULL
    int mem;
    void* stream;                    // NULL = the handle's
};

// The buffers of a forward call that scale with its B * T frames, in floats (the engine lays them out with exactly these counts)
struct TacoForwardSizes {
    long long frames;                // B * T
    size_t mel_in;                   // [frames][80]    staged input
    size_t prenet;                   // [frames][256]   each of the two prenet layers
    size_t gates;                    // [frames][4096]  hoisted attention-LSTM term
    size_t history;                  // [B * bucket(T)][1024 + enc]  cell_out of every step (rows addressed with the real T)
    size_t proj;                     // [frames][81]    projection and gate before mask / sigmoid
};

inline int taco_forward_bucket(int T) { return (T + 255) / 256 * 256; }      // the decode workspace's max_len bucket

inline int taco_refuse(char* msg, size_t n, const char* who, int code, const char* fmt, ...) {
    const int at = snprintf(msg, n, "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (at >= 0 && (size_t)at < n) vsnprintf(msg + at, n - (size_t)at, fmt, ap);
    va_end(ap);
    return code;
}

inline bool taco_bad_mem(int mem) { return mem != TTS_HIP_MEM_HOST && mem != TTS_HIP_MEM_DEVICE; }

// Every reason an encoder run is refused, first match wins, in this order: mem kind, model not ready, tokens / B / Tin
// (1 .. 1024 rows of 1 .. 4096 tokens), a missing speaker embedding.  Reads no memory; TTS_HIP_OK, TTS_HIP_ENOTREADY or
// TTS_HIP_EINVAL with the reason in `msg`.  Nothing is copied or launched before it has passed.
inline int taco_encode_check(const TacoEncode& c, char* msg, size_t n) {
    if (taco_bad_mem(c.mem)) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad mem kind %d", c.mem);
    if (!c.model_ready) return taco_refuse(msg, n, c.who, TTS_HIP_ENOTREADY, "tacotron2 weights not finalized");
    if (!c.tokens || c.B <= 0 || c.B > kMaxEncodeRows || c.Tin <= 0 || c.Tin > kMaxEncodeTokens)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad argument (tokens is NULL, or B = %d outside [1, %d], or Tin = %d outside [1, %d])",
                           c.B, kMaxEncodeRows, c.Tin, kMaxEncodeTokens);
    if (c.spk_dim > 0 && !c.speaker) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "this model needs a speaker embedding");
    return TTS_HIP_OK;
}

// Every reason a run on an encoded batch is refused, first match wins, in this order: precision, mem kind, model not ready,
// encoded batch, its width, then the pointers (decode: keys / offsets of TACO_MASKS_ROWS; forward: mel_input / mel_lengths),
// len (max_len / T), and for forward B * T and mel_lengths[b].  A decode call words a NULL or empty batch and a bad max_len as
// "bad argument: ...".  Reads host memory only (mel_lengths); TTS_HIP_OK, TTS_HIP_ENOTREADY or TTS_HIP_EINVAL with the reason
// in `msg`.  Nothing is copied or launched before it has passed.
inline int taco_run_check(const TacoRun& c, char* msg, size_t n) {
    const bool fwd = c.kind == TACO_FORWARD;
    const char* bad = fwd ? "" : "bad argument: ";
    if (c.precision != 0 && c.precision != 1)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "precision must be 0 (f32) or 1 (f16 weights), got %d", c.precision);
    if (taco_bad_mem(c.mem)) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad mem kind %d", c.mem);
    if (!c.model_ready) return taco_refuse(msg, n, c.who, TTS_HIP_ENOTREADY, "tacotron2 weights not finalized");
    if (!c.has_encoded || c.B <= 0 || c.Tin <= 0)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%sencoded batch is NULL or empty", bad);
    if (c.enc != c.model_enc)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "encoded batch belongs to other weights (width %d, model %d)", c.enc,
                           c.model_enc);
    if (!fwd && c.masks == TACO_MASKS_ROWS && (!c.keys || !c.offsets))
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "keys / offsets is NULL");
    if (fwd && (!c.mel_input || !c.mel_lengths))
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "mel_input or mel_lengths is NULL");
    if (c.len < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%s%s = %d must be at least 1", bad, fwd ? "T" : "max_len", c.len);
    if (!fwd) return TTS_HIP_OK;
    if ((long long)c.B * c.len > kMaxForwardFrames)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B*T too large (B = %d, T = %d: above %lld frames); split the batch", c.B,
                           c.len, kMaxForwardFrames);
    for (int b = 0; b < c.B; ++b)
        if (c.mel_lengths[b] < 1 || c.mel_lengths[b] > c.len)
            return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "mel_lengths[%d] = %d is outside [1, T = %d]", b,
                               (int)c.mel_lengths[b], c.len);
    return TTS_HIP_OK;
}

// (arguments already passed taco_run_check)
inline TacoForwardSizes taco_forward_sizes(int B, int T, int enc) {
    TacoForwardSizes s{};
    s.frames = (long long)B * T;
    s.mel_in = (size_t)s.frames * kForwardMel;
    s.prenet = (size_t)s.frames * kForwardPrenet;
    s.gates = (size_t)s.frames * kForwardGateCols;
    s.history = (size_t)B * taco_forward_bucket(T) * (size_t)(kForwardRnn + enc);
    s.proj = (size_t)s.frames * (kForwardMel + 1);
    return s;
}
