// taco_forward_call.h -- what one teacher-forced Tacotron2 call (tts_hip_tacotron2_forward) is, why it may be refused and how
// large its buffers are: pure host code on the caller's arguments (no HIP include; also built with plain g++ under ASan /
// UBSan by csrc/host_check.cpp, --taco-forward, and compared there with a Python restatement, tests/test_teacher_forced.py).
#pragma once
#include <stdint.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "../../include/tts_hip.h"

constexpr long long kMaxForwardFrames = 65536;      // B * T: the hoisted gate term is 16 KiB per frame, 1 GiB here
constexpr int kForwardGateCols = 4096;              // 4 gates x 1024 units of the attention LSTM
constexpr int kForwardPrenet = 256, kForwardMel = 80, kForwardRnn = 1024;

struct TacoForwardCall {
    const char* who;                 // the entry point, as messages name it
    bool model_ready;                // the handle holds finalized Tacotron2 weights
    bool has_encoded;                // the encoded batch is non-NULL and holds a buffer
    int B, Tin, enc;                 // the encoded batch's rows, tokens per row and width (512 or 768)
    int model_enc;                   // the width the handle's weights expect
    const float* mel_input;          // [B, T, 80], already shifted
    int T;
    const int32_t* mel_lengths;      // host int32 [B], each in 1 .. T
    int precision;                   // 0 f32, 1 fp16 LSTM weights
    int mem;
};

// The buffers of a call that scale with its B * T frames, in floats (the engine lays them out with exactly these counts)
struct TacoForwardSizes {
    long long frames;                // B * T
    size_t mel_in;                   // [frames][80]    staged input
    size_t prenet;                   // [frames][256]   each of the two prenet layers
    size_t gates;                    // [frames][4096]  hoisted attention-LSTM term
    size_t history;                  // [B * bucket(T)][1024 + enc]  cell_out of every step (rows addressed with the real T)
    size_t proj;                     // [frames][81]    projection and gate before mask / sigmoid
};

inline int taco_forward_bucket(int T) { return (T + 255) / 256 * 256; }      // the decode workspace's max_len bucket

inline int taco_forward_refuse(char* msg, size_t n, const char* who, int code, const char* fmt, ...) {
    const int at = snprintf(msg, n, "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (at >= 0 && (size_t)at < n) vsnprintf(msg + at, n - (size_t)at, fmt, ap);
    va_end(ap);
    return code;
}

// Every reason a call is refused, first match wins, in this order: precision, mem kind, model not ready, encoded batch,
// its width, mel_input / mel_lengths, T, B * T, mel_lengths[b].  Reads host memory only (mel_lengths); TTS_HIP_OK,
// TTS_HIP_ENOTREADY or TTS_HIP_EINVAL with the reason in `msg`.  Nothing is copied or launched before it has passed.
inline int taco_forward_check(const TacoForwardCall& c, char* msg, size_t n) {
    if (c.precision != 0 && c.precision != 1)
        return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "precision must be 0 (f32) or 1 (f16 weights), got %d", c.precision);
    if (c.mem != TTS_HIP_MEM_HOST && c.mem != TTS_HIP_MEM_DEVICE)
        return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad mem kind %d", c.mem);
    if (!c.model_ready) return taco_forward_refuse(msg, n, c.who, TTS_HIP_ENOTREADY, "tacotron2 weights not finalized");
    if (!c.has_encoded || c.B <= 0 || c.Tin <= 0)
        return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "encoded batch is NULL or empty");
    if (c.enc != c.model_enc)
        return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "encoded batch belongs to other weights (width %d, model %d)",
                                   c.enc, c.model_enc);
    if (!c.mel_input || !c.mel_lengths)
        return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "mel_input or mel_lengths is NULL");
    if (c.T < 1) return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "T = %d must be at least 1", c.T);
    if ((long long)c.B * c.T > kMaxForwardFrames)
        return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B*T too large (B = %d, T = %d: above %lld frames); split the batch",
                                   c.B, c.T, kMaxForwardFrames);
    for (int b = 0; b < c.B; ++b)
        if (c.mel_lengths[b] < 1 || c.mel_lengths[b] > c.T)
            return taco_forward_refuse(msg, n, c.who, TTS_HIP_EINVAL, "mel_lengths[%d] = %d is outside [1, T = %d]", b,
                                       (int)c.mel_lengths[b], c.T);
    return TTS_HIP_OK;
}

// (arguments already passed taco_forward_check)
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
