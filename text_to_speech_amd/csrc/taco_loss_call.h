// taco_loss_call.h -- what one TacotronLoss call (tts_hip_tacotron2_loss, taco_loss.hip) is, why it may be refused and how its
// workspace is laid out: pure host code on the caller's arguments (no HIP include; also built with plain g++ under ASan / UBSan
// by csrc/host_check.cpp, --taco-loss, and compared there with a Python restatement, tests/test_taco_loss.py).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstddef>

#include "taco_call.h"      // taco_refuse, taco_bad_mem, kMaxForwardFrames: a loss call takes what a forward call can return

constexpr int kLossMel = 80;                 // channels of a frame
constexpr int kLossChunkFrames = 16;         // frames of a row one block sums: a row is cut by T alone, never by B or its index
constexpr int kLossMaxKinds = 4;
// One block's partial sums, float64, in this order: the masked error of decoder_output per kind code 0 .. 3, the same of mel,
// the sum of the mask, the sum of the weighted gate term
constexpr int kLossSums = 2 * kLossMaxKinds + 2, kLossSumMask = 2 * kLossMaxKinds, kLossSumGate = 2 * kLossMaxKinds + 1;

struct TacoLossCall {
    const char* who;                 // the entry point, as messages name it
    const float *mel_target, *gate_target, *decoder_output, *mel, *stop_tokens;      // [B, T, 80] | [B, T]
    int B, T;
    const int32_t* kinds;            // host int32 [n_kinds], TTS_HIP_LOSS_*
    int n_kinds;
    bool mask_mel_padding, from_logits;
    double finish_weight, not_finish_weight;
    float* out;                      // [2 + 2 n_kinds, B]
    int mem;
    void* stream;                    // NULL = the handle's
};

// Where the call's buffers start in the handle's loss workspace, in bytes (each 256-aligned), and its size
struct TacoLossLayout {
    int chunks;                      // ceil(T / kLossChunkFrames)
    int K;                           // 2 + 2 n_kinds
    bool weighted;                   // a weighted kind is asked for: the row extrema pass runs
    size_t in[5];                    // staged inputs of a TTS_HIP_MEM_HOST call, in the argument order (else unused, 0 bytes)
    size_t extrema;                  // float [B][chunks][2]: min(y), min(-y) of each chunk of mel_target (weighted only)
    size_t sums;                     // double [B][chunks][kLossSums]
    size_t out;                      // float [K][B]
    size_t bytes;
};

inline bool taco_loss_weighted(int kind) { return kind == TTS_HIP_LOSS_WEIGHTED_MSE || kind == TTS_HIP_LOSS_WEIGHTED_MAE; }

// Every reason a loss call is refused, first match wins, in this order: a NULL pointer, B / T below 1, B * T above the forward
// pass's frame limit, n_kinds, an unknown kind, a repeated kind, mem kind, the two weights, a device pointer to a [B, T, 80]
// array that is not 16-byte aligned (the pass loads float4).  Reads host memory only (kinds); TTS_HIP_OK or TTS_HIP_EINVAL with
// the reason in `msg`.  Nothing is copied or launched before it has passed.
inline int taco_loss_check(const TacoLossCall& c, char* msg, size_t n) {
    const struct { const void* p; const char* name; } ptrs[] = {
        {c.mel_target, "mel_target"}, {c.gate_target, "gate_target"}, {c.decoder_output, "decoder_output"}, {c.mel, "mel"},
        {c.stop_tokens, "stop_tokens"}, {c.kinds, "kinds"}, {c.out, "out"}};
    for (const auto& a : ptrs)
        if (!a.p) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%s is NULL", a.name);
    if (c.B < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B = %d must be at least 1", c.B);
    if (c.T < 1) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "T = %d must be at least 1", c.T);
    if ((long long)c.B * c.T > kMaxForwardFrames)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "B*T too large (B = %d, T = %d: above %lld frames); split the batch", c.B,
                           c.T, kMaxForwardFrames);
    if (c.n_kinds < 1 || c.n_kinds > kLossMaxKinds)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "n_kinds = %d is outside [1, %d]", c.n_kinds, kLossMaxKinds);
    for (int i = 0; i < c.n_kinds; ++i) {
        if (c.kinds[i] < 0 || c.kinds[i] >= kLossMaxKinds)
            return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "kinds[%d] = %d is no mel loss (0 mse, 1 mae, 2 weighted_mse, 3 weighted_mae)",
                               i, (int)c.kinds[i]);
        for (int j = 0; j < i; ++j)
            if (c.kinds[j] == c.kinds[i])
                return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "kinds[%d] repeats kinds[%d] = %d", i, j, (int)c.kinds[i]);
    }
    if (taco_bad_mem(c.mem)) return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "bad mem kind %d", c.mem);
    if (!std::isfinite(c.finish_weight) || c.finish_weight < 0)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "finish_weight = %g must be finite and not negative", c.finish_weight);
    if (!std::isfinite(c.not_finish_weight) || c.not_finish_weight < 0)
        return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "not_finish_weight = %g must be finite and not negative", c.not_finish_weight);
    if (c.mem == TTS_HIP_MEM_DEVICE)
        for (int i = 0; i < 4; ++i)
            if (i != 1 && (uintptr_t)ptrs[i].p % 16)
                return taco_refuse(msg, n, c.who, TTS_HIP_EINVAL, "%s is not 16-byte aligned", ptrs[i].name);
    return TTS_HIP_OK;
}

// (arguments already passed taco_loss_check)
inline TacoLossLayout taco_loss_layout(const TacoLossCall& c) {
    TacoLossLayout l{};
    l.chunks = (c.T + kLossChunkFrames - 1) / kLossChunkFrames;
    l.K = 2 + 2 * c.n_kinds;
    for (int i = 0; i < c.n_kinds; ++i) l.weighted |= taco_loss_weighted(c.kinds[i]);
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const size_t frames = (size_t)c.B * c.T;
    for (int i = 0; i < 5; ++i)
        l.in[i] = take(c.mem == TTS_HIP_MEM_HOST ? frames * (i == 1 || i == 4 ? 1 : kLossMel) * sizeof(float) : 0);
    l.extrema = take(l.weighted ? (size_t)c.B * l.chunks * 2 * sizeof(float) : 0);
    l.sums = take((size_t)c.B * l.chunks * kLossSums * sizeof(double));
    l.out = take((size_t)l.K * c.B * sizeof(float));
    l.bytes = at;
    return l;
}
