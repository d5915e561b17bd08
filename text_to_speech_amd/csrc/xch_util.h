// xch_util.h -- device helpers shared by the decoder kernels that exchange small vectors between CUs inside one launch
// (taco_persist.hip, taco_fused.hip): tagged 8-byte publishes, DPP cross-lane moves and wave reductions, row dot products,
// weight-vector loads, fast gate functions.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dev_util.h"

namespace ttsxch {
using namespace ttsgemm;

typedef unsigned long long u64;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned fbits(float v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ float bitsf(unsigned v) { return __builtin_bit_cast(float, v); }

__device__ __forceinline__ void publish(u64* p, unsigned tag, float v) {
    __hip_atomic_store(p, ((u64)tag << 32) | fbits(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// buffer descriptor of a whole area (the exchange area, a memory slice): no bounds in the way, raw dword addressing
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x80000000u, 0x00020000);
}
// debug builds (-DTTS_DEBUG_HOOKS): the four blocks that record phase timestamps -> their trace slot, every other block -1
__device__ __forceinline__ int trace_block(int blk) { return blk == 0 ? 0 : blk == 80 ? 1 : blk == 200 ? 2 : blk == 255 ? 3 : -1; }

// Cross-lane moves on the DPP path (a few cycles) instead of ds_bpermute (an LDS round trip, ~100+ cycles each): the
// step's critical path holds ~50 dependent reductions steps, which cost more than the arithmetic.
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E;          // quad_perm [1,0,3,2], [2,3,0,1]
constexpr int DPP_REV4 = 0x1B;                           // quad_perm [3,2,1,0]: lane ^ 3
constexpr int DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140, DPP_ROR4 = 0x124, DPP_ROR8 = 0x128;   // i -> 7 - i, i -> 15 - i, rotations
__device__ __forceinline__ float lane_bcast(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// sum / max over the 64 lanes, result in every lane: four DPP steps inside each row of 16, then the four row results
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp<DPP_XOR1>(v);
    v += dpp<DPP_XOR2>(v);
    v += dpp<DPP_HALF_MIRROR>(v);
    v += dpp<DPP_MIRROR>(v);
    return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp<DPP_XOR1>(v));
    v = fmaxf(v, dpp<DPP_XOR2>(v));
    v = fmaxf(v, dpp<DPP_HALF_MIRROR>(v));
    v = fmaxf(v, dpp<DPP_MIRROR>(v));
    return fmaxf(fmaxf(lane_bcast(v, 0), lane_bcast(v, 16)), fmaxf(lane_bcast(v, 32), lane_bcast(v, 48)));
}
// partner exchange lane ^ (1 << S) inside a row of 16 lanes
template <int S>
__device__ __forceinline__ float row_xor(float v, int lane) {
    if constexpr (S == 0) return dpp<DPP_XOR1>(v);
    else if constexpr (S == 1) return dpp<DPP_XOR2>(v);
    else if constexpr (S == 2) return dpp<DPP_HALF_MIRROR>(dpp<DPP_REV4>(v));    // (i ^ 7) ^ 3 = i ^ 4: two symmetric moves
    else return dpp<DPP_ROR8>(v);
}

// Lane-halving reduction of V (= 8, 16 or 32) per-lane partial sums.  Halving step s pairs lane with lane ^ (1 << s) inside
// its row of 16 (DPP): lanes with bit s clear keep the lower half of the values and receive the partner's, the others the
// upper half -- so after log2 V steps a lane holds ONE value, index = bit reversal of its low log2 V lane bits.  V = 8 folds
// the rest of its row with a rotation (which preserves those bits), V = 32 does its fifth halving across rows; the remaining
// rows are folded with ds_bpermute steps.  Every lane whose low bits are bitrev(i) ends up with the wave total of value i.
template <int V>
__device__ __forceinline__ float reduce_lanes(float (&acc)[V], int lane) {
    static_assert(V == 8 || V == 16 || V == 32, "V");
    auto halve = [&](auto S, int half) {
        const bool hi = (lane >> decltype(S)::value) & 1;
#pragma unroll
        for (int i = 0; i < V / 2; ++i) {
            if (i < half) {
                float a_lo = acc[i], a_hi = acc[i + half];
                asm volatile("" : "+v"(a_lo), "+v"(a_hi));      // keeps select(load, load) from becoming an indexed load
                const float send = hi ? a_lo : a_hi;
                const float keep = hi ? a_hi : a_lo;
                acc[i] = keep + row_xor<decltype(S)::value>(send, lane);
            }
        }
    };
    halve(std::integral_constant<int, 0>{}, V / 2);
    halve(std::integral_constant<int, 1>{}, V / 4);
    halve(std::integral_constant<int, 2>{}, V / 8);
    if constexpr (V >= 16) halve(std::integral_constant<int, 3>{}, V / 16);
    float v;
    if constexpr (V == 32) {
        const bool hi = (lane >> 4) & 1;
        float a_lo = acc[0], a_hi = acc[1];
        asm volatile("" : "+v"(a_lo), "+v"(a_hi));
        const float send = hi ? a_lo : a_hi;
        const float keep = hi ? a_hi : a_lo;
        v = keep + __shfl_xor(send, 16, 64);
    } else {
        v = acc[0];
        if constexpr (V == 8) v += dpp<DPP_ROR8>(v);
        v += __shfl_xor(v, 16, 64);
    }
    v += __shfl_xor(v, 32, 64);
    return v;
}
// lane (of row 0) that holds value `idx` of V after the halving steps: the bit reversal of idx in log2 V bits
template <int V>
__device__ __forceinline__ int reduced_lane(int idx) {
    static_assert(V >= 4 && V <= 32 && (V & (V - 1)) == 0, "V");
    constexpr int LOGV = V == 4 ? 2 : V == 8 ? 3 : V == 16 ? 4 : 5;
    return (int)(__brev((unsigned)idx) >> (32 - LOGV));
}

// role wave: s[b] = row . x[b][cols]   (NI slices of 256 columns; slice i of the row multiplies x columns col[i] ..)
template <int NBT, int NI>
__device__ __forceinline__ void role_dots(float (&s)[NBT], const f32x4 (&R)[NI], const float* xs, int ldx, const int (&col)[NI], int lane) {
#pragma unroll
    for (int b = 0; b < NBT; ++b) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + b * ldx + col[i] + lane * 4);
            acc = fmaf(xv[0], R[i][0], acc);
            acc = fmaf(xv[1], R[i][1], acc);
            acc = fmaf(xv[2], R[i][2], acc);
            acc = fmaf(xv[3], R[i][3], acc);
        }
        s[b] = wave_sum(acc);
    }
}
// s[lane] for the lanes below NBT (one row per lane: the lane that publishes row b's value), 0 elsewhere
template <int NBT>
__device__ __forceinline__ float pick_row(const float (&s)[NBT], int lane) {
    float v = 0.f;
#pragma unroll
    for (int b = 0; b < NBT; ++b) v = lane == b ? s[b] : v;
    return v;
}

// LSTM weight matrices are fp32, or fp16 when HW: four consecutive columns of a row per lane.  NT: non-temporal load (the
// fused kernels' weight stream; the persistent kernel loads its rows once per utterance and passes false).
template <bool HW>
struct WT {
    typedef typename std::conditional<HW, f16x4, f32x4>::type vec;
    typedef typename std::conditional<HW, _Float16, float>::type el;
};
template <bool HW, bool NT>
__device__ __forceinline__ typename WT<HW>::vec load_w(const void* base, long long elem) {
    const typename WT<HW>::vec* p = reinterpret_cast<const typename WT<HW>::vec*>((const typename WT<HW>::el*)base + elem);
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// LSTM gate non-linearities on the transcendental unit: sigmoid(x) = rcp(1 + 2^(-x log2 e)), tanh(x) = 2 sigmoid(2 x) - 1
// (v_exp_f32 / v_rcp_f32, 1 ulp each; absolute error < 2e-7) instead of libm expf / tanhf and IEEE divisions, which were a
// third of the compute on the step's critical path.
__device__ __forceinline__ float sigmoid_fast(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}
__device__ __forceinline__ float tanh_fast(float x) {
    const float xc = fminf(fmaxf(x, -15.f), 15.f);
    return 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(xc * -2.885390081777927f)) - 1.f;
}

}  // namespace ttsxch
