// audio_dev.h -- workgroup-wide reductions and scans of the audio kernels (audio_proc.hip, silence.hip): plain __shfl
// exchanges inside a wave of 64, one LDS slot per wave.  Not the decoder's latency path (xch_util.h has that, float only).
#pragma once
#include <hip/hip_runtime.h>

#include <limits>

struct OpAdd {
    template <class T> __device__ static T id() { return T(0); }
    template <class T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    template <class T> __device__ static T id() { return T(-1); }      // the values are >= 0 (indices, magnitudes), or -1
    template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct OpMin {
    template <class T> __device__ static T id() { return std::numeric_limits<T>::max(); }
    template <class T> __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};

// the reduction over the wave's 64 lanes, in every lane (xor butterfly, 32 first)
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}

// the reduction over the workgroup's threads (<= 1024: 16 waves of 64), in every thread: wave_reduce, one LDS slot per wave,
// then id, sh[0], sh[1], ... folded in that order.  A floating-point sum depends on that association, and the means it feeds
// are compared with thresholds: keep it.  sh holds 16 values; the helper may be called again at once (it ends on a barrier).
template <class T, class Op>
__device__ T block_reduce(T v, T* sh, Op op) {
    v = wave_reduce(v, op);
    const int nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = Op::template id<T>();
    for (int i = 0; i < nw; ++i) s = op(s, sh[i]);
    __syncthreads();
    return s;
}

// inclusive scan over the workgroup's threads (<= 1024: 16 waves of 64); `total` = the reduction over all of them, folded
// from the waves' scanned totals -- for a floating-point sum not the association of block_reduce.
// sh holds 16 values; the helper may be called again at once (it ends on a barrier).
template <class T, class Op>
__device__ T block_scan(T v, T* sh, T& total, Op op) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v = op(u, v);
    }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    T base = Op::template id<T>(), all = Op::template id<T>();
    for (int i = 0; i < nw; ++i) {
        if (i < w) base = op(base, sh[i]);
        all = op(all, sh[i]);
    }
    __syncthreads();
    total = all;
    return op(base, v);
}
