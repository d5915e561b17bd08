// wg_encode.hip -- the position-wise layer of WaveGlow's FORWARD flow (audio -> z and its log-likelihood terms) on gfx950.
//
// The forward flow (Prenger et al. 2018, section 2; oracle/waveglow_ref.forward_flow) runs the twelve flow steps in ascending
// order: invertible 1x1 convolution a <- a @ kernel_k[0], then the affine coupling a1 <- exp(s) a1 + b with (b, s) =
// WN_k(a0, spect); before flows 4 and 8 the first two channels leave as an early output.  The WN block is the one
// waveglow_run evaluates (waveglow.hip: start kernel, eight layers in either form, residual GEMMs); this file holds what
// surrounds it in this direction, fp32 only:
//   encode_init_kernel      natural [B, T*256] audio -> phase-major state [M'][8] with flow 0's matrix applied
//   wn_end_fwd_kernel       folded skip / end conv of a flow, forward coupling, the position's sum of s, and what the next flow
//                           needs: the early output leaves to z, the next flow's matrix is applied to what stays (after flow
//                           11: the final four channels go to z)
//   encode_stats_*_kernel   per row of the batch: sum z^2 and sum s over its real positions, and its log-determinant term
// Layouts, phase-major rows and the meaning of "real" frames: the header comment of waveglow.hip.
//
// Sums: no floating-point atomics anywhere.  Every position is finished by the same lane of the same wave in every flow's
// wn_end_fwd_kernel, so its `slog` entry is a plain read-modify-write; the row statistics are reduced in float64 in an order
// that depends on the call's shape only (fixed chunks, strided threads, a shared-memory tree), so repeats are bit-equal.
#include "engine.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NPH = 32;       // phases (sample groups per mel frame)
constexpr int RPW = 8;        // positions per wave of wn_end_fwd_kernel, as in wn_end_fold_kernel
constexpr int STAT_CHUNKS = 32;   // blocks per row of encode_stats_partial_kernel

enum { MASK_NONE = 0, MASK_LENS = 1 };
__device__ __forceinline__ bool frame_is_real(const int* __restrict__ lens, int f, int T) { return f % T < lens[f / T]; }

// state[m'][c] = sum_j audio[natural m][j] * w0[j][c], m' = p * PR + f  <->  m = f * 32 + p; padding rows (f >= BT) and frames
// that are not real get zeros, and their audio is not read.  One position per thread.
template <int MASK>
__global__ void encode_init_kernel(const float* __restrict__ audio, const float* __restrict__ w0, float* __restrict__ state,
                                   int PR, int BT, const int* __restrict__ lens, int T) {
    const long long mp = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (mp >= (long long)NPH * PR) return;
    const int p = (int)(mp / PR), f = (int)(mp % PR);
    bool real = f < BT;
    if constexpr (MASK != MASK_NONE) real = real && frame_is_real(lens, f, T);
    float y[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) y[c] = 0.f;
    if (real) {
        const float* src = audio + ((long long)f * NPH + p) * 8;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
        const float a[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) t = fmaf(a[j], w0[j * 8 + c], t);
            y[c] = t;
        }
    }
    const f32x4 o0 = {y[0], y[1], y[2], y[3]}, o1 = {y[4], y[5], y[6], y[7]};
    *reinterpret_cast<f32x4*>(state + mp * 8) = o0;
    *reinterpret_cast<f32x4*>(state + mp * 8 + 4) = o1;
}

// Folded skip/end conv + forward affine coupling + the next flow's 1x1 conv, RPW positions per wave.
//   out[m][o] = sum_layer sum_c acts[layer][m][c] * wfold[layer][o][c] + bfold[o]      (b = out[0 .. h), s = out[h .. 2h))
//   a1 = exp(s) * a1 + b;  slog[m] (+)= sum_j s[j];  then, with the state [a0, a1] of 2h channels:
//   next != null: the first n_early channels go to z[natural m][zoff ..], the other n = 2h - n_early are multiplied by the next
//                 flow's matrix next[n][n] and stored as the state;  next == null (flow 11): the 4 channels go to z[..][0 .. 3].
// Rows, lane ownership (C = 512: channels 4l..4l+3 and 256+4l..; C = 256: 4l..4l+3) and the 64-value lane-halving reduction are
// those of the fp32 instantiations of wn_end_fold_kernel (waveglow.hip), whose text this follows; lane 8r finishes position
// m0 + r.  MASK_LENS: positions of frames beyond their row's length store 0 (state, slog and the z channels this flow writes).
template <int MASK, int C>
__global__ __launch_bounds__(256) void wn_end_fwd_kernel(const float* __restrict__ acts, long long layer_stride,
                                                         const float* __restrict__ wfold, const float* __restrict__ bfold,
                                                         float* __restrict__ state, float* __restrict__ slog, int first,
                                                         const float* __restrict__ next, float* __restrict__ z, int zoff,
                                                         int n_early, long long M, int h, int PR, int BT,
                                                         const int* __restrict__ lens, int T) {
    static_assert(C == 512 || C == 256, "wn_end_fwd_kernel: 4 or 8 channels per lane");
    constexpr bool TWO = C == 512;                        // the lane's second slice of 4 channels (w1 / a1)
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long m0 = wave * RPW;
    if (m0 >= M) return;
    const int cch = 2 * h;
    float acc[RPW * 8];                                   // index r * 8 + o
#pragma unroll
    for (int i = 0; i < RPW * 8; ++i) acc[i] = 0.f;
    for (int layer = 0; layer < 8; ++layer) {
        f32x4 w0[8], w1[8], a0[RPW], a1[RPW];
        const float* wl = wfold + ((long long)layer * 8) * C + lane * 4;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            w0[o] = *reinterpret_cast<const f32x4*>(wl + o * C);
            if constexpr (TWO) w1[o] = *reinterpret_cast<const f32x4*>(wl + o * C + C / 2);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const long long m = m0 + r < M ? m0 + r : M - 1;   // clamp: rows past M are computed but never stored
            const float* al = acts + layer * layer_stride + lane * 4;
            a0[r] = *reinterpret_cast<const f32x4*>(al + m * C);
            if constexpr (TWO) a1[r] = *reinterpret_cast<const f32x4*>(al + m * C + C / 2);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                float p = acc[r * 8 + o];
#pragma unroll
                for (int j = 0; j < 4; ++j) p = fmaf(a0[r][j], w0[o][j], p);
                if constexpr (TWO) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) p = fmaf(a1[r][j], w1[o][j], p);
                }
                acc[r * 8 + o] = p;
            }
    }
    // 64 values over 64 lanes: after masks 32..1 lane l holds the full sum of index l = r * 8 + o
#pragma unroll
    for (int half = RPW * 4, msk = 32; half >= 1; half >>= 1, msk >>= 1) {
        const bool hi = (lane & msk) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            float a_lo = acc[i], a_hi = acc[i + half];
            asm volatile("" : "+v"(a_lo), "+v"(a_hi));     // opaque copies (see wn_end_fold_kernel)
            const float send = hi ? a_lo : a_hi;
            const float keep = hi ? a_hi : a_lo;
            acc[i] = keep + __shfl_xor(send, msk, 64);
        }
    }
    const float mine = acc[0] + bfold[lane & 7];
    // lanes 8r .. 8r+7 hold out[r][0..7]; lane 8r finishes position m0 + r
    float out[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) out[o] = __shfl(mine, (lane & ~7) + o, 64);
    const long long m = m0 + (lane >> 3);
    const int ph = (int)(m / PR), fr = (int)(m % PR);          // phase-major row -> (phase, frame)
    const long long mnat = (long long)fr * NPH + ph;           // natural position index b * L + t * 32 + p
    if ((lane & 7) != 0 || m >= M || fr >= BT) return;
    const int n = cch - n_early;                               // channels that stay (next != null)
    float* zrow = z + mnat * 8;
    if constexpr (MASK != MASK_NONE) {
        if (!frame_is_real(lens, fr, T)) {
            slog[m] = 0.f;
            if (next) {
                for (int j = 0; j < n_early; ++j) zrow[zoff + j] = 0.f;
                for (int c = 0; c < n; ++c) state[m * 8 + c] = 0.f;
            } else {
                for (int c = 0; c < cch; ++c) zrow[c] = 0.f;
            }
            return;
        }
    }
    float y[8];
    float ssum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float a = j < cch ? state[m * 8 + j] : 0.f;
        if (j < h) y[j] = a;
        else if (j < cch) {
            y[j] = fmaf(expf(out[j]), a, out[j - h]);
            ssum += out[j];
        } else y[j] = 0.f;
    }
    slog[m] = first ? ssum : slog[m] + ssum;
    if (!next) {
        for (int c = 0; c < cch; ++c) zrow[c] = y[c];
        return;
    }
    for (int j = 0; j < n_early; ++j) zrow[zoff + j] = y[j];
    float res[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float t = 0.f;
        if (c < n) {
            for (int j = 0; j < n; ++j) t = fmaf(y[n_early + j], next[j * n + c], t);
        }
        res[c] = t;
    }
    for (int c = 0; c < n; ++c) state[m * 8 + c] = res[c];
}

// Row statistics, first pass: block (chunk, b) sums z^2 (all 8 channels) and slog over its share of row b's real positions
// i = 32 t + p < lens[b] * 32 (lens null: T * 32), in float64: thread tid takes positions lo + tid, lo + tid + 256, ..., then a
// shared-memory tree.  part[(b * STAT_CHUNKS + chunk) * 2 + {0, 1}].
__global__ __launch_bounds__(256) void encode_stats_partial_kernel(const float* __restrict__ z, const float* __restrict__ slog,
                                                                   const int* __restrict__ lens, int T, int PR,
                                                                   double* __restrict__ part) {
    __shared__ double sm[2][256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const long long n_pos = (long long)(lens ? lens[b] : T) * NPH;
    const long long per = (n_pos + STAT_CHUNKS - 1) / STAT_CHUNKS;
    const long long lo = chunk * per, hi = lo + per < n_pos ? lo + per : n_pos;
    double s2 = 0.0, ss = 0.0;
    for (long long i = lo + tid; i < hi; i += 256) {
        const float* zr = z + ((long long)b * T * NPH + i) * 8;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(zr), v1 = *reinterpret_cast<const f32x4*>(zr + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) s2 += (double)v0[j] * (double)v0[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) s2 += (double)v1[j] * (double)v1[j];
        ss += (double)slog[(i % NPH) * PR + (long long)b * T + i / NPH];
    }
    sm[0][tid] = s2;
    sm[1][tid] = ss;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) {
            sm[0][tid] += sm[0][tid + w];
            sm[1][tid] += sm[1][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[((long long)b * STAT_CHUNKS + chunk) * 2] = sm[0][0];
        part[((long long)b * STAT_CHUNKS + chunk) * 2 + 1] = sm[1][0];
    }
}
// second pass: one thread per row adds its chunks in order; stats [3][B] = sum z^2 | sum s | lens[b] * 32 * log_det_sum
__global__ void encode_stats_final_kernel(const double* __restrict__ part, const int* __restrict__ lens, int T, int B,
                                          double log_det_sum, float* __restrict__ stats) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s2 = 0.0, ss = 0.0;
    for (int c = 0; c < STAT_CHUNKS; ++c) {
        s2 += part[((long long)b * STAT_CHUNKS + c) * 2];
        ss += part[((long long)b * STAT_CHUNKS + c) * 2 + 1];
    }
    stats[b] = (float)s2;
    stats[B + b] = (float)ss;
    stats[2 * B + b] = (float)((double)((long long)(lens ? lens[b] : T) * NPH) * log_det_sum);
}

}  // namespace

int wg_encode_init(tts_hip_engine* e, const float* d_audio, const float* fwd0, float* state, int PR, int BT, const int* d_lens, int T) {
    const long long M = (long long)NPH * PR;
    const dim3 grid((unsigned)((M + 255) / 256));
    if (d_lens)
        hipLaunchKernelGGL(encode_init_kernel<MASK_LENS>, grid, dim3(256), 0, e->stream, d_audio, fwd0, state, PR, BT, d_lens, T);
    else
        hipLaunchKernelGGL(encode_init_kernel<MASK_NONE>, grid, dim3(256), 0, e->stream, d_audio, fwd0, state, PR, BT,
                           (const int*)nullptr, 1);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

int wg_encode_end(tts_hip_engine* e, const WgEncodeEnd& a) {
    const long long waves = (a.M + RPW - 1) / RPW;
    const dim3 grid((unsigned)((waves + 3) / 4));
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, e->stream, a.acts, a.layer_stride, a.wfold, a.bfold, a.state, a.slog, a.first,
                           a.next, a.z, a.zoff, a.n_early, a.M, a.h, a.PR, a.BT, a.d_lens, a.d_lens ? a.T : 1);
    };
    if (a.C == 256) {
        if (a.d_lens) launch(wn_end_fwd_kernel<MASK_LENS, 256>);
        else launch(wn_end_fwd_kernel<MASK_NONE, 256>);
    } else {
        if (a.d_lens) launch(wn_end_fwd_kernel<MASK_LENS, 512>);
        else launch(wn_end_fwd_kernel<MASK_NONE, 512>);
    }
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

size_t wg_encode_stats_bytes(int B) { return (size_t)B * STAT_CHUNKS * 2 * sizeof(double); }

int wg_encode_stats(tts_hip_engine* e, const float* d_z, const float* slog, double* part, const int* d_lens, int B, int T, int PR,
                    double log_det_sum, float* d_stats) {
    hipLaunchKernelGGL(encode_stats_partial_kernel, dim3(STAT_CHUNKS, (unsigned)B), dim3(256), 0, e->stream, d_z, slog, d_lens, T,
                       PR, part);
    hipLaunchKernelGGL(encode_stats_final_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, e->stream,
                       (const double*)part, d_lens, T, B, log_det_sum, d_stats);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}
