// waveglow.hip -- WaveGlow flow inversion on gfx950.
//
// Replaces /root/reference/architectures/waveglow_arch.py:244-306 (WaveGlow.infer), :105-141 (WaveglowBlock.call) and
// architectures/layers/invertible_conv.py:41-51 (Invertible1x1Conv reverse).
//
// HBM layout (all float32, channels-last).  Positions are kept PHASE-MAJOR inside the engine: a position is a group of
// 8 samples, l = 32 * t + p (t = mel frame, p = phase 0..31); row m' = p * PR + f with f = b * T + t the global frame
// index and PR = B*T rounded up to the 256-row tile.  A conv tap l +- d then stays a constant row shift per tile
// (phase' = (p +- d) mod 32, frame carry = floor((p +- d) / 32)) and the phase is uniform per tile, which is what the
// low-rank conditioning below needs.  M' = 32 * PR rows:
// C = n_channels of the handle's model, 512 or 256 (WaveGlowDev::channels, read from the tensors at finalize); the widths
// spelled as numbers in the comments below are those of the 512-channel model.
//   x     [M'][C]     WN residual stream, updated in place by the residual GEMM epilogue
//   acts  [8][M'][C]  gated activations tanh * sigmoid of the 8 layers of the current flow (in-layer GEMM epilogue)
//   a0p   [M'][16]    [audio_0 | 1 | 0..]: operand of the first layer of a flow (start conv composed into its taps)
//   audio [M'][8]     current flow state in the first n_rem columns; the last flow writes the caller's [B][L*8] directly
//   endp  [7][M'][8]  fp32, 512 channels: acts_i @ wfold_i for layers i = 0 .. 6, second output of the layer's residual GEMM
// Per flow: start (VALU) -> 8 x { in-layer implicit GEMM (K = 3 taps * 512 + 4 * 80 mel, N = 1024, gate epilogue),
// residual GEMM (K = 512, N = 512; not for the last layer) } -> folded skip/end + affine inverse + inverse 1x1 conv.
//
// Conditioning folding (exact algebra, load time): the reference upsamples the mel with a transposed conv
// (k 1024, stride 256), regroups 8 samples x 80 channels into 640 channels and applies a 640 -> 1024 1x1 conv per layer
// (waveglow_arch.py:245-253,125).  A group at phase p only sees mel frames t-3..t, so
//     cond_i[l] = V_{i,p} @ [mel[t], mel[t-1], mel[t-2], mel[t-3]] + const,   V_{i,p} = W_cond_i @ U_p  (1024 x 320),
// i.e. K = 320 instead of 640 (-14.7 % of the in-layer FLOPs), no upsampling pass and no [M][640] spectrogram in HBM.
// The price is 32 per-phase copies of the conditioning weights (42 MB per layer, 4 GB in all), streamed once per launch.
//
// Skip path folding (exact algebra, done once at load time): the reference sums the skip halves of the 8 res_skip convs
// and feeds the sum to the `end` 1x1 conv (waveglow_arch.py:129-141).  Both are linear, so
//     end(sum_i skip_i) = sum_i acts_i @ (W_skip_i @ W_end) + (sum_i b_skip_i) @ W_end + b_end .
// The 512 -> 512 skip GEMMs (and the whole res_skip conv of the last layer) disappear -- 9.6 % of the WN FLOPs and the
// read-modify-write of a [M][512] skip buffer per layer -- and are replaced by one [M, 8*512] x [8*512, 2h] product per
// flow (h <= 4), computed by the HBM-bound wn_end_fold_kernel straight from the stored activations -- in the fp16 modes and for
// 256-channel models.  The fp32 path of a 512-channel model never re-reads them: the residual GEMM of layer i, which streams
// acts_i as its A operand, also stores the layer's eight partial sums to endp[i] (gemm_f32.h, GemmArgs::end_sums), and
// wn_end_last_kernel adds the seven slots, layer 7's product (the one layer without a residual GEMM) and the bias.
//
// fp32 calls of 144 frames or more take the Winograd form (wn_wino.hip) instead of the in-layer GEMMs above: layers 1 .. 7 as
// F(4,3) along the taps behind a frame-axis F(4,4) conditioning plane, the first layer of a flow on that plane kernel's K loop.
// That form is built on N = 1024 planes: a 256-channel model always takes the direct form.
//
// Width: the GEMMs take N, K and every stride as run-time values; the VALU kernels of this file whose indexing is built on
// the width are templates on C, instantiated for 512 and 256 and chosen per call by for_width().  Nothing at file scope
// depends on a handle's width, so handles of both widths live side by side.
//
// Host side, in file order: waveglow_free; the load-time algebra above as three host functions and waveglow_finalize, which
// uploads their results; waveglow_build_half (fp16 operands of either fp16 mode, on first use); the pieces of waveglow_run --
// the kWnKernels table (precision x tile family of wg_plan.h -> GEMM launchers), ensure_workspace, wn_call / in_layer_args /
// res_args (one description of the operands for every precision), launch_end_fold, the probe hooks, the Winograd form's
// out-of-memory fallback, wn_flow (the WN block of one flow: the one layer loop for every precision, form, mask kind and
// direction) -- and waveglow_run itself, then waveglow_encode_run: the forward flow (audio -> z, flows ascending) around the same
// wn_flow, with the position-wise kernels of wg_encode.hip.
#include "engine.h"
#include "gemm_f32.h"
#include "wg_plan.h"

#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <utility>

using namespace ttsgemm;

namespace {

constexpr int NCOND = 640;    // n_mel * n_group (reference layout of the conditioning input)
constexpr int KCONV0 = 3 * 16;// first layer of a flow: taps act on [audio_0 | 1] (16-float rows)
constexpr int KMEL = 4 * 80;  // folded conditioning: 4 mel frames x 80 channels
constexpr int NPH = 32;       // phases (sample groups per mel frame)

// dst[n][koff + k] = src[k * src_ld + perm(n)]  for k < K   (Keras [K][N] kernel slice -> Bt rows)
// perm: 0 identity; 1 WN gate interleave (per group of 64 rows: 32 tanh channels then their 32 sigmoid partners, so a
//       wave's pair of adjacent 32-column MFMA tiles holds matching pre-activations for every N tile >= 64 columns)
// taps > 1: src is [taps][K/taps][N] and the K axis of dst is tap-interleaved in chunks of `bk`:
//   dst k = (c / bk) * taps * bk + tap * bk + c % bk     (matches gemm_f32_kernel's NI = taps tile order)
template <int C>
__global__ void pack_bt_kernel(const float* __restrict__ src, int K, int src_ld, float* __restrict__ dst, int N,
                               long long ldb, int koff, int perm, int taps, int bk) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)N * K) return;
    const int n = (int)(idx / K), k = (int)(idx % K);
    int kd = k;
    if (taps > 1) {
        const int cpt = K / taps, tap = k / cpt, c = k % cpt;
        kd = (c / bk) * taps * bk + tap * bk + c % bk;
    }
    int sn = n;
    if (perm == 1) {
        const int grp = n >> 6, q = n & 63;
        sn = q < 32 ? grp * 32 + q : C + grp * 32 + (q - 32);
    }
    dst[(long long)n * ldb + koff + kd] = src[(long long)k * src_ld + sn];
}

template <int C>
__global__ void pack_bias_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dst,
                                 int N, int perm) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int sn = n;
    if (perm == 1) {
        const int grp = n >> 6, q = n & 63;
        sn = q < 32 ? grp * 32 + q : C + grp * 32 + (q - 32);
    }
    dst[n] = a[sn] + (b ? b[sn] : 0.f);
}

// Transposed-conv kernel [1024][80 out][80 in] -> UT[p][q*80 + j][c*8 + g] = W[(p*8 + g) + 256 q][c][j]
// (the "Bt" operand of V_{i,p} = WcT_i @ U_p: row = mel-window input (q, j), K = regrouped channel c*8 + g)
__global__ void pack_ut_kernel(const float* __restrict__ w, float* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)NPH * KMEL * NCOND;
    if (idx >= total) return;
    const int k = (int)(idx % NCOND);
    const int r = (int)((idx / NCOND) % KMEL);
    const int p = (int)(idx / ((long long)NCOND * KMEL));
    const int c = k >> 3, gidx = k & 7, q = r / 80, j = r % 80;
    dst[idx] = w[((long long)(p * 8 + gidx + 256 * q) * 80 + c) * 80 + j];
}

// bias[n] += sum_k WcT[n][k] * b_up[k >> 3]     (upsampling bias pushed through the conditioning conv)
template <int C>
__global__ void cond_bias_kernel(const float* __restrict__ wct, const float* __restrict__ b_up, float* __restrict__ bias) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= 2 * C) return;
    float acc = 0.f;
    for (int k = 0; k < NCOND; ++k) acc = fmaf(wct[(long long)n * NCOND + k], b_up[k >> 3], acc);
    bias[n] += acc;
}

// ---- fp16 operand builders (run once, on first use of the fp16 path, from the packed fp32 device copies)
// `lo` (may be null) receives the second plane of the split-fp16 mode: lo = fp16(v - fp16(v))
__device__ __forceinline__ void put_split(_Float16* dst, _Float16* lo, long long i, float v) {
    const _Float16 hv = (_Float16)v;
    dst[i] = hv;
    if (lo) lo[i] = (_Float16)(v - (float)hv);
}
__global__ void cvt_half_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, long long n,
                                _Float16* __restrict__ lo = nullptr) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) put_split(dst, lo, i, src[i]);
}
// in-layer taps: fp32 [1024][1536] tap-interleaved in chunks of 16 -> fp16 [1024][1536] tap-interleaved in chunks of 32
// (the fp16 kernel's K step is 32 halfs = 64-byte LDS rows, like 16 floats)
template <int C>
__global__ void cvt_taps_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, _Float16* __restrict__ lo = nullptr) {
    constexpr int KCONV = 3 * C;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)2 * C * KCONV) return;
    const int n = (int)(i / KCONV), r = (int)(i % KCONV);
    const int tap = r / C, c = r % C;
    const int ks = (c / 16) * 48 + tap * 16 + c % 16, kd = (c / 32) * 96 + tap * 32 + c % 32;
    put_split(dst, lo, (long long)n * KCONV + kd, src[(long long)n * KCONV + ks]);
}
// first layer of a flow: fp32 [1024][3*16] -> fp16 [1024][3*32] (a0p rows are 32 halfs)
template <int C>
__global__ void cvt_taps0_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, _Float16* __restrict__ lo = nullptr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * C * 96) return;
    const int n = i / 96, r = i % 96, tap = r / 32, jj = r % 32;
    put_split(dst, lo, i, jj < 16 ? src[n * KCONV0 + tap * 16 + jj] : 0.f);
}

// fp16 modes: the conditioning operand of frame f is the contiguous window [mel_t | mel_{t-1} | mel_{t-2} | mel_{t-3}]
// (320 halfs = 10 K steps; four separate 80-wide segments would each be padded to 96 = 12 steps), zeros before the start
// of the utterance.  `lo` (may be null) receives the second plane of the split mode.
__global__ void mel_window_kernel(const float* __restrict__ mel, _Float16* __restrict__ dst, _Float16* __restrict__ lo,
                                  int BT, int T) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)BT * KMEL) return;
    const int f = (int)(i / KMEL), r = (int)(i % KMEL), q = r / 80, j = r % 80;
    const int t = f % T;
    put_split(dst, lo, i, t - q >= 0 ? mel[(long long)(f - q) * 80 + j] : 0.f);
}

// test hook (tts_hip_waveglow_probe): phase-major rows m' = p * PR + b * T + t of one layer's gated activations (W = C) or
// conditioning plane (W = 1024; Winograd form, 512 channels only) -> natural order [B][T * 32][W] (position l = 32 t + p)
__global__ void probe_acts_kernel(const float* __restrict__ acts, float* __restrict__ out, int PR, int BT, int T, int W) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // one float4 of one position
    if (idx >= (long long)BT * NPH * (W / 4)) return;
    const int c = (int)(idx % (W / 4)) * 4;
    const long long pos = idx / (W / 4);               // b * T * 32 + l
    const int p = (int)(pos % NPH);
    const long long f = pos / NPH;                     // b * T + t
    *reinterpret_cast<f32x4*>(out + pos * W + c) = *reinterpret_cast<const f32x4*>(acts + ((long long)p * PR + f) * W + c);
}
// the same for the fp16 activation planes, widened to fp32; `lo` (split-fp16 mode, may be null): value = hi + lo
template <int C>
__global__ void probe_acts16_kernel(const _Float16* __restrict__ acts, const _Float16* __restrict__ lo, float* __restrict__ out,
                                    int PR, int BT, int T) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)BT * NPH * (C / 4)) return;
    const int c = (int)(idx % (C / 4)) * 4;
    const long long pos = idx / (C / 4);
    const int p = (int)(pos % NPH);
    const long long src = ((long long)p * PR + pos / NPH) * C + c;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)acts[src + j] + (lo ? (float)lo[src + j] : 0.f);
    *reinterpret_cast<f32x4*>(out + pos * C + c) = v;
}
// test hook: the flow state after one flow ([M'][8] phase-major, or [BT * 32][8] natural after flow 0) -> [B][T * 32][n];
// pitch: floats between two rows of the source (8: the flow state and z; 1: the forward direction's per-position sums)
__global__ void probe_state_kernel(const float* __restrict__ audio, int natural, float* __restrict__ out, int n, int PR, int BT,
                                   int pitch) {
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= (long long)BT * NPH) return;
    const long long row = natural ? pos : (pos % NPH) * PR + pos / NPH;
    for (int j = 0; j < n; ++j) out[pos * n + j] = audio[row * pitch + j];
}

// Ragged calls (tts_hip_waveglow_infer_ragged): row b = f / T holds lens[b] real frames; frame f is real when f % T < lens[b]
__device__ __forceinline__ bool frame_is_real(const int* __restrict__ lens, int f, int T) { return f % T < lens[f / T]; }
// Which frames of a call are real (MASK template argument of the kernels below): every frame, the first lens[b] of each row
// (ragged calls), or those with a non-zero entry in a per-frame flag array (packed calls: the `lens` argument then IS that
// array, one int per frame of the packed row, 0 on gap frames)
enum { MASK_NONE = 0, MASK_LENS = 1, MASK_FLAGS = 2 };
template <int MASK>
__device__ __forceinline__ bool frame_masked_real(const int* __restrict__ info, int f, int T) {
    if constexpr (MASK == MASK_FLAGS) return info[f] != 0;
    else return frame_is_real(info, f, T);
}

// audio[m'][0..3] = sigma * z[natural m][0..3]  (z null => zeros); m' = p * PR + f  <->  m = f * 32 + p
// MASK != MASK_NONE: frames that are not real start at 0 whatever z holds there (it is not read)
template <int MASK = MASK_NONE>
__global__ void init_audio_kernel(const float* __restrict__ z, float sigma, float* __restrict__ audio, int PR, int BT,
                                  const int* __restrict__ lens = nullptr, int T = 1) {
    const long long mp = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (mp >= (long long)NPH * PR) return;
    const int p = (int)(mp / PR), f = (int)(mp % PR);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    bool real = z && f < BT;
    if constexpr (MASK != MASK_NONE) real = real && frame_masked_real<MASK>(lens, f, T);
    if (real) {
        v = *reinterpret_cast<const f32x4*>(z + ((long long)f * NPH + p) * 8);
        v *= sigma;
    }
    *reinterpret_cast<f32x4*>(audio + mp * 8) = v;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(audio + mp * 8 + 4) = zero;
}

// Ragged calls: private copy of the mel with every frame beyond its row's length cleared.  Every later reader (the direct
// form's conditioning segments, the Winograd mel planes, the fp16 mel windows) takes this copy, so no caller tail value --
// NaN included -- enters a kernel that combines neighbouring frames.  One float4 per thread; tail frames are not read.
__global__ void mel_ragged_copy_kernel(const float* __restrict__ mel, float* __restrict__ dst, const int* __restrict__ lens,
                                       int BT, int T) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)BT * 20) return;
    const int f = (int)(i / 20);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (frame_is_real(lens, f, T)) v = *reinterpret_cast<const f32x4*>(mel + i * 4);
    *reinterpret_cast<f32x4*>(dst + i * 4) = v;
}

// Ragged calls: stores 0 over the rows of the residual stream that lie beyond their utterance's length -- after the start
// conv (then also the a0p rows, constant-1 column included: a tail row must look like the zero padding a run of the row
// alone has there) and after every residual GEMM.  `tail` lists the n_tail frames f = b * T + t with t >= lens[b]; their
// 32 phase rows are p * PR + f.  One float4 of one row per thread: only tail bytes are touched.
// x16 (fp16 modes, else null): the shadow of x, `planes` planes M * C halfs apart; a0p (null after a residual GEMM):
// 16 floats per row, or `planes` planes of 32 halfs per row when x16 is given.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <int C>
__global__ void wn_zero_tail_kernel(const int* __restrict__ tail, int n_tail, int PR, long long M, float* __restrict__ x,
                                    _Float16* __restrict__ x16, int planes, void* __restrict__ a0p) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = idx / (C / 4);
    if (r >= (long long)NPH * n_tail) return;
    const int c = (int)(idx % (C / 4)) * 4;
    const long long m = (r / n_tail) * PR + tail[r % n_tail];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f16x4 zeroh = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    *reinterpret_cast<f32x4*>(x + m * C + c) = zero;
    if (x16)
        for (int pl = 0; pl < planes; ++pl) *reinterpret_cast<f16x4*>(x16 + pl * M * C + m * C + c) = zeroh;
    if (a0p) {
        if (x16) {
            if (c < 32)
                for (int pl = 0; pl < planes; ++pl) *reinterpret_cast<f16x4*>((_Float16*)a0p + pl * M * 32 + m * 32 + c) = zeroh;
        } else if (c < 16) {
            *reinterpret_cast<f32x4*>((float*)a0p + m * 16 + c) = zero;
        }
    }
}

// Packed calls (tts_hip_waveglow_infer_packed): the real frames of all rows laid one after another in ONE row of F frames,
// TTS_HIP_WG_GAP_FRAMES zero frames between two rows.  flags[f] = 1 + (b * T + t) for the packed frame f that holds frame t
// of row b, 0 for a gap frame: "is real" for the kernels above and the source index of the gather in one int.
// Gather: dst[f][..] = src[flags[f] - 1][..] (q4 float4 per frame: 20 for the mel, 64 for z), 0 on gap frames.  One float4
// per thread, consecutive threads take consecutive float4 of both sides; caller frames beyond a row's length are not read.
__global__ void packed_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ flags,
                                     int F, int q4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * q4) return;
    const int f = (int)(i / q4), r = (int)(i % q4);
    const int s = flags[f];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (s) v = *reinterpret_cast<const f32x4*>(src + ((long long)(s - 1) * q4 + r) * 4);
    *reinterpret_cast<f32x4*>(dst + i * 4) = v;
}
// Scatter: audio[b][t * 256 ..] = packed[(start[b] + t) * 256 ..] for t < len[b], 0 behind it -- every float of the caller's
// [B][T * 256] is written once, so the output needs no clear.  seg = [start[B] | len[B]]; 64 float4 per frame.
__global__ void packed_scatter_kernel(const float* __restrict__ packed, const int* __restrict__ seg, float* __restrict__ audio,
                                      int B, int T) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * T * 64) return;
    const int r = (int)(i % 64);
    const long long fr = i / 64;
    const int b = (int)(fr / T), t = (int)(fr % T);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t < seg[B + b]) v = *reinterpret_cast<const f32x4*>(packed + ((long long)(seg[b] + t) * 64 + r) * 4);
    *reinterpret_cast<f32x4*>(audio + i * 4) = v;
}

// x[m][c] = sum_{j < h} audio[m][j] * w[j][c] + b[c]      (start 1x1 conv, waveglow_arch.py:108)
// Also writes a0p[m][..] = [audio_0 (h values) | 1 | 0 ...]: the operand of the first WN layer, whose dilated conv is
// composed with the start conv at load time (the constant 1 carries the start bias through the zero padding).
// HALF: x stays fp32 (master copy for the residual accumulation) and additionally gets an fp16 shadow x16 (the GEMM
// operand); a0p is written as 32 halfs per row.
template <int C, bool HALF>
__global__ void wn_start_kernel(const float* __restrict__ audio, const float* __restrict__ w,
                                const float* __restrict__ b, float* __restrict__ x, void* __restrict__ a0p_v,
                                _Float16* __restrict__ x16, long long M, int h, int split = 0) {
    // split != 0 (split-fp16 mode): the fp16 arrays are [2 planes][M][..]; plane 1 gets v - fp16(v)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one float4 of channels
    if (idx >= M * (C / 4)) return;
    const long long m = idx / (C / 4);
    const int c = (int)(idx % (C / 4)) * 4;
    if (c < (HALF ? 32 : 16)) {                         // the first threads of the row also write the a0p row
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = c + j;
            v[j] = col < h ? audio[m * 8 + col] : (col == h ? 1.f : 0.f);
        }
        if constexpr (HALF) {
            const f16x4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            *reinterpret_cast<f16x4*>((_Float16*)a0p_v + m * 32 + c) = hv;
            if (split) {
                const f16x4 lv = {(_Float16)(v[0] - (float)hv[0]), (_Float16)(v[1] - (float)hv[1]),
                                  (_Float16)(v[2] - (float)hv[2]), (_Float16)(v[3] - (float)hv[3])};
                *reinterpret_cast<f16x4*>((_Float16*)a0p_v + M * 32 + m * 32 + c) = lv;
            }
        } else {
            const f32x4 fv = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>((float*)a0p_v + m * 16 + c) = fv;
        }
    }
    f32x4 acc = *reinterpret_cast<const f32x4*>(b + c);
    // the reference accumulates the dot product first and adds the bias last (Conv1D = conv + bias)
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < h; ++j) {
        const float a = audio[m * 8 + j];
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + j * C + c);
        s += a * wv;
    }
    acc += s;
    *reinterpret_cast<f32x4*>(x + m * C + c) = acc;
    if constexpr (HALF) {
        const f16x4 hv = {(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
        *reinterpret_cast<f16x4*>(x16 + m * C + c) = hv;
        if (split) {
            const f16x4 lv = {(_Float16)(acc[0] - (float)hv[0]), (_Float16)(acc[1] - (float)hv[1]),
                              (_Float16)(acc[2] - (float)hv[2]), (_Float16)(acc[3] - (float)hv[3])};
            *reinterpret_cast<f16x4*>(x16 + M * C + m * C + c) = lv;
        }
    }
}

// Folded skip/end conv + affine inverse + inverse 1x1 conv (+ early-z prepend), RPW positions per wave.
//   out[m][o] = sum_layer sum_c acts[layer][m][c] * wfold[layer][o][c] + bfold[o]          (waveglow_arch.py:129-141)
//   audio_1 = (audio_1 - b) / exp(s); audio = [audio_0, audio_1] @ inv; prepend sigma * z_early   (:284-304)
// C = 512: lane l owns channels 4l..4l+3 and 256+4l..256+4l+3 (every wave-level load is one contiguous 1 KiB run); per layer
// the lane's 8x8 slice of wfold sits in registers and is reused for the RPW rows; the RPW*8 partial sums are reduced with the lane-halving exchange (63 shuffles for 64 values).
// C = 256: a wave still owns RPW whole rows and a lane owns 4 channels of each, 4l..4l+3 (fp32: one float4, the wave-level
// load is the whole 1 KiB row; fp16 modes: 4 halfs, one 8-byte load per plane), i.e. the second slice (w1 / a1) is absent.
// The other choice, two rows per wave, would keep 16-byte fp16 loads but needs a second reduction tree (32 lanes per row,
// 128 values per wave), another row-to-lane map for the masked epilogue and twice the accumulators per lane.  The kernel
// streams 8 x M x C activations once and is bound by that stream at either width; with one row per wave the reduction,
// the three MASK modes and the early-z prepend below are the very same code as at 512.
constexpr int RPW = 8;
// MASK != MASK_NONE: positions of frames that are not real (beyond their row's length; gap frames of a packed call) store
// 0 -- the flow state stays 0 there from flow to flow and the last flow gives the zero tail of the output -- and z is not
// read there.
template <bool HALF, bool SPLIT = false, int MASK = MASK_NONE, int C = 512>
__global__ __launch_bounds__(256) void wn_end_fold_kernel(const void* __restrict__ acts_v, long long layer_stride,
                                                          const float* __restrict__ wfold,
                                                          const float* __restrict__ bfold,
                                                          const float* __restrict__ inv, float* __restrict__ audio_io,
                                                          float* __restrict__ audio_out, int out_natural,
                                                          const float* __restrict__ z, int zoff, int n_early,
                                                          float sigma, long long M, int h, int PR, int BT,
                                                          long long lo_plane = 0,
                                                          const int* __restrict__ lens = nullptr, int T = 1) {
    // lo_plane != 0 (split-fp16 mode): activation = hi + lo, lo at + lo_plane halfs
    static_assert(C == 512 || C == 256, "wn_end_fold_kernel: 4 or 8 channels per lane");
    constexpr bool TWO = C == 512;                        // the lane's second slice of 4 channels (w1 / a1)
    constexpr int WQ = 8 * C / 4 / 256;                   // float4 per thread of a layer's folded weights [8][C]
    // fp16 variants: the folded weights of a layer ([8 outputs][C]: 16 KB at 512, the same for every wave) are staged in LDS once
    // per block and layer (double buffered; the next layer's rows are requested before this layer's arithmetic).  With
    // 8 consecutive channels per lane a lane's two weight float4 sit 32 B apart, and pulling those slices through the L1
    // per wave cost more than the halved activation stream saved (fp16 0.68 -> 0.42 ms, split 1.14 -> 0.90 ms).
    __shared__ __attribute__((aligned(16))) float wsm[HALF ? 2 : 1][HALF ? 8 * C : 4];
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long m0 = wave * RPW;
    const bool wave_valid = m0 < M;                       // (M is a multiple of 4 * RPW; with barriers in the fp16 variants
    if (!HALF && !wave_valid) return;                     //  nobody may leave early)
    const int cch = 2 * h;
    float acc[RPW * 8];                                   // index r * 8 + o
#pragma unroll
    for (int i = 0; i < RPW * 8; ++i) acc[i] = 0.f;
    if constexpr (HALF) {
        const f32x4* src = reinterpret_cast<const f32x4*>(wfold);
#pragma unroll
        for (int i = 0; i < WQ; ++i) reinterpret_cast<f32x4*>(wsm[0])[threadIdx.x + i * 256] = src[threadIdx.x + i * 256];
        __syncthreads();
    }
    for (int layer = 0; layer < 8; ++layer) {
        f32x4 w0[8], w1[8], a0[RPW], a1[RPW], wnext[HALF ? WQ : 1];
        if constexpr (HALF) {
            if (layer + 1 < 8) {
                const f32x4* src = reinterpret_cast<const f32x4*>(wfold + (long long)(layer + 1) * 8 * C);
#pragma unroll
                for (int i = 0; i < WQ; ++i) wnext[i] = src[threadIdx.x + i * 256];
            }
        }
        // fp32 activations: lane owns channels 4l..4l+3 and 256+4l..; fp16 activations: channels 8l..8l+7, so that one
        // 16-byte load per plane and row fetches them (C = 256: channels 4l..4l+3 in every precision)
        constexpr int CPL = C / 64;                       // channels per lane
        const float* wl = HALF ? wsm[layer & 1] + lane * CPL : wfold + ((long long)layer * 8) * C + lane * 4;
        constexpr int W1 = HALF ? 4 : C / 2;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            w0[o] = *reinterpret_cast<const f32x4*>(wl + o * C);
            if constexpr (TWO) w1[o] = *reinterpret_cast<const f32x4*>(wl + o * C + W1);
        }
        if constexpr (HALF) {
            // all loads of the layer first (a run-time test of `lo_plane` between them made the compiler wait for every
            // load before issuing the next: 1.9 ms instead of 0.6 ms), conversions afterwards
            typedef _Float16 f16xNv __attribute__((ext_vector_type(CPL)));
            f16xNv hv[RPW], lv[SPLIT ? RPW : 1];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const long long m = m0 + r < M ? m0 + r : M - 1;   // clamp: tail rows are computed but never stored
                const _Float16* al = (const _Float16*)acts_v + layer * layer_stride + m * C + lane * CPL;
                hv[r] = *reinterpret_cast<const f16xNv*>(al);
                if constexpr (SPLIT) lv[r] = *reinterpret_cast<const f16xNv*>(al + lo_plane);
            }
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                a0[r] = f32x4{(float)hv[r][0], (float)hv[r][1], (float)hv[r][2], (float)hv[r][3]};
                if constexpr (TWO) a1[r] = f32x4{(float)hv[r][4], (float)hv[r][5], (float)hv[r][6], (float)hv[r][7]};
                if constexpr (SPLIT) {
                    a0[r] += f32x4{(float)lv[r][0], (float)lv[r][1], (float)lv[r][2], (float)lv[r][3]};
                    if constexpr (TWO) a1[r] += f32x4{(float)lv[r][4], (float)lv[r][5], (float)lv[r][6], (float)lv[r][7]};
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const long long m = m0 + r < M ? m0 + r : M - 1;   // clamp: tail rows are computed but never stored
                const float* al = (const float*)acts_v + layer * layer_stride + lane * 4;
                a0[r] = *reinterpret_cast<const f32x4*>(al + m * C);
                if constexpr (TWO) a1[r] = *reinterpret_cast<const f32x4*>(al + m * C + C / 2);
            }
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
        if constexpr (HALF) {
            if (layer + 1 < 8) {
#pragma unroll
                for (int i = 0; i < WQ; ++i) reinterpret_cast<f32x4*>(wsm[(layer + 1) & 1])[threadIdx.x + i * 256] = wnext[i];
            }
            __syncthreads();
        }
    }
    if (!wave_valid) return;
    // 64 values over 64 lanes: after masks 32..1 lane l holds the full sum of index l = r * 8 + o
#pragma unroll
    for (int half = RPW * 4, msk = 32; half >= 1; half >>= 1, msk >>= 1) {
        const bool hi = (lane & msk) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            float a_lo = acc[i], a_hi = acc[i + half];
            // opaque copies: otherwise instcombine turns select(load, load) into a dynamically indexed load of the
            // register array, which lowers to a compare/select chain over every element (seen for <7, 8>: 3.3 k extra VALU)
            asm volatile("" : "+v"(a_lo), "+v"(a_hi));
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
    if ((lane & 7) == 0 && m < M && fr < BT) {
        if constexpr (MASK != MASK_NONE) {
            if (!frame_masked_real<MASK>(lens, fr, T)) {
                float* dst = audio_out + (out_natural ? mnat : m) * 8;
                for (int j = 0; j < n_early + cch; ++j) dst[j] = 0.f;
                return;
            }
        }
        float a[8], y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = j < cch ? audio_io[m * 8 + j] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < h) y[j] = a[j];
            else if (j < cch) y[j] = (a[j] - out[j - h]) / expf(out[j]);
            else y[j] = 0.f;
        }
        float res[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float t = 0.f;
            if (c < cch) {
                for (int j = 0; j < cch; ++j) t = fmaf(y[j], inv[j * cch + c], t);
            }
            res[c] = t;
        }
        float* dst = audio_out + (out_natural ? mnat : m) * 8;
        for (int j = 0; j < n_early; ++j) dst[j] = z ? sigma * z[mnat * 8 + zoff + j] : 0.f;
        for (int c = 0; c < cch; ++c) dst[n_early + c] = res[c];
    }
}


// fp32, 512 channels: the same on top of the flow's end partial sums.  endp[layer][m][o], layer < 7, already holds acts[layer][m] .
// wfold[layer][o] -- the residual GEMM of that layer formed it while it streamed those activations (gemm_f32.h,
// GemmArgs::end_sums) -- so this kernel reads the activations of layer 7 only, the one layer without a residual GEMM:
// out = ((endp[0] + .. + endp[6]) + acts7 . wfold7) + bfold, in this order.  Lane and row ownership as above.  Rows that
// store 0 (padding, tails, gap frames) do not read their endp.
template <int MASK>
__global__ __launch_bounds__(256) void wn_end_last_kernel(const float* __restrict__ acts7, const float* __restrict__ wfold7,
                                                          const float* __restrict__ endp, const float* __restrict__ bfold,
                                                          const float* __restrict__ inv, float* __restrict__ audio_io,
                                                          float* __restrict__ audio_out, int out_natural,
                                                          const float* __restrict__ z, int zoff, int n_early, float sigma,
                                                          long long M, int h, int PR, int BT, const int* __restrict__ lens, int T) {
    constexpr int C = 512;
    const int lane = threadIdx.x & 63;
    const long long m0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
    if (m0 >= M) return;
    f32x4 w0[8], w1[8], a0[RPW], a1[RPW];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        w0[o] = *reinterpret_cast<const f32x4*>(wfold7 + o * C + lane * 4);
        w1[o] = *reinterpret_cast<const f32x4*>(wfold7 + o * C + C / 2 + lane * 4);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long long m = m0 + r < M ? m0 + r : M - 1;   // clamp: tail rows are computed but never stored
        a0[r] = *reinterpret_cast<const f32x4*>(acts7 + m * C + lane * 4);
        a1[r] = *reinterpret_cast<const f32x4*>(acts7 + m * C + C / 2 + lane * 4);
    }
    float acc[RPW * 8];                                   // index r * 8 + o
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            float p = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) p = fmaf(a0[r][j], w0[o][j], p);
#pragma unroll
            for (int j = 0; j < 4; ++j) p = fmaf(a1[r][j], w1[o][j], p);
            acc[r * 8 + o] = p;
        }
    // 64 values over 64 lanes, as in wn_end_fold_kernel: afterwards lane l holds the full sum of index l = r * 8 + o
#pragma unroll
    for (int half = RPW * 4, msk = 32; half >= 1; half >>= 1, msk >>= 1) {
        const bool hi = (lane & msk) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            float a_lo = acc[i], a_hi = acc[i + half];
            asm volatile("" : "+v"(a_lo), "+v"(a_hi));
            const float send = hi ? a_lo : a_hi;
            const float keep = hi ? a_hi : a_lo;
            acc[i] = keep + __shfl_xor(send, msk, 64);
        }
    }
    const long long m = m0 + (lane >> 3);
    const int fr = (int)(m % PR);
    bool real = m < M && fr < BT;
    if constexpr (MASK != MASK_NONE) real = real && frame_masked_real<MASK>(lens, fr < BT ? fr : 0, T);
    float part = 0.f;
    if (real) {
        float pl[7];
#pragma unroll
        for (int layer = 0; layer < 7; ++layer) pl[layer] = endp[(layer * M + m) * 8 + (lane & 7)];
        part = pl[0];
#pragma unroll
        for (int layer = 1; layer < 7; ++layer) part += pl[layer];
    }
    const float mine = (part + acc[0]) + bfold[lane & 7];
    float out[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) out[o] = __shfl(mine, (lane & ~7) + o, 64);
    // from here on the text of wn_end_fold_kernel's last part (kept as a copy: sharing it as a function changes the register
    // allocation of the nine instantiations of that kernel, which this path leaves as they are)
    const int cch = 2 * h;
    const int ph = (int)(m / PR);                              // phase-major row -> (phase, frame)
    const long long mnat = (long long)fr * NPH + ph;           // natural position index b * L + t * 32 + p
    if ((lane & 7) == 0 && m < M && fr < BT) {
        if constexpr (MASK != MASK_NONE) {
            if (!frame_masked_real<MASK>(lens, fr, T)) {
                float* dst = audio_out + (out_natural ? mnat : m) * 8;
                for (int j = 0; j < n_early + cch; ++j) dst[j] = 0.f;
                return;
            }
        }
        float a[8], y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = j < cch ? audio_io[m * 8 + j] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < h) y[j] = a[j];
            else if (j < cch) y[j] = (a[j] - out[j - h]) / expf(out[j]);
            else y[j] = 0.f;
        }
        float res[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float t = 0.f;
            if (c < cch) {
                for (int j = 0; j < cch; ++j) t = fmaf(y[j], inv[j * cch + c], t);
            }
            res[c] = t;
        }
        float* dst = audio_out + (out_natural ? mnat : m) * 8;
        for (int j = 0; j < n_early; ++j) dst[j] = z ? sigma * z[mnat * 8 + zoff + j] : 0.f;
        for (int c = 0; c < cch; ++c) dst[n_early + c] = res[c];
    }
}


// f(std::integral_constant<int, C>) for a handle's width: the one place that maps the run-time width to the <C> instantiations
// of the kernels above (finalize admits no other width)
template <class F>
void for_width(int C, F f) {
    if (C == 256) f(std::integral_constant<int, 256>{});
    else f(std::integral_constant<int, 512>{});
}

int pack_bt(tts_hip_engine* e, int C, const float* d_src, int K, int src_ld, float* dst, int N, long long ldb, int koff,
            int perm, int taps = 1, int bk = 0) {
    const long long total = (long long)N * K;
    for_width(C, [&](auto cc) {
        hipLaunchKernelGGL(pack_bt_kernel<decltype(cc)::value>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream,
                           d_src, K, src_ld, dst, N, ldb, koff, perm, taps, bk);
    });
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

}  // namespace

void waveglow_free(tts_hip_engine* e) {
    WaveGlowDev& wg = e->wg;
    for (void* p : wg.allocs) (void)hipFree(p);
    wg.allocs.clear();
    wg.for_each_buf([](DevBuf& b) { b.release(); });
    wg.wino_ready = false;
    wg.f16_ready = false;
    wg.x3_ready = false;
    wg.ready = false;
    wg.channels = 0;
}

// ---- load-time algebra of waveglow_finalize: host arithmetic in double, no HIP calls
namespace {

// Start conv composed into the first layer's taps (waveglow_arch.py:108).  w_in [3 taps][C][2 C], ws [h][C], bs [C]
// -> [3 taps][16][2 C] for pack_bt: rows j < h: sum_c ws[j][c] * w_in[tap][c][n]; row h: sum_c bs[c] * w_in[tap][c][n];
// rows > h: 0.
std::vector<float> compose_start_taps(int C, const float* w_in, const float* ws, const float* bs, int h) {
    std::vector<float> comp((size_t)3 * 16 * 2 * C, 0.f);
    std::vector<double> rowacc(2 * C);
    for (int tap = 0; tap < 3; ++tap)
        for (int j = 0; j <= h; ++j) {
            for (int n = 0; n < 2 * C; ++n) rowacc[n] = 0.0;
            for (int c = 0; c < C; ++c) {
                const double sv = j < h ? (double)ws[(size_t)j * C + c] : (double)bs[c];
                const float* wr = w_in + ((size_t)tap * C + c) * 2 * C;
                for (int n = 0; n < 2 * C; ++n) rowacc[n] += sv * (double)wr[n];
            }
            float* dst = comp.data() + ((size_t)tap * 16 + j) * 2 * C;
            for (int n = 0; n < 2 * C; ++n) dst[n] = (float)rowacc[n];
        }
    return comp;
}

// Skip halves of the 8 res_skip convs folded into the `end` conv we [C][no], be [no]:
//   wf[i][o][c] = sum_s W_skip_i[c][s] * we[s][o]  ([8][8][C], rows o >= no zero);  bf[o] = sum_i b_skip_i @ we + be[o]
// wk[i] / bk[i]: kernel [C][rs_full] and bias [rs_full] of layer i, the skip half behind the C residual columns
// (layer 7 has no residual half).
void fold_skip_into_end(int C, const float* const wk[8], const float* const bk[8], const float* we, const float* be, int no,
                        std::vector<float>* wf, std::vector<float>* bf) {
    wf->assign((size_t)8 * 8 * C, 0.f);
    bf->assign(8, 0.f);
    std::vector<double> bsum(be, be + no), row(no);
    for (int i = 0; i < 8; ++i) {
        const int rs_full = i < 7 ? 2 * C : C, soff = i < 7 ? C : 0;
        for (int c = 0; c < C; ++c) {
            for (int o = 0; o < no; ++o) row[o] = 0.0;
            const float* ws = wk[i] + (size_t)c * rs_full + soff;
            for (int sidx = 0; sidx < C; ++sidx) {
                const double wv = ws[sidx];
                const float* wend = we + (size_t)sidx * no;
                for (int o = 0; o < no; ++o) row[o] += wv * (double)wend[o];
            }
            for (int o = 0; o < no; ++o) (*wf)[((size_t)i * 8 + o) * C + c] = (float)row[o];
        }
        for (int sidx = 0; sidx < C; ++sidx)
            for (int o = 0; o < no; ++o) bsum[o] += (double)bk[i][soff + sidx] * (double)we[(size_t)sidx * no + o];
    }
    for (int o = 0; o < no; ++o) (*bf)[o] = (float)bsum[o];
}

// Invertible1x1Conv.build_inverse (invertible_conv.py:41-47): W = kernel[0]^T, W_inverse = inv(W)^T, and the reverse conv
// (kernel layout [1][in][out]) computes out = audio @ W_inverse = audio @ inv(kernel[0]^T)^T.
// kernel [n][n] -> minv[j][c] = inv(W)[c][j]; false when the kernel is singular.  *log_abs_det = log |det kernel| (= that of
// its transpose W): the sum of log |pivot|, row swaps only change the sign.
bool invert_1x1(const float* kernel, int n, std::vector<float>* minv, double* log_abs_det) {
    std::vector<double> a((size_t)n * 2 * n, 0.0);      // [W | I], W[r][c] = kernel[c][r]
    for (int r = 0; r < n; ++r) {
        for (int c = 0; c < n; ++c) a[(size_t)r * 2 * n + c] = (double)kernel[(size_t)c * n + r];
        a[(size_t)r * 2 * n + n + r] = 1.0;
    }
    double logdet = 0.0;
    for (int col = 0; col < n; ++col) {                  // Gauss-Jordan with partial pivoting
        int piv = col;
        for (int r = col + 1; r < n; ++r)
            if (std::fabs(a[(size_t)r * 2 * n + col]) > std::fabs(a[(size_t)piv * 2 * n + col])) piv = r;
        if (std::fabs(a[(size_t)piv * 2 * n + col]) < 1e-12) return false;
        if (piv != col)
            for (int c = 0; c < 2 * n; ++c) std::swap(a[(size_t)piv * 2 * n + c], a[(size_t)col * 2 * n + c]);
        const double d = a[(size_t)col * 2 * n + col];
        logdet += std::log(std::fabs(d));
        for (int c = 0; c < 2 * n; ++c) a[(size_t)col * 2 * n + c] /= d;
        for (int r = 0; r < n; ++r) {
            if (r == col) continue;
            const double f = a[(size_t)r * 2 * n + col];
            if (f != 0.0)
                for (int c = 0; c < 2 * n; ++c) a[(size_t)r * 2 * n + c] -= f * a[(size_t)col * 2 * n + c];
        }
    }
    minv->resize((size_t)n * n);
    for (int j = 0; j < n; ++j)
        for (int c = 0; c < n; ++c) (*minv)[(size_t)j * n + c] = (float)a[(size_t)c * 2 * n + n + j];
    *log_abs_det = logdet;
    return true;
}

// The staging buffers of waveglow_finalize (raw Keras-layout kernels; largest: upsample 1024*80*80 = 6.55 M floats).  However
// finalize returns they are released, and unless it got to `keep` so is everything it has uploaded.
struct FinalizeGuard {
    tts_hip_engine* e;
    DevBuf stage, stage2, ut, wct;
    bool keep = false;
    ~FinalizeGuard() {
        for (DevBuf* b : {&stage, &stage2, &ut, &wct}) b->release();
        if (!keep) waveglow_free(e);
    }
};

}  // namespace

int waveglow_finalize(tts_hip_engine* e) {
    WaveGlowDev& wg = e->wg;
    waveglow_free(e);
    auto dims_str = [](const std::vector<int64_t>& d) {
        std::string s = "[";
        for (size_t i = 0; i < d.size(); ++i) s += (i ? ", " : "") + std::to_string(d[i]);
        return s + "]";
    };
    // the width of this handle's model: what block 0's start conv [1][n_half = 4][C] says; every other tensor must agree
    int C = 0;
    {
        const char* name = "waveglow/block-0/start_conv/kernel";
        const HostTensor* sc = find_tensor(e, name);
        if (!sc) return set_err(e, TTS_HIP_ENOTREADY, "missing tensor %s", name);
        const bool shaped = sc->dims.size() == 3 && sc->dims[0] == 1 && sc->dims[1] == 4;
        if (!shaped || (sc->dims[2] != 256 && sc->dims[2] != 512))
            return set_err(e, TTS_HIP_EINVAL, "tensor %s: expected [1, 4, n_channels] with n_channels = 256 or 512 (the supported widths), got %s",
                           name, dims_str(sc->dims).c_str());
        C = (int)sc->dims[2];
    }
    const int KCONV = 3 * C;                        // taps part of the in-layer K
    auto need = [&](const std::string& name, std::initializer_list<int64_t> dims, const HostTensor** out) -> int {
        const HostTensor* t = find_tensor(e, name);
        if (!t) return set_err(e, TTS_HIP_ENOTREADY, "missing tensor %s", name.c_str());
        if (t->dims != std::vector<int64_t>(dims))
            return set_err(e, TTS_HIP_EINVAL, "tensor %s has an unexpected shape %s (n_channels = %d by waveglow/block-0/start_conv/kernel)",
                           name.c_str(), dims_str(t->dims).c_str(), C);
        *out = t;
        return 0;
    };
    int rc;
    FinalizeGuard gd{e};
    DevBuf &stage = gd.stage, &stage2 = gd.stage2, &ut = gd.ut, &wct = gd.wct;
    HIPCHK(e, stage.ensure((size_t)1024 * 80 * 80 * 4));
    HIPCHK(e, stage2.ensure((size_t)1024 * 4 * 2 + 1024));
    HIPCHK(e, ut.ensure((size_t)NPH * KMEL * NCOND * 4));
    HIPCHK(e, wct.ensure((size_t)2 * C * NCOND * 4));
    auto put = [&](DevBuf& b, const HostTensor* t) -> int {
        HIPCHK(e, hipMemcpyAsync(b.p, t->data.data(), t->numel() * 4, hipMemcpyHostToDevice, e->stream));
        return 0;
    };
    const HostTensor *t, *t2;
    // ---- transposed-conv upsampling kernel -> per-phase operand UT (only used to fold the conditioning convs below)
    if ((rc = need("waveglow/upsample/kernel", {1024, 80, 80}, &t))) return rc;
    if ((rc = put(stage, t))) return rc;
    {
        const long long total = (long long)NPH * KMEL * NCOND;
        hipLaunchKernelGGL(pack_ut_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, stage.f(),
                           ut.f());
        HIPCHK(e, hipGetLastError());
    }
    if ((rc = need("waveglow/upsample/bias", {80}, &t))) return rc;
    float* d_bup = stage2.f() + 4 * C;              // 80 floats behind the bias staging area
    HIPCHK(e, hipMemcpyAsync(d_bup, t->data.data(), 80 * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));

    // ---- flows
    int n_half = 4, n_rem = 8;
    for (int k = 0; k < 12; ++k) {
        if (k % 4 == 0 && k > 0) {
            n_half -= 1;
            n_rem -= 2;
        }
        WgFlowDev& fl = wg.flow[k];
        fl.n_rem = n_rem;
        fl.n_half = n_half;
        const std::string p = "waveglow/block-" + std::to_string(k);
        const HostTensor *ws, *bs;
        if ((rc = need(p + "/start_conv/kernel", {1, n_half, C}, &ws))) return rc;
        if ((rc = upload(e, ws->data.data(), ws->numel(), &fl.start_w, wg.allocs))) return rc;
        if ((rc = need(p + "/start_conv/bias", {C}, &bs))) return rc;
        if ((rc = upload(e, bs->data.data(), bs->numel(), &fl.start_b, wg.allocs))) return rc;
        const float *skip_w[8], *skip_b[8];
        for (int i = 0; i < 8; ++i) {
            WgLayerDev& ly = fl.layer[i];
            const std::string si = std::to_string(i);
            const int kconv = i == 0 ? KCONV0 : KCONV;
            if ((rc = dev_alloc(e, (size_t)2 * C * kconv, &ly.in_Bt, wg.allocs, false))) return rc;
            if ((rc = need(p + "/in_conv-" + si + "/kernel", {3, C, 2 * C}, &t))) return rc;
            if (i == 0) {
                const std::vector<float> comp = compose_start_taps(C, t->data.data(), ws->data.data(), bs->data.data(), n_half);
                HIPCHK(e, hipMemcpyAsync(stage.p, comp.data(), comp.size() * 4, hipMemcpyHostToDevice, e->stream));
                HIPCHK(e, hipStreamSynchronize(e->stream));
                if ((rc = pack_bt(e, C, stage.f(), KCONV0, 2 * C, ly.in_Bt, 2 * C, kconv, 0, 1))) return rc;   // K order tap*16 + j
            } else {
                if ((rc = put(stage, t))) return rc;
                if ((rc = pack_bt(e, C, stage.f(), 3 * C, 2 * C, ly.in_Bt, 2 * C, kconv, 0, 1, WN_TAPS, WN_BK))) return rc;
            }
            HIPCHK(e, hipStreamSynchronize(e->stream));
            // conditioning conv: WcT[n'][k] (gate-permuted rows), then V_{i,p} = WcT @ U_p for the 32 phases
            if ((rc = need(p + "/cond_layer-" + si + "/kernel", {1, NCOND, 2 * C}, &t))) return rc;
            if ((rc = put(stage, t))) return rc;
            if ((rc = pack_bt(e, C, stage.f(), NCOND, 2 * C, wct.f(), 2 * C, NCOND, 0, 1))) return rc;
            if ((rc = dev_alloc(e, (size_t)NPH * 2 * C * KMEL, &ly.cond_Bt, wg.allocs, false))) return rc;
            {
                GemmArgs g{};
                g.M = 2 * C;
                g.N = KMEL;
                g.L = 2 * C;
                g.nseg = 1;
                g.seg[0] = ASeg{wct.f(), NCOND, 0, NCOND, NCOND};
                g.Bt = ut.f();
                g.ldb = NCOND;
                g.strideBz = (long long)KMEL * NCOND;
                g.mode = EPI_LINEAR;
                g.split = KMEL;
                g.out0 = ly.cond_Bt;
                g.ld0 = KMEL;
                g.strideOutZ = (long long)2 * C * KMEL;
                HIPCHK(e, gemm_small(g, NPH, e->stream));
            }
            if ((rc = need(p + "/in_conv-" + si + "/bias", {2 * C}, &t))) return rc;
            if ((rc = need(p + "/cond_layer-" + si + "/bias", {2 * C}, &t2))) return rc;
            if ((rc = dev_alloc(e, 2 * C, &ly.in_bias, wg.allocs, false))) return rc;
            HIPCHK(e, hipMemcpyAsync(stage2.p, t->data.data(), 2 * C * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHK(e, hipMemcpyAsync(stage2.f() + 2 * C, t2->data.data(), 2 * C * 4, hipMemcpyHostToDevice, e->stream));
            for_width(C, [&](auto cc) {
                constexpr int CC = decltype(cc)::value;
                hipLaunchKernelGGL(pack_bias_kernel<CC>, dim3(2 * CC / 256), dim3(256), 0, e->stream, stage2.f(), stage2.f() + 2 * CC,
                                   ly.in_bias, 2 * CC, 1);
                hipLaunchKernelGGL(cond_bias_kernel<CC>, dim3(2 * CC / 256), dim3(256), 0, e->stream, wct.f(), d_bup, ly.in_bias);
            });
            HIPCHK(e, hipGetLastError());
            HIPCHK(e, hipStreamSynchronize(e->stream));
            // res_skip conv: keep only the residual half as a GEMM operand (layers 0..6); the skip half is folded below
            const int rs_full = i < 7 ? 2 * C : C;
            if ((rc = need(p + "/res_skip_conv-" + si + "/kernel", {1, C, rs_full}, &t))) return rc;
            if ((rc = need(p + "/res_skip_conv-" + si + "/bias", {rs_full}, &t2))) return rc;
            skip_w[i] = t->data.data();
            skip_b[i] = t2->data.data();
            ly.rs_n = i < 7 ? C : 0;
            if (i < 7) {
                if ((rc = dev_alloc(e, (size_t)C * C, &ly.rs_Bt, wg.allocs, false))) return rc;
                if ((rc = put(stage, t))) return rc;
                if ((rc = pack_bt(e, C, stage.f(), C, rs_full, ly.rs_Bt, C, C, 0, 0))) return rc;      // rows n < C = residual outputs
                HIPCHK(e, hipStreamSynchronize(e->stream));
                if ((rc = upload(e, t2->data.data(), C, &ly.rs_bias, wg.allocs))) return rc;
            }
        }
        {
            const HostTensor *we, *be;
            if ((rc = need(p + "/end_conv/kernel", {1, C, 2 * n_half}, &we))) return rc;
            if ((rc = need(p + "/end_conv/bias", {2 * n_half}, &be))) return rc;
            std::vector<float> wf, bf;
            fold_skip_into_end(C, skip_w, skip_b, we->data.data(), be->data.data(), 2 * n_half, &wf, &bf);
            if ((rc = upload(e, wf.data(), wf.size(), &fl.end_w, wg.allocs))) return rc;
            if ((rc = upload(e, bf.data(), bf.size(), &fl.end_b, wg.allocs))) return rc;
        }
        if ((rc = need("waveglow/invertible_conv-" + std::to_string(k) + "/conv/kernel", {1, n_rem, n_rem}, &t))) return rc;
        std::vector<float> minv;
        if (!invert_1x1(t->data.data(), n_rem, &minv, &fl.log_det))
            return set_err(e, TTS_HIP_EINVAL, "invertible_conv-%d kernel is singular", k);
        if ((rc = upload(e, minv.data(), minv.size(), &fl.inv, wg.allocs))) return rc;
        if ((rc = upload(e, t->data.data(), t->numel(), &fl.fwd, wg.allocs))) return rc;      // forward flow: audio @ kernel[0]
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    gd.keep = true;
    wg.channels = C;
    wg.ready = true;
    return TTS_HIP_OK;
}

// Builds the fp16 GEMM operands of one mode from the packed fp32 device copies (once).  split: every matrix as two planes,
// hi = fp16(w) and, n elements behind it, lo = fp16(w - hi).
static int waveglow_build_half(tts_hip_engine* e, bool split) {
    WaveGlowDev& wg = e->wg;
    bool& ready = split ? wg.x3_ready : wg.f16_ready;
    if (ready) return TTS_HIP_OK;
    const int C = wg.channels, KCONV = 3 * C;
    hipStream_t st = e->stream;
    auto alloc_h = [&](size_t n, _Float16** out) -> int {
        void* p = nullptr;
        HIPCHK(e, hipMalloc(&p, (split ? 2 : 1) * n * sizeof(_Float16)));
        wg.allocs.push_back(p);
        *out = (_Float16*)p;
        return TTS_HIP_OK;
    };
    auto lo = [&](_Float16* hi, size_t n) { return split ? hi + n : (_Float16*)nullptr; };
    auto grid = [](size_t n) { return dim3((unsigned)((n + 255) / 256)); };
    int rc;
    for (int k = 0; k < 12; ++k)
        for (int i = 0; i < 8; ++i) {
            WgLayerDev& ly = wg.flow[k].layer[i];
            _Float16 *a, *c, *r = nullptr;
            const size_t na = (size_t)2 * C * (i == 0 ? 96 : KCONV), nc = (size_t)NPH * 2 * C * KMEL, nr = (size_t)C * C;
            if ((rc = alloc_h(na, &a))) return rc;
            for_width(C, [&](auto cc) {
                constexpr int CC = decltype(cc)::value;
                if (i == 0) hipLaunchKernelGGL(cvt_taps0_kernel<CC>, grid(na), dim3(256), 0, st, ly.in_Bt, a, lo(a, na));
                else hipLaunchKernelGGL(cvt_taps_kernel<CC>, grid(na), dim3(256), 0, st, ly.in_Bt, a, lo(a, na));
            });
            if ((rc = alloc_h(nc, &c))) return rc;
            hipLaunchKernelGGL(cvt_half_kernel, grid(nc), dim3(256), 0, st, ly.cond_Bt, c, (long long)nc, lo(c, nc));
            if (ly.rs_n) {
                if ((rc = alloc_h(nr, &r))) return rc;
                hipLaunchKernelGGL(cvt_half_kernel, grid(nr), dim3(256), 0, st, ly.rs_Bt, r, (long long)nr, lo(r, nr));
            }
            HIPCHK(e, hipGetLastError());
            ly.in_Bt16[split] = a;
            ly.cond_Bt16[split] = c;
            ly.rs_Bt16[split] = r;
        }
    HIPCHK(e, hipStreamSynchronize(st));
    ready = true;
    return TTS_HIP_OK;
}

// ---- the pieces of waveglow_run
namespace {

// The three WN GEMM launchers of a call, chosen once from (precision, tile family).  This table is the only place that names
// the gemm_wn_* wrappers of gemm_f32.h; the wrappers that take a bool are bound to it here.
using WnLaunch = hipError_t (*)(const GemmArgs&, hipStream_t);
template <hipError_t (*F)(const GemmArgs&, bool, hipStream_t), bool V>
hipError_t bound(const GemmArgs& g, hipStream_t s) {
    return F(g, V, s);
}
struct WnKernels {
    WnLaunch in0, in, res;      // first layer of a flow (K = 3 taps of a0p), layers 1 .. 7, residual GEMM
};
const WnKernels kWnKernels[3][4] = {
    // fp32                                                                                        WgTiles
    {{gemm_wn_in0, gemm_wn_in, gemm_wn_res_skip},                                               // WG_T256
     {gemm_wn_in0_128, gemm_wn_in_128, gemm_wn_res_skip},                                       // WG_T128
     {gemm_wn_in0_64, gemm_wn_in_64, gemm_wn_res_64},                                           // WG_T128x64
     {gemm_wn_in0_r64, gemm_wn_in_r64, gemm_wn_res_r64}},                                       // WG_ROW64
    // fp16: the 128- and 256-row families are one wrapper with a bool t128
    {{bound<gemm_wn_in0_h, false>, bound<gemm_wn_in_h, false>, gemm_wn_res_h},
     {bound<gemm_wn_in0_h, true>, bound<gemm_wn_in_h, true>, gemm_wn_res_h},
     {gemm_wn_in0_64h, gemm_wn_in_64h, gemm_wn_res_64h},
     {gemm_wn_in0_r64h, gemm_wn_in_r64h, gemm_wn_res_r64h}},
    // split fp16: two tile shapes, a bool small; wg_plan reports WG_T256 or WG_ROW64 only
    {{bound<gemm_wn_in0_x3, false>, bound<gemm_wn_in_x3, false>, bound<gemm_wn_res_x3, false>},
     {bound<gemm_wn_in0_x3, false>, bound<gemm_wn_in_x3, false>, bound<gemm_wn_res_x3, false>},
     {bound<gemm_wn_in0_x3, false>, bound<gemm_wn_in_x3, false>, bound<gemm_wn_res_x3, false>},
     {bound<gemm_wn_in0_x3, true>, bound<gemm_wn_in_x3, true>, bound<gemm_wn_res_x3, true>}},
};

// x, audio and the operands of the call's precision (layouts: the header comment of this file)
int ensure_workspace(tts_hip_engine* e, const WgPlan& p, int precision) {
    WaveGlowDev& wg = e->wg;
    const size_t M = (size_t)p.M, NP = (size_t)p.NP, C = (size_t)wg.channels;
    HIPCHK(e, wg.x.ensure(M * C * 4));
    HIPCHK(e, wg.audio.ensure(M * 8 * 4));
    if (precision != 0) {
        HIPCHK(e, wg.x16.ensure(NP * M * C * 2));
        HIPCHK(e, wg.acts16.ensure(8 * NP * M * C * 2));
        HIPCHK(e, wg.a0p16.ensure(NP * M * 32 * 2));
        HIPCHK(e, wg.mel16.ensure(NP * p.BT * KMEL * 2 + 256));
    } else {
        HIPCHK(e, wg.acts.ensure(8 * M * C * 4));              // activations of the 8 layers of one flow
        HIPCHK(e, wg.a0p.ensure(M * 16 * 4));
        HIPCHK(e, wg.endp.ensure(7 * M * 8 * 4));              // end partial sums of layers 0 .. 6 (512 channels only)
    }
    return TTS_HIP_OK;
}

// One A operand as the GEMM kernels address it: rows of `ld` floats and, in split fp16, the lo plane `plane` floats behind
// the hi plane.  An fp16 operand is described in these float units too (one unit = 2 halfs), so its ld, k, kpad and the ldb
// of its weights are half the element counts -- WnCall::unit below is the one place that says so.
struct WnOperand {
    const float* p;
    int ld;
    long long plane;
};
// The operands of one call in its precision
struct WnCall {
    WgPlan plan;
    int C;                          // n_channels of the handle
    int precision, T;
    int unit;                       // elements per float unit: 1 fp32, 2 the fp16 modes
    WnOperand a0p, x, mel;          // first-layer operand, residual stream (fp16 modes: its shadow), mel frames / windows
    float* x32;                     // fp32 residual stream (fp16 modes: the master copy)
    float* acts;                    // gated activations of layer 0; layer i lies i * acts_stride floats behind, with x's plane
    long long acts_stride;
    float* endp;                    // [7][M][8] end partial sums of the current flow, one slot per residual GEMM (fp32, 512
                                    // channels: the table of gemm_f32.h is laid out for K = N = 512); else null
    bool split() const { return precision == 2; }
    float* acts_of(int i) const { return acts + i * acts_stride; }
    // a weight matrix of the call's precision (the fp16 ones exist once waveglow_build_half has run)
    const float* weights(const float* f32, _Float16* const (&f16)[2]) const {
        return precision == 0 ? f32 : (const float*)f16[split()];
    }
};

WnCall wn_call(WaveGlowDev& wg, const WgPlan& p, int precision, int T, const float* d_mel) {
    const bool f16 = precision != 0;
    const long long pl = precision == 2 ? 1 : 0;       // split fp16: the lo plane lies one whole operand behind the hi plane
    WnCall c{};
    const int C = wg.channels;
    c.plan = p;
    c.C = C;
    c.precision = precision;
    c.T = T;
    c.unit = f16 ? 2 : 1;
    c.a0p = {f16 ? wg.a0p16.f() : wg.a0p.f(), 16, pl * p.M * 16};            // 16 floats or 32 halfs per row
    c.x = {f16 ? wg.x16.f() : wg.x.f(), C / c.unit, pl * p.M * C / 2};
    // fp32: four frames t .. t-3 of 80 floats against the per-phase weights V_{i,p}; fp16: one contiguous 4-frame window
    c.mel = {f16 ? wg.mel16.f() : d_mel, f16 ? KMEL / 2 : 80, pl * p.BT * KMEL / 2};
    c.x32 = wg.x.f();
    c.acts = f16 ? wg.acts16.f() : wg.acts.f();
    c.acts_stride = p.NP * p.M * C / c.unit;
    c.endp = (precision == 0 && C == 512) ? wg.endp.f() : nullptr;
    return c;
}

// In-layer GEMM of layer i: K = 3 taps (of a0p for the first layer: conv(start(a0)) composed at load time, K = 3 x 16 with
// h + 1 used instead of 3 x C; of x otherwise) + the folded conditioning, N = 2 C, gate epilogue -> acts_of(i)
GemmArgs in_layer_args(const WnCall& c, const WgLayerDev& ly, int i) {
    const WgPlan& p = c.plan;
    const int d = 1 << i, u = c.unit, C = c.C;
    GemmArgs g{};
    g.M = (int)p.M;
    g.N = 2 * C;
    g.L = c.T;                                 // sequence bounds are tested on the frame index inside a batch item
    g.phase_rows = p.PR;
    g.frames = p.BT;
    g.phase_step = d < 32 ? d : 1;             // taps at +-d groups: another phase block for d < 32, else +-d / 32 frames
    g.bias = ly.in_bias;
    g.mode = EPI_GATE;
    g.split = 2 * C;
    g.wide_epi = 1;
    const WnOperand& a = i == 0 ? c.a0p : c.x;
    for (int tap = 0; tap < 3; ++tap) g.seg[tap] = ASeg{a.p, a.ld, (tap - 1) * d, a.ld, a.ld, SEG_PHASE_TAP, a.plane};
    const int nmel = c.precision == 0 ? 4 : 1;
    for (int q = 0; q < nmel; ++q) g.seg[3 + q] = ASeg{c.mel.p, c.mel.ld, -q, c.mel.ld, c.mel.ld, SEG_FRAME, c.mel.plane};
    g.nseg = 3 + nmel;
    g.Bt = c.weights(ly.in_Bt, ly.in_Bt16);
    g.ldb = 3 * a.ld;
    g.planeB = c.split() ? (long long)2 * C * g.ldb : 0;
    g.Bt2 = c.weights(ly.cond_Bt, ly.cond_Bt16);
    g.ldb2 = KMEL / u;
    g.strideB2p = (long long)2 * C * KMEL / u;
    g.planeB2 = c.split() ? (long long)NPH * 2 * C * KMEL / 2 : 0;
    g.ld0 = C;
    if (c.precision == 0) {
        g.out0 = c.acts_of(i);
    } else {
        g.out0 = c.x32;                        // unused by the gate epilogue (fp16 output below)
        g.out0h = (_Float16*)c.acts_of(i);
        g.ld0h = C;
        g.planeOut = p.M * C;
    }
    return g;
}

// Residual GEMM of layer i < 7: x += acts_i @ W_res + b_res   (skip half folded into wn_end_fold).  With c.endp the launch
// also stores endp[i] = acts_i @ wfold_i^T, wfold_i = end_w + i * 8 * C the layer's folded end weights
GemmArgs res_args(const WnCall& c, const WgLayerDev& ly, int i, const float* end_w) {
    const int u = c.unit, C = c.C;
    GemmArgs r{};
    r.M = (int)c.plan.M;
    r.N = C;
    r.L = (int)c.plan.M;
    r.nseg = 1;
    r.seg[0] = ASeg{c.acts_of(i), C / u, 0, C / u, C / u, SEG_ROWS, c.x.plane};
    r.Bt = c.weights(ly.rs_Bt, ly.rs_Bt16);
    r.ldb = C / u;
    r.planeB = c.split() ? (long long)C * C / 2 : 0;
    r.bias = ly.rs_bias;
    r.mode = EPI_LINEAR;
    r.act = ACT_NONE;
    r.split = C;
    r.out0 = c.x32;                            // fp16 modes: fp32 master of the residual stream (read-modify-write)
    r.ld0 = C;
    r.acc0 = 1;
    r.wide_epi = 1;
    if (c.precision != 0) {
        r.out0h = (_Float16*)const_cast<float*>(c.x.p);    // fp16 shadow = operand of the next layer's taps
        r.ld0h = C;
        r.planeOut = c.plan.M * C;
    }
    if (c.endp) {                              // (GemmArgs::end_sums: the second output of a single-output launch)
        r.end_sums = 1;
        r.altbias = end_w + (long long)i * 8 * C;
        r.out1 = c.endp + (long long)i * c.plan.M * 8;
        r.ld1 = 8;
    }
    return r;
}

int in_layer_timing_kind(int precision, int i) {
#ifdef TTS_DEBUG_HOOKS
    static const bool split_dil = getenv("TTS_TIME_SPLIT_DIL") != nullptr;    // measurement builds: time the fp16 / f16x3
    if (precision != 0 && i > 0 && split_dil && (1 << i) >= 32) return 2;     // layers with d >= 32 as kind 2
#endif
    return i == 0 ? 3 : 0;
}

// Folded skip / end conv + affine inverse + inverse 1x1 conv of one flow: one of the nine <HALF, SPLIT, MASK> instantiations
// of wn_end_fold_kernel of the handle's width, with the kernel's arguments `a`
template <bool HALF, bool SPLIT, int MASK, class... A>
void end_fold(int C, dim3 grid, hipStream_t st, A... a) {
    if (C == 512) {                 // the kernel's default width: the instantiations a 512-channel model has always run
        hipLaunchKernelGGL((wn_end_fold_kernel<HALF, SPLIT, MASK>), grid, dim3(256), 0, st, a...);
    } else {
        const auto narrow = wn_end_fold_kernel<HALF, SPLIT, MASK, 256>;
        hipLaunchKernelGGL(narrow, grid, dim3(256), 0, st, a...);
    }
}
template <class... A>
void launch_end_fold(int C, int precision, int mask, dim3 grid, hipStream_t st, A... a) {
    switch (precision * 3 + mask) {
        case 0 * 3 + MASK_NONE: return end_fold<false, false, MASK_NONE>(C, grid, st, a...);
        case 0 * 3 + MASK_LENS: return end_fold<false, false, MASK_LENS>(C, grid, st, a...);
        case 0 * 3 + MASK_FLAGS: return end_fold<false, false, MASK_FLAGS>(C, grid, st, a...);
        case 1 * 3 + MASK_NONE: return end_fold<true, false, MASK_NONE>(C, grid, st, a...);
        case 1 * 3 + MASK_LENS: return end_fold<true, false, MASK_LENS>(C, grid, st, a...);
        case 1 * 3 + MASK_FLAGS: return end_fold<true, false, MASK_FLAGS>(C, grid, st, a...);
        case 2 * 3 + MASK_NONE: return end_fold<true, true, MASK_NONE>(C, grid, st, a...);
        case 2 * 3 + MASK_LENS: return end_fold<true, true, MASK_LENS>(C, grid, st, a...);
        case 2 * 3 + MASK_FLAGS: return end_fold<true, true, MASK_FLAGS>(C, grid, st, a...);
    }
}

// ---- test hook (tts_hip_waveglow_probe): the call stops at the probed layer or flow and copies what it holds there
bool probe_wants_layer(const WaveGlowDev& wg, int precision, int k, int i) {
    // what 0: the gated activations; 2: the layer's conditioning plane, which only the fp32 path has
    return wg.probe_out && wg.probe_flow == k && wg.probe_layer == i && (precision == 0 ? wg.probe_what != 1 : wg.probe_what == 0);
}
int probe_layer(tts_hip_engine* e, const WnCall& c, int i, bool wino_layer) {
    WaveGlowDev& wg = e->wg;
    const WgPlan& p = c.plan;
    const int C = c.C;
    const bool plane = wg.probe_what == 2;                    // the layer's conditioning plane (Winograd form only)
    if (plane && !wino_layer)
        return set_err(e, TTS_HIP_EINVAL, "waveglow_probe: layer %d of this call has no conditioning plane", i);
    const int W = plane ? 2 * C : C;
    const long long n4 = (long long)p.BT * NPH * (W / 4);
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (c.precision == 0) {
        hipLaunchKernelGGL(probe_acts_kernel, grid, dim3(256), 0, e->stream, plane ? wg.wino_cond.f() : c.acts_of(i),
                           wg.probe_out, p.PR, p.BT, c.T, W);
    } else {
        const _Float16* acts_i = (const _Float16*)c.acts_of(i);
        for_width(C, [&](auto cc) {
            hipLaunchKernelGGL(probe_acts16_kernel<decltype(cc)::value>, grid, dim3(256), 0, e->stream, acts_i,
                               c.split() ? acts_i + p.M * C : (const _Float16*)nullptr, wg.probe_out, p.PR, p.BT, c.T);
        });
    }
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}
bool probe_wants_state(const WaveGlowDev& wg, int k) { return wg.probe_out && wg.probe_what == 1 && wg.probe_flow == k; }
int probe_state(tts_hip_engine* e, const WgPlan& p, const float* state, int natural, int n, float* out, int pitch = 8) {
    const long long np = (long long)p.BT * NPH;
    hipLaunchKernelGGL(probe_state_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, e->stream, state, natural, out, n,
                       p.PR, p.BT, pitch);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

// fp32, the layers in their Winograd form (wn_wino.hip): builds its operands.  They are extra (8.1 GB of weight planes on
// first use, the conditioning plane -- 0.84 GB at config 2 -- and the mel planes per call): when the device cannot hold them
// -- and only then: any other error is the call's error -- *wino = false and this handle keeps the direct form from now on
int wino_begin_or_fall_back(tts_hip_engine* e, const WgPlan& p, const float* d_mel, int T, bool* wino) {
    WaveGlowDev& wg = e->wg;
    const int C = 512;                                                // the Winograd form is a 512-channel form (waveglow_run)
    size_t free_b = 0, total_b = 0;
    HIPCHK(e, hipMemGetInfo(&free_b, &total_b));
    const size_t plane = (size_t)p.M * 2 * C * 4 > wg.wino_cond.bytes ? (size_t)p.M * 2 * C * 4 : 0;
    const size_t need = (wg.wino_ready ? 0 : (size_t)9 << 30) + plane;
    int rc = free_b < need ? TTS_HIP_ENOMEM : waveglow_build_wino(e);
    if (!rc) rc = waveglow_wino_begin(e, d_mel, p.PR, p.BT, T, wg.form_mode);
    if (rc && rc != TTS_HIP_ENOMEM) return rc;
    if (rc) {
        (void)hipGetLastError();                                      // (clears the sticky out-of-memory status)
        wg.form_mode = 0;
        *wino = false;
    }
    return TTS_HIP_OK;
}

// Which frames of a call are not real: the mask kind and the list of those frames (waveglow_run)
struct WnTails {
    int mask;
    const int* d_tail;
    int n_tail;
};
// x (and its fp16 shadow; after the start conv also the a0p rows) = 0 on the tail rows: store-only, tail bytes only
int zero_tail(tts_hip_engine* e, const WnCall& c, const WnTails& t, bool with_a0p) {
    if (t.mask == MASK_NONE || t.n_tail == 0) return TTS_HIP_OK;
    WaveGlowDev& wg = e->wg;
    const long long n4 = (long long)NPH * t.n_tail * (c.C / 4);
    const bool h16 = c.precision != 0;
    for_width(c.C, [&](auto cc) {
        hipLaunchKernelGGL(wn_zero_tail_kernel<decltype(cc)::value>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, e->stream,
                           t.d_tail, t.n_tail, c.plan.PR, c.plan.M, wg.x.f(), h16 ? (_Float16*)wg.x16.p : (_Float16*)nullptr,
                           c.precision == 2 ? 2 : 1, with_a0p ? (h16 ? wg.a0p16.p : wg.a0p.p) : nullptr);
    });
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

// The WN block of flow k on the flow state wg.audio, for either direction: start kernel, the eight layers in the call's form,
// the residual GEMMs.  Leaves the eight layers' activations (and, with call.endp, the end partial sums) for the direction's
// boundary kernel.  probes: the inverse direction's test hook may stop the call at a layer (*stopped, with the probe's status
// as the return value); the forward direction passes false and ignores armed hooks.
int wn_flow(tts_hip_engine* e, const WnCall& call, const WnKernels& kn, const WgFlowDev& fl, int k, bool wino,
            const WnTails& tails, bool probes, bool* stopped) {
    WaveGlowDev& wg = e->wg;
    hipStream_t st = e->stream;
    const int C = call.C, precision = call.precision, h = fl.n_half, PR = call.plan.PR, BT = call.plan.BT, T = call.T;
    const long long M = call.plan.M;
    *stopped = false;
    {
        const long long n4 = M * (C / 4);
        const dim3 grid((unsigned)((n4 + 255) / 256));
        for_width(C, [&](auto cc) {
            constexpr int CC = decltype(cc)::value;
            if (precision != 0)
                hipLaunchKernelGGL((wn_start_kernel<CC, true>), grid, dim3(256), 0, st, wg.audio.f(), fl.start_w, fl.start_b,
                                   wg.x.f(), wg.a0p16.p, (_Float16*)wg.x16.p, M, h, precision == 2 ? 1 : 0);
            else
                hipLaunchKernelGGL((wn_start_kernel<CC, false>), grid, dim3(256), 0, st, wg.audio.f(), fl.start_w, fl.start_b,
                                   wg.x.f(), wg.a0p.p, (_Float16*)nullptr, M, h);
        });
        HIPCHK(e, hipGetLastError());
        if (int rc = zero_tail(e, call, tails, true)) return rc;
    }
    for (int i = 0; i < 8; ++i) {
        const WgLayerDev& ly = fl.layer[i];
        const bool wino_layer = wino && i > 0;
        if (wino_layer) {
            if (int rc = waveglow_wino_layer(e, ly, i, wg.x.f(), call.acts_of(i), PR, BT, T)) return rc;
        } else if (wino) {                 // first layer of a flow: the plane kernel's K loop, taps and gate in its epilogue
            if (int rc = waveglow_wino_layer0(e, ly, h, wg.a0p.f(), call.acts_of(0), PR, BT, T)) return rc;
        } else {
            const GemmArgs g = in_layer_args(call, ly, i);
            timing_begin(e, in_layer_timing_kind(precision, i));
            HIPCHK(e, (i == 0 ? kn.in0 : kn.in)(g, st));
            timing_end(e);
        }
        if (probes && probe_wants_layer(wg, precision, k, i)) {      // test hook: stop here
            *stopped = true;
            return probe_layer(e, call, i, wino_layer);
        }
        if (i < 7) {
            const GemmArgs r = res_args(call, ly, i, fl.end_w);
            timing_begin(e, 1);
            HIPCHK(e, kn.res(r, st));
            timing_end(e);
            if (int rc = zero_tail(e, call, tails, false)) return rc;
        }
    }
    return TTS_HIP_OK;
}

// Ragged calls: private copy of the mel with cleared tails (mel_ragged_copy_kernel) -> *d_mel
int ragged_mel(tts_hip_engine* e, const float** d_mel, const int* d_lens, int BT, int T) {
    WaveGlowDev& wg = e->wg;
    HIPCHK(e, wg.mel_ragged.ensure((size_t)BT * 80 * 4));
    const long long n4 = (long long)BT * 20;
    hipLaunchKernelGGL(mel_ragged_copy_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, e->stream, *d_mel,
                       wg.mel_ragged.f(), d_lens, BT, T);
    HIPCHK(e, hipGetLastError());
    *d_mel = wg.mel_ragged.f();
    return TTS_HIP_OK;
}

}  // namespace

// precision 0: exact fp32 MFMA path.  precision 1: fp16 operands (activations, mel and weights fp16 in HBM), fp32
// accumulation and fp32 epilogue math, fp32 master copy of the residual stream and of the flow state.  precision 2: split
// fp16 -- every GEMM operand is a pair of fp16 planes (hi, lo), three MFMAs per product (hi*hi + hi*lo + lo*hi), fp32
// accumulation: ~22 operand bits, i.e. fp32-class results at 3/16 of the fp32 MFMA cost.
// Ragged calls (d_lens != null): d_lens [B] frames of each row are real, d_tail lists the n_tail frames b * T + t beyond them.
// x is kept at 0 on those rows wherever it is written; the transposed-conv upsampling is causal (a sample only sees mel
// frames at or before its own), so the residual stream is the only way a row's tail could reach its real positions, and
// a row then computes what a call on its own frames computes.  d_lens == null: the launches below
// are exactly those of a call without lengths.
// Packed calls (d_flags != null, B = 1, d_lens null): d_flags [T] is non-zero on the real frames of the one row, d_tail lists
// its n_tail gap frames, and d_mel is already a private copy with zero gap frames (waveglow_run_packed below).  The same
// argument holds with "gap frame" for "tail frame": nothing in it needs the zero frames to be at the end of a row.
//
// The driver: wg_plan (wg_plan.h) says which tile family and form the call takes, kWnKernels which three GEMM launchers that
// means, wn_call describes the operands of the precision once; the loop below is then the same for every call.
int waveglow_run(tts_hip_engine* e, const float* d_mel, int B, int T, const float* d_z, float sigma, float* d_audio,
                 int precision, const int* d_lens, const int* d_tail, int n_tail, const int* d_flags) {
    WaveGlowDev& wg = e->wg;
    if (d_flags && (B != 1 || d_lens)) return set_err(e, TTS_HIP_EINVAL, "waveglow_run: a packed run is one row without lengths");
    const int mask = d_flags ? MASK_FLAGS : d_lens ? MASK_LENS : MASK_NONE;      // which frames are not real
    const int* mask_info = d_flags ? d_flags : d_lens;
    if (precision != 0)
        if (int rc = waveglow_build_half(e, precision == 2)) return rc;
    const int C = wg.channels;
    WgPlan plan = wg_plan(B * T, precision, wg.form_mode);
    if (C != 512) plan.wino_wanted = false;      // the Winograd form (wn_wino.hip) is built on N = 1024 planes: 512 channels only
    const int BT = plan.BT, PR = plan.PR;
    const long long M = plan.M;
    if ((double)M * C * 4.0 >= 2147483648.0 - 65536.0)
        return set_err(e, TTS_HIP_EINVAL, "waveglow_infer: B*T = %d frames exceeds one call's limit (~32000)", BT);
    if (int rc = ensure_workspace(e, plan, precision)) return rc;
    hipStream_t st = e->stream;
    if (mask == MASK_LENS)                                       // every reader below takes the copy with cleared tails
        if (int rc = ragged_mel(e, &d_mel, d_lens, BT, T)) return rc;
    const WnTails tails{mask, d_tail, n_tail};
    bool wino = plan.wino_wanted;
    if (wino)
        if (int rc = wino_begin_or_fall_back(e, plan, d_mel, T, &wino)) return rc;
    wg.last_form = wino ? 1 : 0;
    wg.last_tiles = plan.tiles;
    const WnKernels& kn = kWnKernels[precision][plan.tiles];
    const WnCall call = wn_call(wg, plan, precision, T, d_mel);
    _Float16* mel16 = (_Float16*)wg.mel16.p;

    const unsigned mb = (unsigned)((M + 255) / 256);
    if (mask == MASK_FLAGS)
        hipLaunchKernelGGL(init_audio_kernel<MASK_FLAGS>, dim3(mb), dim3(256), 0, st, d_z, sigma, wg.audio.f(), PR, BT, d_flags, T);
    else if (mask == MASK_LENS)
        hipLaunchKernelGGL(init_audio_kernel<MASK_LENS>, dim3(mb), dim3(256), 0, st, d_z, sigma, wg.audio.f(), PR, BT, d_lens, T);
    else
        hipLaunchKernelGGL(init_audio_kernel<MASK_NONE>, dim3(mb), dim3(256), 0, st, d_z, sigma, wg.audio.f(), PR, BT, (const int*)nullptr, 1);
    if (precision != 0) {
        const long long n = (long long)BT * KMEL;
        hipLaunchKernelGGL(mel_window_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_mel, mel16,
                           precision == 2 ? mel16 + n : (_Float16*)nullptr, BT, T);
    }
    HIPCHK(e, hipGetLastError());

    int zoff = 4;
    for (int k = 11; k >= 0; --k) {
        const WgFlowDev& fl = wg.flow[k];
        const int h = fl.n_half;
        bool stopped = false;
        if (int rc = wn_flow(e, call, kn, fl, k, wino, tails, true, &stopped)) return rc;
        if (stopped) return TTS_HIP_OK;
        const bool early = (k % 4 == 0) && k > 0;
        float* dst = (k == 0) ? d_audio : wg.audio.f();
        const long long waves = (M + RPW - 1) / RPW;
        // elements between two layers' activations and (split fp16) from their hi to their lo plane; a call without a mask
        // passes no frame info and T = 1 (not read)
        const dim3 egrid((unsigned)((waves + 3) / 4));
        if (call.endp) {                                         // fp32: layer 7 on top of the residual GEMMs' partial sums
            auto last = [&](auto kern) {
                hipLaunchKernelGGL(kern, egrid, dim3(256), 0, st, (const float*)call.acts_of(7), (const float*)(fl.end_w + 7 * 8 * C),
                                   (const float*)call.endp, (const float*)fl.end_b, (const float*)fl.inv, wg.audio.f(), dst,
                                   k == 0 ? 1 : 0, d_z, zoff, early ? 2 : 0, sigma, M, h, PR, BT, mask_info,
                                   mask == MASK_NONE ? 1 : T);
            };
            if (mask == MASK_FLAGS) last(wn_end_last_kernel<MASK_FLAGS>);
            else if (mask == MASK_LENS) last(wn_end_last_kernel<MASK_LENS>);
            else last(wn_end_last_kernel<MASK_NONE>);
        } else {
            launch_end_fold(C, precision, mask, egrid, st, (const void*)call.acts, plan.NP * M * C, fl.end_w, fl.end_b, fl.inv,
                            wg.audio.f(), dst, k == 0 ? 1 : 0, d_z, zoff, early ? 2 : 0, sigma, M, h, PR, BT,
                            precision == 2 ? M * C : 0ll, mask_info, mask == MASK_NONE ? 1 : T);
        }
        HIPCHK(e, hipGetLastError());
        if (probe_wants_state(wg, k))                            // test hook: the state after this flow
            return probe_state(e, plan, dst, k == 0 ? 1 : 0, 2 * h + (early ? 2 : 0), wg.probe_out);
        if (early) zoff += 2;
    }
    return TTS_HIP_OK;
}

// Forward flow (fp32): audio [B, T*256] -> z [B, T*32, 8] in the layout waveglow_run consumes, and stats [3][B] (sum z^2, sum s,
// lens[b] * 32 * sum_k log|det kernel_k|) over each row's real positions.  Same plan, workspace, form and tail handling as
// waveglow_run, flows ascending; the position-wise kernels are wg_encode.hip's.  The end partial sums of the 512-channel fp32
// path are not used in this direction (call.endp stays null: the residual GEMMs run plain and wn_end_fwd_kernel reads the
// eight layers' activations), and the inverse direction's armed probe hooks are ignored.
// probe (tts_hip_waveglow_encode_probe, a test hook): nothing before the stop differs from the plain call; after
// wn_end_fwd_kernel of flow probe->flow (-1: after encode_init_kernel) the run copies to probe->out, natural position order,
//   what 0: the stored flow state [B, T*32, n] -- what the next flow reads, that flow's matrix already applied, n = its
//           channel count; after flow 11 nothing is stored, and the copy is z's channels 0 .. 3;
//   what 1: slog [B, T*32], the per-position sum of s through that flow
// and returns; d_stats is not written.
int waveglow_encode_run(tts_hip_engine* e, const float* d_audio, const float* d_mel, int B, int T, const int* d_lens,
                        const int* d_tail, int n_tail, float* d_z, float* d_stats, const WgEncodeProbe* probe) {
    WaveGlowDev& wg = e->wg;
    const int C = wg.channels;
    WgPlan plan = wg_plan(B * T, 0, wg.form_mode);
    if (C != 512) plan.wino_wanted = false;
    const int BT = plan.BT, PR = plan.PR;
    const long long M = plan.M;
    if ((double)M * C * 4.0 >= 2147483648.0 - 65536.0)
        return set_err(e, TTS_HIP_EINVAL, "waveglow_encode: B*T = %d frames exceeds one call's limit (~32000)", BT);
    if (int rc = ensure_workspace(e, plan, 0)) return rc;
    const size_t part_at = (size_t)M * 4;                        // enc_ws: [slog M floats | partial sums]
    HIPCHK(e, wg.enc_ws.ensure(part_at + wg_encode_stats_bytes(B)));
    float* slog = wg.enc_ws.f();
    if (d_lens)
        if (int rc = ragged_mel(e, &d_mel, d_lens, BT, T)) return rc;
    const WnTails tails{d_lens ? MASK_LENS : MASK_NONE, d_tail, n_tail};
    bool wino = plan.wino_wanted;
    if (wino)
        if (int rc = wino_begin_or_fall_back(e, plan, d_mel, T, &wino)) return rc;
    wg.last_form = wino ? 1 : 0;
    wg.last_tiles = plan.tiles;
    const WnKernels& kn = kWnKernels[0][plan.tiles];
    WnCall call = wn_call(wg, plan, 0, T, d_mel);
    call.endp = nullptr;
    if (int rc = wg_encode_init(e, d_audio, wg.flow[0].fwd, wg.audio.f(), PR, BT, d_lens, T)) return rc;
    if (probe && probe->flow < 0) return probe_state(e, plan, wg.audio.f(), 0, 8, probe->out);
    double log_det_sum = 0.0;
    for (int k = 0; k < 12; ++k) {
        const WgFlowDev& fl = wg.flow[k];
        bool stopped = false;
        if (int rc = wn_flow(e, call, kn, fl, k, wino, tails, false, &stopped)) return rc;
        log_det_sum += fl.log_det;
        const bool early = k + 1 == 4 || k + 1 == 8;             // the first two channels leave before flows 4 and 8
        WgEncodeEnd a{};
        a.C = C, a.acts = call.acts, a.layer_stride = call.acts_stride, a.wfold = fl.end_w, a.bfold = fl.end_b;
        a.state = wg.audio.f(), a.slog = slog, a.first = k == 0, a.next = k < 11 ? wg.flow[k + 1].fwd : nullptr;
        a.z = d_z, a.zoff = k + 1 == 4 ? 6 : 4, a.n_early = early ? 2 : 0;
        a.M = M, a.h = fl.n_half, a.PR = PR, a.BT = BT, a.d_lens = d_lens, a.T = T;
        if (int rc = wg_encode_end(e, a)) return rc;
        if (probe && probe->flow == k) {                         // test hook: stop here
            if (probe->what == 1) return probe_state(e, plan, slog, 0, 1, probe->out, 1);
            if (k == 11) return probe_state(e, plan, d_z, 1, 4, probe->out);
            return probe_state(e, plan, wg.audio.f(), 0, 2 * fl.n_half - a.n_early, probe->out);
        }
    }
    return wg_encode_stats(e, d_z, slog, (double*)((char*)wg.enc_ws.p + part_at), d_lens, B, T, PR, log_det_sum, d_stats);
}

// Packed call: gather the real frames of mel / z [B, T, ..] into one row of F frames (mel_ragged / packed_z), run that row as
// an ordinary one-row call whose gap frames are not real, scatter the row's audio back to [B, T * 256] with zero tails.
// d_info = [start[B] | len[B] | flags[F] | gap frames[n_gap]] (staged by the caller once per call, csrc/engine.hip).
int waveglow_run_packed(tts_hip_engine* e, const float* d_mel, int B, int T, const float* d_z, float sigma, float* d_audio,
                        int precision, const int* d_info, int F, int n_gap) {
    WaveGlowDev& wg = e->wg;
    hipStream_t st = e->stream;
    const int* d_flags = d_info + 2 * (size_t)B;
    if (F > 0) {
        HIPCHK(e, wg.mel_ragged.ensure((size_t)F * 80 * 4));
        HIPCHK(e, wg.packed_out.ensure((size_t)F * 256 * 4));
        if (d_z) HIPCHK(e, wg.packed_z.ensure((size_t)F * 256 * 4));
        hipLaunchKernelGGL(packed_gather_kernel, dim3((unsigned)(((long long)F * 20 + 255) / 256)), dim3(256), 0, st, d_mel,
                           wg.mel_ragged.f(), d_flags, F, 20);
        if (d_z)
            hipLaunchKernelGGL(packed_gather_kernel, dim3((unsigned)(((long long)F * 64 + 255) / 256)), dim3(256), 0, st, d_z,
                               wg.packed_z.f(), d_flags, F, 64);
        HIPCHK(e, hipGetLastError());
        int rc = waveglow_run(e, wg.mel_ragged.f(), 1, F, d_z ? wg.packed_z.f() : nullptr, sigma, wg.packed_out.f(), precision,
                              nullptr, d_flags + F, n_gap, d_flags);
        if (rc) return rc;
        if (wg.probe_out) return TTS_HIP_OK;                     // test hook: an armed probe stopped the run, no audio to scatter
    }
    // (no real frame at all: the scatter reads nothing of `packed` and stores the zeros)
    const long long n4 = (long long)B * T * 64;
    hipLaunchKernelGGL(packed_scatter_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                       (const float*)wg.packed_out.p, d_info, d_audio, B, T);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}
