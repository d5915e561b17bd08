// wn_wino.hip -- Winograd minimal filtering F(4,3) along the tap axis of the WN dilated convolution (fp32 path, calls of 144
// frames or more).
//
// The in-layer pre-activation of WaveGlow's WN (/root/reference/architectures/waveglow_arch.py:117-127) is a k = 3 dilated
// convolution plus the conditioning term,  y[l] = W- x[l - d] + W0 x[l] + W+ x[l + d] + c[l] + b.  The FOUR outputs
// y[l], y[l + d], y[l + 2d], y[l + 3d] share the six inputs x[l - d] ... x[l + 4d] and need only SIX K = 512 products
// instead of twelve (K per output 768 instead of 1536) on M / 4 "group rows":
//
//   input transform    U_p = sum_i BT[p][i] x_i                      (six combinations of the six inputs)
//   products           P_p = U_p G_p^T                                (G: tap combinations, built at load)
//   output transform   y_j = sum_p AT[j][p] P_p + c_j + b,  acts = tanh(.) * sigmoid(.)  written to the four output rows
//
// Round 4: ONE kernel per layer (wino4_fused2_kernel, the default form).  A block owns 64 group rows x 128 pre-activation
// columns of ALL SIX products (a wave: 32 x 64 x 6 = 192 accumulator registers).  Its K loop walks the 512 tap columns chunk by
// chunk: the six INPUT tiles of a chunk arrive by LDS-DMA with per-lane row addresses (phase carries, frame groups, zeros
// outside an utterance through out-of-range offsets), a product's A fragment is three or four input fragments combined in
// registers under the other half step's MFMAs, and the epilogue applies the output transform, conditioning plane (staged through the
// released LDS by DMA, one tile in flight behind the one being gated) and gate in registers:
// no U planes, no P planes, no pre-pass or combine launch.  Measured at config 2 on one box: three passes (round 3) 433 ms
// per step, fused GEMM behind the pre-pass 415, this 401 (direct form 565); the kernel runs the 456 GFLOP a layer executes in
// 3.62 ms (80 % of the fp32 MFMA peak INCLUDING both transforms and the gate; the per-product GEMM of round 3 alone ran at
// 85 %, its layer -- 0.19 + 3.55 + 0.27 ms -- at 74 %).  What bounds the tile: six accumulator sets leave room for 64 x 128
// per four waves at two blocks per CU (8-wave 128 x 128 blocks measured 3 % slower: one barrier domain per CU and 12.5
// rounds of 256 blocks), i.e. 12 DMA pieces per 16 MFMAs and wave -- twice the direct kernel's bytes per MFMA.
// Forms 2 and 3 (tts_hip_set_waveglow_form; measurement only, bit-identical results) keep the earlier stages: the three
// passes (wino4_prepass_kernel, one z slice of gemm_f32_kernel per product, wino4_combine_kernel) and the fused GEMM behind
// the pre-pass (wino4_fused_kernel).
//
// The conditioning term (K = 320 per output in the direct form) is not part of these kernels: whatever the dilation it is a
// 4-tap FIR along FRAMES with per-phase weights, so a second Winograd transform, F(4, 4) along frames, computes it with
// K = 140 per output in a kernel of its own (wino_cond_kernel, below: one launch per layer ahead of the in-layer kernel), which
// leaves a plane cond[32 PR][1024] (bias included) that the in-layer kernels add in their epilogue in place of the bias.  A
// layer executes K = 768 + 140 per output instead of 768 + 320 (dilations 32 / 64: + 200, the earlier F(4, 2) form).
// The first layer of a flow (taps on the flow's h <= 4 coupling channels) runs on the same K loop, with its taps, bias and gate
// in the epilogue (wino_layer0_kernel): K = 140 + 16 per output instead of 320 + 48, and no plane.
//
// Groups.  Dilation d <= 8 (sample groups): four PHASES p0 + j d of one frame, 8 group phases p0 = (gp / d) 4d + gp % d.
// d >= 32 (s = d / 32 frames): four FRAMES t0 + j s of one phase.  d = 16: two phases x two frames.  Frame groups are cut per
// utterance, so any utterance length works.
//
// Numerics: every operand stays fp32, weight / mel combinations are formed in fp64 and rounded once.  F(4,3)'s transform
// constants (4, 5, 8, 1/6, 1/24) cost accuracy: one layer's gated activations against the oracle 1.9e-6 relative RMS (direct
// form 1.4e-6; tests/test_waveglow_gpu.py), end to end 6.0e-7 waveform RMS (direct form 4.96e-7; tolerance 1e-4), with four
// times less `end` attenuation 6.5e-6 (4.9e-6).  Not bit-identical to the direct form.
#include "engine.h"
#include "gemm_f32.h"
#include "wg_plan.h"

#include <algorithm>

using namespace ttsgemm;

namespace {
constexpr int C = 512;
constexpr int NPH = 32;
constexpr int KMEL = 320;
constexpr int KCONV = 3 * C;

// x row of (phase ps -- may leave [0, 32): carried into the neighbouring frame -- , frame row f + df), zero outside the utterance
__device__ __forceinline__ f32x4 x_at(const float* __restrict__ x, int ps, long long f, int df, int c, int PR, int BT, int T) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (f >= BT) return zero;
    const int carry = (ps >> 5) + df;                  // arithmetic shift: floor
    const int t = (int)(f % T) + carry;
    if (t < 0 || t >= T) return zero;
    return *reinterpret_cast<const f32x4*>(x + ((long long)(ps & 31) * PR + f + carry) * C + c);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The transforms (Lavin & Gray's F(4,3); fp32 error ~3x the direct form's, far inside the tolerance), with the six inputs
// x_i = x[l + (i - 1) d] of the four outputs l, l + d, l + 2d, l + 3d:
//   U0 = 4 x0 - 5 x2 + x4            G0 = W- / 4                          y0 = P0 + P1 + P2 + P3 + P4
//   U1 = -4 x1 - 4 x2 + x3 + x4      G1 = -(W- + W0 + W+) / 6             y1 = P1 - P2 + 2 P3 - 2 P4
//   U2 = 4 x1 - 4 x2 - x3 + x4       G2 = -(W- - W0 + W+) / 6             y2 = P1 + P2 + 4 P3 + 4 P4
//   U3 = -2 x1 - x2 + 2 x3 + x4      G3 = W- / 24 + W0 / 12 + W+ / 6      y3 = P1 - P2 + 8 P3 - 8 P4 + P5
//   U4 = 2 x1 - x2 - 2 x3 + x4       G4 = W- / 24 - W0 / 12 + W+ / 6
//   U5 = 4 x1 - 5 x3 + x5            G5 = W+

__device__ __forceinline__ int group_phase0(int gp, int d) { return (gp / d) * 4 * d + gp % d; }

// Frame groups (dilations >= 32, s = d / 32): every utterance owns G = 4 ceil(T / 16) group rows per phase for every s, so
// that no group straddles two utterances whatever T is; group g of an utterance starts at frame t0 = (g / s) 4s + g % s and
// covers t0 + j s (frames >= T: inputs read as zero, outputs are not written; t0 >= T: an empty group).
__host__ __device__ __forceinline__ int frame_groups_per_utt(int T) { return (T + 15) / 16 * 4; }
__device__ __forceinline__ bool frame_group(int gf, int s, int BT, int T, int& b, int& t0) {
    const int G = frame_groups_per_utt(T);
    b = gf / G;
    const int g = gf % G;
    t0 = (g / s) * 4 * s + g % s;
    return (long long)b * T < BT && t0 < T;
}
// Dilation 16: the four outputs l + 16 j of a group are two phases x two frames -- (p0, t), (p0 + 16, t), (p0, t + 1),
// (p0 + 16, t + 1) for p0 < 16 and even t; every utterance owns ceil(T / 2) group rows per p0.
__host__ __device__ __forceinline__ int mixed_groups_per_utt(int T) { return (T + 1) / 2; }
__device__ __forceinline__ bool mixed_group(int gm, int BT, int T, int& b, int& t0) {
    const int G = mixed_groups_per_utt(T);
    b = gm / G;
    t0 = 2 * (gm % G);
    return (long long)b * T < BT;                          // (t0 < T always)
}
// x row of (phase p, utterance b, frame t), zero outside the utterance
__device__ __forceinline__ f32x4 x_bt(const float* __restrict__ x, int p, int b, int t, int c, int PR, int T) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (t < 0 || t >= T) return zero;
    return *reinterpret_cast<const f32x4*>(x + ((long long)p * PR + (long long)b * T + t) * C + c);
}

__global__ void wino4_prepass_kernel(const float* __restrict__ x, float* __restrict__ U, int d, int PR, int BT, int T, long long Mq) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Mq * (C / 4)) return;
    const long long mg = idx / (C / 4);
    const int c = (int)(idx % (C / 4)) * 4;
    f32x4 v[6];
    if (d == 16) {                                         // two phases x two frames (PRm group rows per p0)
        const int PRm = (int)(Mq / 16);
        const int p0 = (int)(mg / PRm);
        int b, t0;
        const bool ok = mixed_group(mg % PRm, BT, T, b, t0);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int ps = p0 + 16 * (i - 1);
            v[i] = ok ? x_bt(x, ps & 31, b, t0 + (ps >> 5), c, PR, T) : zero;
        }
    } else if (d < NPH) {                                  // four phases of one frame
        const int gp = (int)(mg / PR);
        const long long f = mg % PR;
        const int p0 = group_phase0(gp, d);
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = x_at(x, p0 + (i - 1) * d, f, 0, c, PR, BT, T);
    } else {                                               // four frames f0 + j s of one phase (PRq group rows per phase)
        const int s = d / NPH, PRq = (int)(Mq / NPH);
        const int p = (int)(mg / PRq);
        int b, t0;
        const bool ok = frame_group(mg % PRq, s, BT, T, b, t0);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = ok ? x_bt(x, p, b, t0 + (i - 1) * s, c, PR, T) : zero;
    }
    const long long o = mg * C + c, plane = Mq * C;
    *reinterpret_cast<f32x4*>(U + o) = 4.f * v[0] - 5.f * v[2] + v[4];
    *reinterpret_cast<f32x4*>(U + plane + o) = -4.f * (v[1] + v[2]) + v[3] + v[4];
    *reinterpret_cast<f32x4*>(U + 2 * plane + o) = 4.f * (v[1] - v[2]) - v[3] + v[4];
    *reinterpret_cast<f32x4*>(U + 3 * plane + o) = 2.f * (v[3] - v[1]) - v[2] + v[4];
    *reinterpret_cast<f32x4*>(U + 4 * plane + o) = 2.f * (v[1] - v[3]) - v[2] + v[4];
    *reinterpret_cast<f32x4*>(U + 5 * plane + o) = 4.f * v[1] - 5.f * v[3] + v[5];
}

__global__ void wino4_weights_kernel(const float* __restrict__ in_Bt, float* __restrict__ G) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * C * C) return;
    const int n = idx / C, c = idx % C;
    const float* row = in_Bt + (long long)n * KCONV + (c / 16) * 48 + c % 16;
    const double wm = row[0], w0 = row[16], wp = row[32];
    const long long plane = (long long)2 * C * C;
    G[idx] = (float)(wm / 4.0);
    G[plane + idx] = (float)(-(wm + w0 + wp) / 6.0);
    G[2 * plane + idx] = (float)(-(wm - w0 + wp) / 6.0);
    G[3 * plane + idx] = (float)(wm / 24.0 + w0 / 12.0 + wp / 6.0);
    G[4 * plane + idx] = (float)(wm / 24.0 - w0 / 12.0 + wp / 6.0);
    G[5 * plane + idx] = (float)wp;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The conditioning term.  For every phase p and layer it is a 4-tap FIR along frames with per-phase weights, whatever the
// dilation:  cond[p, t] = sum_q V_{p,q} mel[t - q]  (V_{p,q}: the 80-column slice q of cond_Bt[p], 1024 x 80), so four
// consecutive frames t0 .. t0 + 3 of one phase share the seven mel frames d_i = mel[t0 - 3 + i] and Winograd F(4, 4) computes
// them with SEVEN K = 80 products instead of sixteen (K = 140 per output instead of 320):
//   y_j = sum_q' g_q' d_{j + q'},  g_q' = V_{p, 3 - q'}       y = AT [(G g) . (BT d)]
// with the evaluation matrix E_k of the points 0, 1, -1, 2, -2, 1/2, -1/2 (row i = [1, a_i, ..., a_i^(k - 1)]):  G = E_4,
// AT = E_4^T, BT = (E_7^-1)^T.  The weight planes W_{p,x} = sum_q G[x][3 - q] V_{p,q} are built at load ([32][7][1024][80],
// 73 MB per layer), the mel planes Z_x = BT d once per call ([7][groups][80]: the same for every phase, layer and flow; every
// utterance owns ceil(T / 4) groups, frames outside it read as zero), and ONE kernel per layer (wino_cond_kernel) runs the
// seven products of a (phase, 64 groups, 64 columns) tile into seven accumulator sets, applies AT in registers, adds the
// in-layer bias and stores the plane cond[p PR + b T + t][1024] that the in-layer kernels add in place of the bias.
// Both are formed in fp64 and rounded once.  (fp32 model, i.i.d. mel frames in U(-11.5, 1.2): 4.4e-7 relative RMS of the
// conditioning, the direct K = 320 sum 1.7e-7.)
constexpr int NPT = 7, NMEL = 80;
__constant__ double C44_G[7][4] = {{1., 0., 0., 0.},
                                   {1., 1., 1., 1.},
                                   {1., -1., 1., -1.},
                                   {1., 2., 4., 8.},
                                   {1., -2., 4., -8.},
                                   {1., 1. / 2, 1. / 4, 1. / 8},
                                   {1., -1. / 2, 1. / 4, -1. / 8}};
__constant__ double C44_BT[7][7] = {{1., 0., -21. / 4, 0., 21. / 4, 0., -1.},
                                    {0., -2. / 9, -2. / 9, 17. / 18, 17. / 18, -2. / 9, -2. / 9},
                                    {0., 2. / 9, -2. / 9, -17. / 18, 17. / 18, 2. / 9, -2. / 9},
                                    {0., 1. / 180, 1. / 360, -1. / 36, -1. / 72, 1. / 45, 1. / 90},
                                    {0., -1. / 180, 1. / 360, 1. / 36, -1. / 72, -1. / 45, 1. / 90},
                                    {0., 64. / 45, 128. / 45, -16. / 9, -32. / 9, 16. / 45, 32. / 45},
                                    {0., -64. / 45, 128. / 45, 16. / 9, -32. / 9, -16. / 45, 32. / 45}};
// (the output transform AT = [1, a, a^2, a^3] per point is written out in wino_cond_kernel's epilogue)

// ---- Record of the scheme the plane replaced, kept because tests/test_wino_frame_fir.py restates it
// from this file: until the plane the conditioning ran INSIDE the tap kernels, as extra K chunks of the six products -- three K
// slices A / B / C of the 320 columns spread over product subsets (phase groups, dilation 128), the whole K = 320 on products
// 1 .. 4 (dilation 16), and for dilations 32 / 64 a frame-axis F(4, 2) at the points 0, 1, -1, 2, -2 of the tap transform whose
// five products were added into the tap products of the same points.  Nothing below is launched or read by the engine: the
// constants and the chunk words are what that scheme used, so that its algebra and its 272 / 242 K steps per tile stay checked
// against the numbers DESIGN.md quotes for it.
constexpr int K4 = 224, SA = 112, SB = 96, SC = 112;       // conditioning K of a product; slice widths (A, B, C)
constexpr int KF = 160;                                    // conditioning K of a product, F(4, 2) layers
[[maybe_unused]] __constant__ double FIR_X[5] = {0, 1, -1, 2, -2};
[[maybe_unused]] __constant__ double FIR_BT[5][5] = {{1, 0, -5. / 4, 0, 1. / 4},
                                                     {0, 2. / 3, 2. / 3, -1. / 6, -1. / 6},
                                                     {0, -2. / 3, 2. / 3, 1. / 6, -1. / 6},
                                                     {0, -1. / 12, -1. / 24, 1. / 12, 1. / 24},
                                                     {0, 1. / 12, -1. / 24, -1. / 12, 1. / 24}};
__host__ __device__ __forceinline__ int fir_qb(int s, int half) { return s == 1 ? 2 * half + 1 : half + 2; }   // older tap of a half
// product p's conditioning chunks (16 columns each), 16 bits per product (p < 4: cfg_lo): n1 | b1 << 5 | n2 << 9 | b2 << 12 --
// operand chunks 0 .. n1 + n2 - 1 against weight chunks b1 .. b1 + n1 - 1, then b2 .. b2 + n2 - 1
struct InKernelCondChunks {
    unsigned long long cfg_lo = 0, cfg_hi = 0;
};
inline InKernelCondChunks in_kernel_cond_chunks(bool phases, bool mixed, bool fir) {
    InKernelCondChunks a;
    unsigned ccfg[6] = {0, 0, 0, 0, 0, 0};
    auto cc = [](unsigned n1, unsigned b1, unsigned n2 = 0, unsigned b2 = 0) { return n1 | b1 << 5 | n2 << 9 | b2 << 12; };
    if (phases) {                                          // [A | B | 0], [A | C], [B | C | 0] of K4 columns
        for (int p = 0; p < 6; ++p) ccfg[p] = cc(p == 1 || p == 2 ? K4 / 16 : (SA + SB) / 16, 0);
    } else if (mixed) {                                    // products 1 .. 4: K = 320
        for (int p = 1; p < 5; ++p) ccfg[p] = cc(KMEL / 16, 0);
    } else if (fir) {                                      // frame groups, s = 1, 2: products 0 .. 4, K = 160
        for (int p = 0; p < 5; ++p) ccfg[p] = cc(KF / 16, 0);
    } else {                                               // frame groups, s = 4: chunk ranges of cond_Bt's 320 columns
        ccfg[0] = ccfg[5] = cc((SA + SB) / 16, 0);                         // [A | B]
        ccfg[1] = ccfg[2] = cc(SA / 16, 0, SC / 16, (SA + SB) / 16);       // [A | C]
        ccfg[3] = ccfg[4] = cc((SB + SC) / 16, SA / 16);                   // [B | C]
    }
    for (int p = 0; p < 6; ++p) (p < 4 ? a.cfg_lo : a.cfg_hi) |= (unsigned long long)ccfg[p] << (16 * (p & 3));
    return a;
}

__host__ __device__ __forceinline__ int cond_groups_per_utt(int T) { return (T + 3) / 4; }

// W[32][7][1024][80] from cond_Bt [32][1024][320] (rows keep cond_Bt's gate-interleaved order)
__global__ void wino_cond_weights_kernel(const float* __restrict__ cond_Bt, float* __restrict__ W) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)NPH * NPT * 2 * C * NMEL) return;
    const int c = (int)(idx % NMEL), n = (int)((idx / NMEL) % (2 * C)), x = (int)((idx / ((long long)NMEL * 2 * C)) % NPT),
              p = (int)(idx / ((long long)NMEL * 2 * C * NPT));
    const float* row = cond_Bt + ((long long)p * 2 * C + n) * KMEL + c;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc += C44_G[x][3 - q] * (double)row[q * NMEL];
    W[idx] = (float)acc;
}

// mel planes Z[7][rows][80]: group row gr <-> frames t0 .. t0 + 3 of its utterance, t0 = 4 (gr % ceil(T / 4))
__global__ void wino_cond_mel_planes_kernel(const float* __restrict__ mel, float* __restrict__ Z, int rows, int BT, int T) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)NPT * rows * NMEL) return;
    const int c = (int)(idx % NMEL), gr = (int)((idx / NMEL) % rows), x = (int)(idx / ((long long)rows * NMEL));
    const int G = cond_groups_per_utt(T), b = gr / G, t0 = 4 * (gr % G);
    double acc = 0.0;
    if ((long long)b * T < BT) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int t = t0 - 3 + i;
            if (t >= 0 && t < T) acc += C44_BT[x][i] * (double)mel[((long long)b * T + t) * NMEL + c];
        }
    }
    Z[idx] = (float)acc;
}

// group row -> its frames, for wino_cond_kernel's stores: (b T + t0) | (number of the frames t0 .. t0 + 3 inside the utterance) << 16
// (0 for the padding rows; b T + t0 < 2^15)
__global__ void wino_cond_rows_kernel(int* __restrict__ tab, int rows, int BT, int T) {
    const int gr = blockIdx.x * blockDim.x + threadIdx.x;
    if (gr >= rows) return;
    const int G = cond_groups_per_utt(T), b = gr / G, t0 = 4 * (gr % G);
    const int left = T - t0;
    tab[gr] = (long long)b * T < BT ? (b * T + t0) | (left < 4 ? left : 4) << 16 : 0;
}

// The seven products of one layer.  A block owns BM = 32 WR group rows x BN = 32 WC columns of one phase (a wave: 32 x 32 x 7 =
// 112 accumulator registers); its K loop walks point after point (5 chunks of 16 columns each) through one LDS-DMA pipeline
// (the tile stream and the half-step rotation of wino4_fused_kernel below).  Blocks are ordered so that the row tiles of one
// (phase, column tile) run back to back on one XCD: its weight panel (7 x BN x 80 floats) is fetched from HBM once.
struct WinoCondArgs {
    const float* Z;                    // mel planes [7][rows][80]
    const int* rowtab;                 // [rows] (wino_cond_rows_kernel)
    const float* W;                    // weight planes [32][7][1024][80]
    const float* bias;                 // [1024] (gate-permuted like the weight rows)
    float* cond;                       // [32 PR][1024]
    int rows;                          // group rows (a multiple of BM)
    int PR, BT, T;
    // first layer of a flow (wino_layer0_kernel) only: no plane, the gated activations instead
    const float* taps;                 // tap operand [32 PR][16] (wino_tap_operand_kernel)
    const float* Wt;                   // tap weights [1024][16], rows in W's order (wino_tap_weights_kernel)
    float* acts;                       // [32 PR][512]
};

// The first layer of a flow.  Its taps act on the flow's h <= 4 coupling channels (the start conv is composed into them at
// load time), so its whole pre-activation is the conditioning FIR plus a K <= 15 product per position: the plane kernel's K loop
// on the layer's own weight planes, and an epilogue that adds the tap term by one K = 16 MFMA chunk per output frame, adds the
// bias, gates and stores acts -- no plane, no K = 320 + 48 GEMM.
// Tap operand: one 16-float row per position, [a(n-1)[0..h), v(n-1) | a(n)[0..h), v(n) | a(n+1)[0..h), v(n+1) | 0 ..], copied
// from the a0p rows of the three positions (wn_tap_row, wg_plan.h; after the tail rows of a0p were cleared), zeros for a
// neighbour outside the utterance; tap weights: the matching columns of the composed in_Bt [1024][3 x 16].
__global__ void wino_tap_operand_kernel(const float* __restrict__ a0p, float* __restrict__ taps, int h, int PR, int BT, int T) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)NPH * PR * 16) return;
    const int k = (int)(idx & 15);
    const long long m = idx >> 4;
    const int tap = wn_tap_of_col(k, h);
    const long long src = tap < 3 ? wn_tap_row((int)(m / PR), (int)(m % PR), tap - 1, PR, BT, T) : -1;
    taps[idx] = src >= 0 ? a0p[src * 16 + wn_tap_src_col(k, h)] : 0.f;
}
__global__ void wino_tap_weights_kernel(const float* __restrict__ in_Bt0, float* __restrict__ Wt, int h) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * C * 16) return;
    const int k = idx & 15, tap = wn_tap_of_col(k, h);
    Wt[idx] = tap < 3 ? in_Bt0[(idx >> 4) * 48 + tap * 16 + wn_tap_src_col(k, h)] : 0.f;
}

// (the body of both kernels; L0: the first layer of a flow)
template <int WR, int WC, int NBUF, bool L0>
__device__ __forceinline__ void wino_cond_body(const WinoCondArgs& g) {
    constexpr int NW = WR * WC, BM = WR * 32, BN = WC * 32;
    constexpr int NPA = BM / 16, NPB = BN / 16, PPW = (NPA + NPB) / NW;     // 16-row DMA pieces: A side, B side, per wave
    static_assert((NPA + NPB) % NW == 0 && PPW <= 4, "the pieces of a tile divide among the waves, one per MFMA of a half step");
    constexpr int STAGE = (BM + BN) * 16;                                   // floats per LDS buffer: [A rows | B rows] x 16 k
    constexpr int NKC = NMEL / 16, NT = NPT * NKC;                          // chunks per point, tiles per block
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int li = lane & 31, lh = lane >> 5;

    constexpr int numNt = 2 * C / BN;
    const int numMt = g.rows / BM;
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int pair = (slot / numMt) * 8 + xcd, mt = slot % numMt;           // (32 numNt pairs: a multiple of 8)
    const int ph = pair / numNt, nt = pair % numNt;
    const int m0 = mt * BM, n0 = nt * BN;

    f32x16 acc[NPT];
#pragma unroll
    for (int p = 0; p < NPT; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;

    // ---- tile stream (as wino4_fused_kernel): piece q < NPA = 16 operand rows, else 16 weight rows; lane l fetches chunk
    // (l & 3) ^ ((l >> 4) & 3) of row l >> 2
    const int prow = lane >> 2, chunk = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned vo0[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int q = wave * PPW + i;
        const int row = (q < NPA ? q : q - NPA) * 16 + prow;
        vo0[i] = (unsigned)((row * NMEL + chunk * 4) * 4);
    }
    const float* const abase = g.Z + (long long)m0 * NMEL;
    const float* const bbase = g.W + ((long long)ph * NPT * 2 * C + n0) * NMEL;
    const long long zplane = (long long)g.rows * NMEL, wplane = (long long)2 * C * NMEL;
    int lt = 0;                                                             // the next tile to request
    unsigned vo[PPW], ko = 0;
    const float* pb[PPW];
    auto prepare = [&]() {
        const bool live = lt < NT;                                          // past the last tile the pieces fetch nothing
        const int x = live ? lt / NKC : 0, kc = live ? lt % NKC : 0;
        ko = (unsigned)kc * 64u;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const bool isA = wave * PPW + i < NPA;                          // wave-uniform
            pb[i] = isA ? abase + x * zplane : bbase + x * wplane;
            vo[i] = live ? vo0[i] : OOB;
        }
        ++lt;
    };
    auto issue_piece = [&](int i, int buf) {
        const unsigned voff = vo[i], koff = ko;                             // (by-value copies: see wino4_fused_kernel)
        const float* base = pb[i];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(make_rsrc_uniform(base), (lds_ptr_t)(smem + buf * STAGE + (wave * PPW + i) * 256), 16,
                                                 voff, koff, 0, 0);
    };
    const int xr = (li >> 2) & 3;
    struct Frag {
        f32x4 a, b;
    };
    auto read_frag = [&](int buf, int k8, Frag& f) {
        const int koff = ((2 * k8 + lh) ^ xr) * 4;
        f.a = *reinterpret_cast<const f32x4*>(smem + buf * STAGE + (wr * 32 + li) * 16 + koff);
        f.b = *reinterpret_cast<const f32x4*>(smem + buf * STAGE + BM * 16 + (wc * 32 + li) * 16 + koff);
    };

#pragma unroll
    for (int b = 0; b < NBUF; ++b) {
        prepare();
#pragma unroll
        for (int i = 0; i < PPW; ++i) issue_piece(i, b);
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NBUF - 1)) : "memory");
    __builtin_amdgcn_s_barrier();
    Frag f0, f1;
    read_frag(0, 0, f0);
    int buf = 0;
    static_for<NPT>([&](auto pc) {
        constexpr int P = decltype(pc)::value;
        for (int s = 0; s < NKC; ++s) {
            read_frag(buf, 1, f1);
            prepare();
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[P] = __builtin_amdgcn_mfma_f32_32x32x2f32(f0.a[kk], f0.b[kk], acc[P], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PPW * (NBUF - 2)) : "memory");
            __builtin_amdgcn_s_barrier();
            const int bufn = buf == NBUF - 1 ? 0 : buf + 1;
            read_frag(bufn, 0, f0);                                         // (past the last tile: zeros nothing uses)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                acc[P] = __builtin_amdgcn_mfma_f32_32x32x2f32(f1.a[kk], f1.b[kk], acc[P], 0, 0, 0);
                if (kk < PPW) {
                    issue_piece(kk, buf);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            buf = bufn;
        }
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the fetch-nothing pieces of the last steps

    // ---- epilogue: output transform + bias; lane (li, lh) holds column li of the 16 group rows (r & 3) + 8 (r >> 2) + 4 lh.
    // The phase block and the tile's first column go into the descriptor, a row's frame and the lane's column into a 32-bit
    // offset, the output's frame step into the scalar offset; frames past the end of the utterance: out-of-range offset, no store
    const float bv = g.bias[n0 + wc * 32 + li];
    const int* const rt = g.rowtab + m0 + wr * 32 + 4 * lh;
    if constexpr (!L0) {
        const __amdgpu_buffer_rsrc_t ro = make_rsrc_uniform(g.cond + (long long)ph * g.PR * (2 * C) + n0 + wc * 32);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int info = rt[(r & 3) + 8 * (r >> 2)];
            const unsigned voff = ((unsigned)(info & 0xffff) * (2 * C) + li) * 4u;
            const int nout = info >> 16;
            const float s12 = acc[1][r] + acc[2][r], d12 = acc[1][r] - acc[2][r];
            const float s34 = acc[3][r] + acc[4][r], d34 = acc[3][r] - acc[4][r];
            const float s56 = acc[5][r] + acc[6][r], d56 = acc[5][r] - acc[6][r];
            float y[4];
            y[0] = acc[0][r] + s12 + s34 + s56 + bv;
            y[1] = d12 + 2.f * d34 + 0.5f * d56 + bv;
            y[2] = s12 + 4.f * s34 + 0.25f * s56 + bv;
            y[3] = d12 + 8.f * d34 + 0.125f * d56 + bv;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[j]), ro, j < nout ? voff : OOB, j * (2 * C * 4), 0);
        }
    } else {
        static_assert(WC == 2, "waves (wr, 0) and (wr, 1) hold the tanh and the sigmoid half of the same 32 channels");
        // the tap term's operands: as an MFMA A row, lane (li, lh) holds columns 8 lh .. 8 lh + 7 of the operand row of group
        // row li's frame j (a frame past the utterance, a padding row: zeros through an out-of-range offset), as a B row the
        // same columns of its own weight row -- K step kk of the chunk is column 8 lh + kk on both sides
        const int arow = g.rowtab[m0 + wr * 32 + li];
        const __amdgpu_buffer_rsrc_t rta = make_rsrc_uniform(g.taps + (long long)ph * g.PR * 16);
        f32x4 ta[4][2], tb[2];
        auto load_taps = [&](int j) {
            const unsigned off = j < arow >> 16 ? ((unsigned)(arow & 0xffff) + j) * 64u + lh * 32u : OOB;
            ta[j][0] = buf_load4(rta, off);
            ta[j][1] = buf_load4(rta, off + 16u);
        };
        load_taps(0);                                                       // (frames 2, 3 once sets 4 .. 6 are free: register budget)
        load_taps(1);
        tb[0] = *reinterpret_cast<const f32x4*>(g.Wt + (n0 + wc * 32 + li) * 16 + lh * 8);
        tb[1] = *reinterpret_cast<const f32x4*>(g.Wt + (n0 + wc * 32 + li) * 16 + lh * 8 + 4);
        // output transform in place: frames 0 .. 3 into accumulator sets 0 .. 3 (sets 4 .. 6 are free from here on)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s12 = acc[1][r] + acc[2][r], d12 = acc[1][r] - acc[2][r];
            const float s34 = acc[3][r] + acc[4][r], d34 = acc[3][r] - acc[4][r];
            const float s56 = acc[5][r] + acc[6][r], d56 = acc[5][r] - acc[6][r];
            acc[0][r] = acc[0][r] + s12 + s34 + s56;
            acc[1][r] = d12 + 2.f * d34 + 0.5f * d56;
            acc[2][r] = s12 + 4.f * s34 + 0.25f * s56;
            acc[3][r] = d12 + 8.f * d34 + 0.125f * d56;
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);            // (four rows' temporaries at a time: register budget)
        }
        load_taps(2);
        load_taps(3);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[j][kk >> 2][kk & 3], tb[kk >> 2][kk & 3], acc[j], 0, 0, 0);
        // gate: the tanh wave (wc 0) gates frames 0, 1 and hands its frames 2, 3 to the sigmoid wave (wc 1), which hands over
        // its frames 0, 1 -- 32 values per lane through the released pipeline LDS, register index major (32 consecutive floats
        // per half wave: no bank conflict).  Every wave has passed its vmcnt(0) before the barrier: no DMA piece (the fetch-
        // nothing ones land zeros) is still on its way into the LDS that is written here.
        float* const give = smem + wave * (32 * 64) + lane;
        const float* const take = smem + (wave ^ 1) * (32 * 64) + lane;
        __builtin_amdgcn_s_barrier();
        auto hand_over = [&](auto jc) {                                     // JG: the first of the two frames given away
            constexpr int JG = decltype(jc)::value;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int r = 0; r < 16; ++r) give[(jj * 16 + r) * 64] = acc[JG + jj][r] + bv;
        };
        auto gate_store = [&](auto jc) {                                    // JK: the first of the two frames kept
            constexpr int JK = decltype(jc)::value;
            const __amdgpu_buffer_rsrc_t ro = make_rsrc_uniform(g.acts + (long long)ph * g.PR * C + (n0 >> 6) * 32);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int info = rt[(r & 3) + 8 * (r >> 2)];
                const unsigned voff = ((unsigned)(info & 0xffff) * C + li) * 4u;
                const int nout = info >> 16;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const float mine = acc[JK + jj][r] + bv, other = take[(jj * 16 + r) * 64];
                    const float v = JK == 0 ? gate_tanh_sigmoid(mine, other) : gate_tanh_sigmoid(other, mine);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, JK + jj < nout ? voff : OOB,
                                                          (JK + jj) * (C * 4), 0);
                }
            }
        };
        if (wc == 0) hand_over(std::integral_constant<int, 2>{});
        else hand_over(std::integral_constant<int, 0>{});
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wc == 0) gate_store(std::integral_constant<int, 0>{});
        else gate_store(std::integral_constant<int, 2>{});
    }
}

template <int WR, int WC, int NBUF, int OCC>
__global__ __launch_bounds__(WR * WC * 64, OCC) void wino_cond_kernel(const WinoCondArgs g) {
    wino_cond_body<WR, WC, NBUF, false>(g);
}
template <int WR, int WC, int NBUF, int OCC>
__global__ __launch_bounds__(WR * WC * 64, OCC) void wino_layer0_kernel(const WinoCondArgs g) {
    wino_cond_body<WR, WC, NBUF, true>(g);
}

template <int WR, int WC, int NBUF, int OCC, bool L0 = false>
hipError_t launch_wino_cond(const WinoCondArgs& a, hipStream_t st) {
    constexpr int BM = WR * 32, BN = WC * 32;
    // (first layer: the gate's exchange, 32 floats per lane, needs more than the pipeline's three buffers)
    const size_t lds = std::max((size_t)NBUF * (BM + BN) * 16, L0 ? (size_t)WR * WC * 32 * 64 : (size_t)0) * sizeof(float);
    if (a.rows % BM != 0) return hipErrorInvalidValue;
    auto kern = L0 ? wino_layer0_kernel<WR, WC, NBUF, OCC> : wino_cond_kernel<WR, WC, NBUF, OCC>;
    static PerDeviceOnce attr_set;
    if (hipError_t e = set_max_dyn_lds_once((const void*)kern, lds, attr_set); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(NPH * (2 * C / BN) * (a.rows / BM))), dim3(WR * WC * 64), lds, st, a);
    return hipGetLastError();
}

// Output rows of group row gl (inside its (group) phase block) in `acts` and in the conditioning plane: output j is row
// jbase(j) + (pack & 0xfffff) and exists iff jstep(j) < pack >> 20 (block-uniform jbase / jstep: group_out_base)
__device__ __forceinline__ unsigned group_out_pack(int kind, int gl, int sfr, int BT, int T) {
    if (kind == 0) return (unsigned)gl | 15u << 20;                         // four phases of one frame row (padding rows included)
    int b, t0;
    const bool ok = kind == 1 ? frame_group(gl, sfr, BT, T, b, t0) : mixed_group(gl, BT, T, b, t0);
    if (!ok) return 0u;
    const int left = T - t0;                                                // frames from t0 to the end of the utterance
    return (unsigned)(b * T + t0) | (unsigned)(left < 15 ? left : 15) << 20;
}
__device__ __forceinline__ long long group_out_base(int kind, int ph, int j, int d, int PR, unsigned& jstep) {
    if (kind == 0) {
        jstep = 0;
        return (long long)(group_phase0(ph, d) + j * d) * PR;
    }
    if (kind == 1) {
        jstep = (unsigned)(j * (d / NPH));
        return (long long)ph * PR + j * (d / NPH);
    }
    jstep = (unsigned)(j >> 1);
    return (long long)(ph + 16 * (j & 1)) * PR + (j >> 1);
}

__global__ void wino4_combine_kernel(const float* __restrict__ P, const float* __restrict__ cond, float* __restrict__ acts, int d,
                                     int PR, int BT, int T, long long Mq) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Mq * (C / 4)) return;
    const long long mg = idx / (C / 4);
    const int ch = (int)(idx % (C / 4)) * 4;
    const int col = (ch >> 5) * 64 + (ch & 31);
    const long long plane = Mq * 2 * C, o = mg * 2 * C + col;
    f32x4 a[6], b[6];
#pragma unroll
    for (int z = 0; z < 6; ++z) {
        a[z] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + z * plane + o));
        b[z] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + z * plane + o + 32));
    }
    // group row -> (group) phase block, row inside it: phase groups 8 x PR, mixed groups 16 x PRm, frame groups 32 x PRq
    const int kind = d == 16 ? 2 : d < NPH ? 0 : 1;
    const int prows = kind == 0 ? PR : (int)(Mq / (kind == 2 ? 16 : NPH));
    const int ph = (int)(mg / prows);
    const unsigned pack = group_out_pack(kind, (int)(mg % prows), d / NPH, BT, T);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned jstep;
        const long long row = group_out_base(kind, ph, j, d, PR, jstep) + (pack & 0xfffffu);
        if (jstep >= pack >> 20) break;                    // (padding / empty group, frames past the end of the utterance)
        const f32x4 ca = *reinterpret_cast<const f32x4*>(cond + row * (2 * C) + col);
        const f32x4 cb = *reinterpret_cast<const f32x4*>(cond + row * (2 * C) + col + 32);
        f32x4 t, s;
        if (j == 0) {
            t = a[0] + a[1] + a[2] + a[3] + a[4] + ca;
            s = b[0] + b[1] + b[2] + b[3] + b[4] + cb;
        } else if (j == 1) {
            t = a[1] - a[2] + 2.f * (a[3] - a[4]) + ca;
            s = b[1] - b[2] + 2.f * (b[3] - b[4]) + cb;
        } else if (j == 2) {
            t = a[1] + a[2] + 4.f * (a[3] + a[4]) + ca;
            s = b[1] + b[2] + 4.f * (b[3] + b[4]) + cb;
        } else {
            t = a[1] - a[2] + 8.f * (a[3] - a[4]) + a[5] + ca;
            s = b[1] - b[2] + 8.f * (b[3] - b[4]) + b[5] + cb;
        }
        f32x4 g;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gate_tanh_sigmoid(t[k], s[k]);
        *reinterpret_cast<f32x4*>(acts + row * C + ch) = g;
    }
}

// Epilogue of wino4_fused_kernel (form 3; the default kernel's is wino_gate_store_dma below, same arithmetic): output transform
// + conditioning plane + gate in registers (the arithmetic of
// wino4_combine_kernel, written identically), each gated 32 x 32 tile transposed through a wave-private LDS patch (32 x 36
// floats) so that a lane stores 16 bytes of one acts row.  A wave holds group rows gl0 .. gl0 + 31 of (group) phase block ph and
// pre-activation columns col0 .. col0 + 63 (tanh half | sigmoid half); lane (li, lh) of an accumulator holds column li of the
// rows (r & 3) + 8 (r >> 2) + 4 lh and reads its conditioning values there: 32 lanes x 4 bytes of one plane row per request.
__device__ __forceinline__ void wino_gate_store(const f32x16 (&acc)[6][2], float* patch, const float* __restrict__ cond,
                                                float* __restrict__ acts, int kind, int d, int ph, int gl0, int col0, int PR, int BT,
                                                int T, int lane) {
    const int li = lane & 31, lh = lane >> 5, er = lane >> 3, ec4 = (lane & 7) * 4;
    const int sfr = d / NPH;
    const int ch0 = (col0 >> 6) * 32 + ec4;
    unsigned orow[16];                                                      // output rows of the accumulator rows
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        orow[r] = group_out_pack(kind, gl0 + (r & 3) + 8 * (r >> 2) + 4 * lh, sfr, BT, T);
        __builtin_amdgcn_sched_barrier(0);                                  // (one division's temporaries at a time: register budget)
    }
    static_for<4>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        unsigned jstep;
        const long long jb = group_out_base(kind, ph, j, d, PR, jstep);
        // plane row jb (block-uniform) goes into the descriptor, the lane's row and column into a 32-bit offset (rows < 2^15)
        const __amdgpu_buffer_rsrc_t rc = make_rsrc_uniform(cond + jb * (2 * C) + col0);
        // the plane reads of an output go out together, ahead of the arithmetic (output 0, with all six accumulator sets still
        // live, in two rounds: register budget)
        constexpr int RB = j == 0 ? 8 : 16;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += RB) {
            float ctv[RB], csv[RB];
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
                // (no such output: reads as zero through an out-of-range offset; nothing is stored either)
                const unsigned pk = orow[r0 + rr];
                const unsigned off = jstep < pk >> 20 ? ((pk & 0xfffffu) * (2 * C) + li) * 4u : OOB;
                ctv[rr] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rc, off, 0, 0));
                csv[rr] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rc, off, 128, 0));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
                const int r = r0 + rr;
                const float ct = ctv[rr], cs = csv[rr];
                float tv, sv;
                if constexpr (j == 0) {
                    tv = acc[0][0][r] + acc[1][0][r] + acc[2][0][r] + acc[3][0][r] + acc[4][0][r] + ct;
                    sv = acc[0][1][r] + acc[1][1][r] + acc[2][1][r] + acc[3][1][r] + acc[4][1][r] + cs;
                } else if constexpr (j == 1) {
                    tv = acc[1][0][r] - acc[2][0][r] + 2.f * (acc[3][0][r] - acc[4][0][r]) + ct;
                    sv = acc[1][1][r] - acc[2][1][r] + 2.f * (acc[3][1][r] - acc[4][1][r]) + cs;
                } else if constexpr (j == 2) {
                    tv = acc[1][0][r] + acc[2][0][r] + 4.f * (acc[3][0][r] + acc[4][0][r]) + ct;
                    sv = acc[1][1][r] + acc[2][1][r] + 4.f * (acc[3][1][r] + acc[4][1][r]) + cs;
                } else {
                    tv = acc[1][0][r] - acc[2][0][r] + 8.f * (acc[3][0][r] - acc[4][0][r]) + acc[5][0][r] + ct;
                    sv = acc[1][1][r] - acc[2][1][r] + 8.f * (acc[3][1][r] - acc[4][1][r]) + acc[5][1][r] + cs;
                }
                patch[((r & 3) + 8 * (r >> 2) + 4 * lh) * 36 + li] = gate_tanh_sigmoid(tv, sv);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // wave-private patch: no barrier needed
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(patch + (er + 8 * qq) * 36 + ec4);
            const unsigned srow = group_out_pack(kind, gl0 + er + 8 * qq, sfr, BT, T);
            if (jstep < srow >> 20) *reinterpret_cast<f32x4*>(acts + (jb + (srow & 0xfffffu)) * C + ch0) = v;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // patch reads done before the next output overwrites it
    });
}

// The same epilogue for wino4_fused2_kernel, with the conditioning tile staged through LDS by DMA instead of fetched into
// registers (128 four-byte loads per wave in five dependent rounds, each an exposed round trip at two waves per SIMD).  After the
// K loop the pipeline's LDS is dead; a wave owns 16 KB of it: two slots of one output's tile, 32 rows x 64 columns (256 B:
// tanh half | sigmoid half).  One DMA instruction fetches four rows -- lane l: 16-byte piece l & 15 of row 4 k + (l >> 4), the
// row's plane row in the per-lane offset (group_out_pack), a missing output out of range: its rows land as zeros, the value the
// register path read -- so an output is 8 instructions.  Outputs 0 and 1 are requested at once and output j + 2 when slot j & 1
// is consumed: one tile is always in flight behind the one being gated.  The gated value overwrites its own (consumed) tanh
// element, and the rows are read back 16 bytes per lane for the store: no separate transpose patch.  Rows with bit 1 set keep
// their halves swapped (through the source piece, wino_stage_piece), which spreads the four rows of a ds_read_b128 lane group
// over all 64 banks; the 4-byte accesses are 32 consecutive floats per half wave either way.
// Ordering is by count alone (wave-private slots: no barrier).  Every request and every store below is issued unconditionally
// (stores of missing rows go out of range), so the wave's queue is  t0 t1 | t2 s0 | t3 s1 | s2 | s3  (t = 8 requests, s = 4
// stores) and the wait for tile j allows the younger ones to stay outstanding.  The compiler's spill stores and reloads
// (14 registers of outputs 1 and 3, scratch) count on vmcnt too: they only add entries ahead of a wait or drain the queue early,
// which makes a wait stricter, never weaker -- safe, at the price of some of the overlap in outputs 2 and 3.
__host__ __device__ constexpr int wino_stage_row(int k, int lane) { return 4 * k + (lane >> 4); }                 // tile row of request k
__host__ __device__ constexpr int wino_stage_piece(int lane) { return (lane & 15) ^ (((lane >> 5) & 1) << 3); }   // its source piece
// float offset inside a slot of tile element (row, col) [col < 32: tanh half, else sigmoid half]
__host__ __device__ constexpr int wino_stage_at(int row, int col) { return row * 64 + (col ^ (((row >> 1) & 1) << 5)); }

__device__ __forceinline__ void wino_gate_store_dma(const f32x16 (&acc)[6][2], float* stage, const float* __restrict__ cond,
                                                    float* __restrict__ acts, int kind, int d, int ph, int gl0, int col0, int PR,
                                                    int BT, int T, int lane) {
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    constexpr int TILE = 32 * 64;                                           // floats per slot
    const int li = lane & 31, lh = lane >> 5, er = lane >> 3, ec4 = (lane & 7) * 4;
    const int sfr = d / NPH;
    unsigned drow[8], srow[4];                                              // output rows of the rows this lane requests / stores
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        drow[k] = group_out_pack(kind, gl0 + wino_stage_row(k, lane), sfr, BT, T);
        __builtin_amdgcn_sched_barrier(0);                                  // (one division's temporaries at a time: register budget)
    }
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        srow[qq] = group_out_pack(kind, gl0 + er + 8 * qq, sfr, BT, T);
        __builtin_amdgcn_sched_barrier(0);
    }
    const unsigned dcol = (unsigned)wino_stage_piece(lane) * 16u;
    auto request = [&](auto jc) {                                           // the tile of output J -> slot J & 1
        constexpr int J = decltype(jc)::value;
        unsigned jstep;
        const long long jb = group_out_base(kind, ph, J, d, PR, jstep);
        // plane row jb (block-uniform) goes into the descriptor, the lane's row and piece into a 32-bit offset
        const __amdgpu_buffer_rsrc_t rc = make_rsrc_uniform(cond + jb * (2 * C) + col0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned pk = drow[k];
            const unsigned voff = jstep < pk >> 20 ? (pk & 0xfffffu) * (2 * C * 4) + dcol : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, (lds_ptr_t)(stage + (J & 1) * TILE + k * 256), 16, voff, 0, 0, 0);
        }
    };
    request(std::integral_constant<int, 0>{});
    request(std::integral_constant<int, 1>{});
    static_for<4>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        unsigned jstep;
        const long long jb = group_out_base(kind, ph, j, d, PR, jstep);
        float* const mine = stage + (j & 1) * TILE + lh * (4 * 64) + li;    // element (row 4 lh, column li) of the slot
        // all but the younger requests and stores: tile j has landed
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(j == 0 ? 8 : j == 1 ? 12 : j == 2 ? 16 : 8) : "memory");
        // (output 0, with all six accumulator sets still live, in two rounds: register budget)
        constexpr int RB = j == 0 ? 8 : 16;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += RB) {
            float ctv[RB], csv[RB];
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
                const int r = r0 + rr, row = (r & 3) + 8 * (r >> 2);        // (+ 4 lh: bit 1 of the row is bit 1 of r)
                ctv[rr] = mine[wino_stage_at(row, 0)];
                csv[rr] = mine[wino_stage_at(row, 32)];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
                const int r = r0 + rr;
                const float ct = ctv[rr], cs = csv[rr];
                float tv, sv;
                if constexpr (j == 0) {
                    tv = acc[0][0][r] + acc[1][0][r] + acc[2][0][r] + acc[3][0][r] + acc[4][0][r] + ct;
                    sv = acc[0][1][r] + acc[1][1][r] + acc[2][1][r] + acc[3][1][r] + acc[4][1][r] + cs;
                } else if constexpr (j == 1) {
                    tv = acc[1][0][r] - acc[2][0][r] + 2.f * (acc[3][0][r] - acc[4][0][r]) + ct;
                    sv = acc[1][1][r] - acc[2][1][r] + 2.f * (acc[3][1][r] - acc[4][1][r]) + cs;
                } else if constexpr (j == 2) {
                    tv = acc[1][0][r] + acc[2][0][r] + 4.f * (acc[3][0][r] + acc[4][0][r]) + ct;
                    sv = acc[1][1][r] + acc[2][1][r] + 4.f * (acc[3][1][r] + acc[4][1][r]) + cs;
                } else {
                    tv = acc[1][0][r] - acc[2][0][r] + 8.f * (acc[3][0][r] - acc[4][0][r]) + acc[5][0][r] + ct;
                    sv = acc[1][1][r] - acc[2][1][r] + 8.f * (acc[3][1][r] - acc[4][1][r]) + acc[5][1][r] + cs;
                }
                mine[wino_stage_at((r & 3) + 8 * (r >> 2), 0)] = gate_tanh_sigmoid(tv, sv);     // in place of its tanh element
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // wave-private slot: no barrier needed
        f32x4 v[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
            v[qq] = *reinterpret_cast<const f32x4*>(stage + (j & 1) * TILE + (er + 8 * qq) * 64 + (((er >> 1) & 1) << 5) + ec4);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // the slot is consumed: the next tile may land in it
        if constexpr (j + 2 < 4) request(std::integral_constant<int, j + 2>{});
        // (32-bit offset: row * 2 KB stays below the descriptor's 2^31 bytes because waveglow.hip refuses a call whose
        //  phase-major rows x C x 4 bytes reach 2^31)
        const __amdgpu_buffer_rsrc_t ra = make_rsrc_uniform(acts + jb * C + (col0 >> 6) * 32);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const unsigned pk = srow[qq];
            const unsigned voff = jstep < pk >> 20 ? (pk & 0xfffffu) * (C * 4) + (unsigned)ec4 * 4u : OOB;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v[qq]), ra, voff, 0, 0);
        }
    });
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fused form of the GEMM + combine passes.  One block owns BM group rows x BN pre-activation columns of ALL SIX products: its
// K loop walks product after product (K = 512) through one LDS-DMA pipeline, each product
// into its own accumulator set (a wave holds 32 rows x 64 columns x 6 products = 192 accumulator registers), and the epilogue
// applies the output transform, adds the conditioning plane (bias included) and the gate in registers and stores the four output row sets of `acts` -- no P planes
// (1.26 GB written and read per layer at config 2), no combine launch.  Same products in the same k order as the three-pass
// form, so the two agree to the last bit of the fp32 sums (the output transform is written identically).
struct WinoFusedArgs {
    const float* U;   long long uplane;                       // transformed inputs [6][Mq][512]
    const float* G;   long long gplane;                       // tap combinations [6][1024][512]
    const float* cond;                 // conditioning plane [32 PR][1024], bias included (wino_cond_kernel)
    float* acts;                       // [32 PR][512]
    int Mq, phase_rows;                // group rows; group rows per (group) phase block
    int kind;                          // 0 phase groups (d <= 8), 1 frame groups (d >= 32), 2 mixed groups (d = 16)
    int d, PR, BT, T;
};

template <int WR, int WC, int NBUF, int OCC>
__global__ __launch_bounds__(WR * WC * 64, OCC) void wino4_fused_kernel(const WinoFusedArgs g) {
    constexpr int NW = WR * WC, BM = WR * 32, BN = WC * 64;
    constexpr int NPA = BM / 16, NPB = BN / 16, PPW = (NPA + NPB) / NW;     // 16-row DMA pieces: A side, B side, per wave
    static_assert((NPA + NPB) % NW == 0, "the pieces of a tile divide among the waves");
    constexpr int STAGE = (BM + BN) * 16;                                   // floats per LDS buffer: [A rows | B rows] x 16 k
    static_assert(NBUF * STAGE >= NW * 32 * 36, "the epilogue's transpose patches fit the pipeline buffers");
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int li = lane & 31, lh = lane >> 5;

    // XCD-aware order (as gemm_f32_kernel): the numNt column blocks of an M tile run back to back on one XCD
    constexpr int numNt = 2 * C / BN;
    const int numMt = g.Mq / BM;
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int mt = (slot / numNt) * 8 + xcd, nt = slot % numNt;
    if (mt >= numMt) return;
    const int m0 = mt * BM, n0 = nt * BN;
    const int ph = m0 / g.phase_rows, fr0 = m0 - ph * g.phase_rows;        // block-uniform (group) phase, first row inside it

    f32x16 acc[6][2];
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][h][r] = 0.f;

    // ---- tile stream.  Piece q of a tile = 16 rows x 64 B: q < NPA operand rows, else weight rows; lane l of a piece fetches
    // chunk (l & 3) ^ ((l >> 4) & 3) of row l >> 2 and lands at byte 16 l of the piece (XOR swizzle through the source address)
    const int prow = lane >> 2, chunk = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned vo0[PPW];                                                      // per-lane byte offsets
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int q = wave * PPW + i;
        const int row = (q < NPA ? q : q - NPA) * 16 + prow;
        vo0[i] = (unsigned)((row * C + chunk * 4) * 4);
    }
    int lp = 0, lkc = 0;                                                    // (product, chunk) of the next tile to request
    // The tile stream in two parts, as in gemm_f32_kernel's rotated loop: `prepare` does the (scalar) address math of the next
    // tile, `issue_piece` requests one 16-row piece of it.
    unsigned vo[PPW], ko = 0;                                               // per-lane offsets / scalar K offset of the prepared tile
    const float* pb[PPW];                                                   // (wave-uniform) descriptor bases of its pieces
    auto prepare = [&]() {
        const bool live = lp < 6;                                           // past the last tile the pieces fetch nothing
        const int p = live ? lp : 0;
        ko = (unsigned)lkc * 64u;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const bool isA = wave * PPW + i < NPA;                          // wave-uniform
            pb[i] = isA ? g.U + p * g.uplane + (long long)m0 * C : g.G + p * g.gplane + (long long)n0 * C;
            vo[i] = live ? vo0[i] : OOB;
        }
        if (live && ++lkc == C / 16) {
            lkc = 0;
            ++lp;
        }
    };
    auto issue_piece = [&](int i, int buf) {
        // (by-value copies: with an element of a local array as the builtin's operand hipcc's HOST pass silently emits no stub
        //  for the kernel -- undefined symbol when the library is loaded)
        const unsigned voff = vo[i], koff = ko;
        const float* base = pb[i];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(make_rsrc_uniform(base), (lds_ptr_t)(smem + buf * STAGE + (wave * PPW + i) * 256), 16,
                                                 voff, koff, 0, 0);
    };
    const int xr = (li >> 2) & 3;
    struct Frag {
        f32x4 a, b0, b1;
    };
    auto read_frag = [&](int buf, int k8, Frag& f) {                        // the K = 8 half k8 of a tile: one A and two B fragments
        const int koff = ((2 * k8 + lh) ^ xr) * 4;
        const float* a = smem + buf * STAGE + (wr * 32 + li) * 16 + koff;
        const float* b = smem + buf * STAGE + BM * 16 + (wc * 64 + li) * 16 + koff;
        f.a = *reinterpret_cast<const f32x4*>(a);
        f.b0 = *reinterpret_cast<const f32x4*>(b);
        f.b1 = *reinterpret_cast<const f32x4*>(b + 32 * 16);
    };

    // K loop, rotated by half a step (gemm_f32_kernel: the plain loop left the matrix pipe idle after every barrier while all
    // waves issued their DMA pieces and waited for their operand reads: 71 % of peak).  Step t = [reads of tile t's second half |
    // MFMAs of its first half | wait for tile t + 1, barrier | reads of tile t + 1's first half | MFMAs of the second half with
    // the pieces of tile t + NBUF requested one per MFMA pair into tile t's buffer -- every wave holds tile t in registers].
#pragma unroll
    for (int b = 0; b < NBUF; ++b) {
        prepare();
#pragma unroll
        for (int i = 0; i < PPW; ++i) issue_piece(i, b);
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NBUF - 1)) : "memory");
    __builtin_amdgcn_s_barrier();
    Frag f0, f1;
    read_frag(0, 0, f0);
    int buf = 0;
    static_for<6>([&](auto pc) {
        constexpr int P = decltype(pc)::value;
        for (int s = 0; s < C / 16; ++s) {
            read_frag(buf, 1, f1);
            prepare();                                                      // tile t + NBUF (address math only)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                acc[P][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f0.a[kk], f0.b0[kk], acc[P][0], 0, 0, 0);
                acc[P][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f0.a[kk], f0.b1[kk], acc[P][1], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);                              // (keeps the MFMAs above the wait)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PPW * (NBUF - 2)) : "memory");
            __builtin_amdgcn_s_barrier();
            const int bufn = buf == NBUF - 1 ? 0 : buf + 1;
            read_frag(bufn, 0, f0);                                         // (past the last tile: zeros nothing uses)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                acc[P][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f1.a[kk], f1.b0[kk], acc[P][0], 0, 0, 0);
                acc[P][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f1.a[kk], f1.b1[kk], acc[P][1], 0, 0, 0);
                if (kk < PPW) {
                    issue_piece(kk, buf);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            static_assert(PPW <= 4, "one DMA piece per MFMA pair of the second half");
            buf = bufn;
        }
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the fetch-nothing pieces of the last steps
    __builtin_amdgcn_s_barrier();

    // ---- epilogue
    wino_gate_store(acc, smem + wave * (32 * 36), g.cond, g.acts, g.kind, g.d, ph, fr0 + wr * 32, n0 + wc * 64, g.PR, g.BT, g.T, lane);
}

template <int WR, int WC, int NBUF, int OCC>
hipError_t launch_wino_fused(const WinoFusedArgs& a, hipStream_t st) {
    constexpr int BM = WR * 32, BN = WC * 64;
    const size_t lds = (size_t)NBUF * (BM + BN) * 16 * sizeof(float);
    if (a.Mq % BM != 0 || a.phase_rows % BM != 0 || a.Mq % a.phase_rows != 0) return hipErrorInvalidValue;
    auto kern = wino4_fused_kernel<WR, WC, NBUF, OCC>;
    static PerDeviceOnce attr_set;
    if (hipError_t e = set_max_dyn_lds_once((const void*)kern, lds, attr_set); e != hipSuccess) return e;
    const int numMt8 = (a.Mq / BM + 7) / 8 * 8;
    hipLaunchKernelGGL(kern, dim3(numMt8 * (2 * C / BN)), dim3(WR * WC * 64), lds, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fused form WITHOUT the pre-pass: the input transform moves into the operand reads.  The K loop of the tap part runs chunk
// by chunk (16 columns of the 512), and for every chunk the SIX INPUT tiles x[l + (i - 1) d] of the block's 64 group rows are
// fetched once (the same bytes as six transformed tiles) by LDS-DMA with per-lane row addresses -- the gather the pre-pass
// did: phase carries, frame groups, rows outside an utterance read as zero through out-of-range offsets -- and stay in LDS for
// the six products of that chunk; a product's A fragment is then 3 - 4 ds_read_b128 of input fragments combined in registers
// (U0 = 4 x0 - 5 x2 + x4, ...: the arithmetic of wino4_prepass_kernel) under the MFMAs of the other half step.  No U planes
// (0.63 GB of workspace and 1.26 GB of traffic per layer at config 2), no pre-pass launch.  4 waves, 64 x 128 tile per
// product, two blocks per CU; LDS: two stages of six input tiles (48 KB) + three weight tiles (24 KB).
struct WinoFused2Args {
    const float* x;                                           // residual stream [32 PR][512]
    const float* G;   long long gplane;                       // tap combinations [6][1024][512]
    const float* cond;                                        // conditioning plane [32 PR][1024], bias included
    float* acts;
    int Mq, phase_rows, kind, d, PR, BT, T;
};

// Phase measurement for scripts/wino_stamps.py: only in a build made with -DTTS_WINO_STAMPS (csrc/build.sh never passes it).
// Every block leaves its clock at entry, at the end of its K loop and at its end, and where it ran; the last launch stays.
#ifdef TTS_WINO_STAMPS
__device__ unsigned long long g_wino_stamps[4 * 8192];
#define WINO_STAMP(i)                                                                               \
    do {                                                                                            \
        if (tid == 0 && bid < 8192) g_wino_stamps[4 * bid + (i)] = __builtin_amdgcn_s_memtime();    \
    } while (0)
#else
#define WINO_STAMP(i) do { } while (0)
#endif

__global__ __launch_bounds__(256, 2) void wino4_fused2_kernel(const WinoFused2Args g) {
    constexpr int BM = 64, BN = 128, NBUF = 3, NG = C / 16;                 // NG = 32 chunks of the tap part
    constexpr int XT = BM * 16, XS = 6 * XT, BS = BN * 16;                  // floats: one input tile, one stage of six, one weight tile
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const xs = smem;                                                 // [2][6][64][16]
    float* const Bs = smem + 2 * XS;                                        // [3][128][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    constexpr int numNt = 2 * C / BN;
    const int numMt = g.Mq / BM;
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int mt = (slot / numNt) * 8 + xcd, nt = slot % numNt;
    if (mt >= numMt) return;
    const int m0 = mt * BM, n0 = nt * BN;
    const int ph = m0 / g.phase_rows, fr0 = m0 - ph * g.phase_rows;
#ifdef TTS_WINO_STAMPS
    if (tid == 0 && bid < 8192)                                             // HW_ID | XCC_ID << 32
        g_wino_stamps[4 * bid + 3] = (unsigned long long)__builtin_amdgcn_s_getreg(31 << 11 | 4) |
                                     (unsigned long long)__builtin_amdgcn_s_getreg(31 << 11 | 20) << 32;
#endif
    WINO_STAMP(0);

    f32x16 acc[6][2];
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][h][r] = 0.f;

    // ---- per-lane source offsets.  A DMA piece = 16 rows x 64 B; lane l fetches chunk (l & 3) ^ ((l >> 4) & 3) of row l >> 2.
    const int prow = lane >> 2, chunk = (lane & 3) ^ ((lane >> 4) & 3);
    const int sfr = g.d / NPH;
    // input i of this lane's group row = (block-uniform row delta of input i) + (this lane's base row), or nothing: one base
    // offset and a validity mask per lane, the deltas go into the descriptor base
    unsigned xbase = 0, xvalid = 0;
    int xdelta[6];                                                          // (floats; < 2^31: checked at launch)
    {
        const int gl = fr0 + wave * 16 + prow;                              // group row inside the (group) phase block
        int b = 0, t0 = 0;
        bool ok;
        if (g.kind == 0) {                                                  // four phases of one frame: base = the frame row
            ok = gl < g.BT;
            t0 = gl % g.T;
            xbase = (unsigned)gl;
        } else if (g.kind == 1) {                                           // four frames of one phase: base = frame t0 of the utterance
            ok = frame_group(gl, sfr, g.BT, g.T, b, t0);
            xbase = (unsigned)(b * g.T + t0);
        } else {                                                            // two phases x two frames
            ok = mixed_group(gl, g.BT, g.T, b, t0);
            xbase = (unsigned)(b * g.T + t0);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            int dt;                                                         // frame offset of input i from the base row
            if (g.kind == 0) {
                const int ps = group_phase0(ph, g.d) + (i - 1) * g.d;
                dt = ps >> 5;
                xdelta[i] = ((ps & 31) * g.PR + dt) * C;
            } else if (g.kind == 1) {
                dt = (i - 1) * sfr;
                xdelta[i] = (ph * g.PR + dt) * C;
            } else {
                const int ps = ph + 16 * (i - 1);
                dt = ps >> 5;
                xdelta[i] = ((ps & 31) * g.PR + dt) * C;
            }
            if (ok && t0 + dt >= 0 && t0 + dt < g.T) xvalid |= 1u << i;
        }
        xbase = xbase * (unsigned)(C * 4) + (unsigned)chunk * 16u;
    }
    // this wave's two weight pieces are 16 rows apart: one per-lane offset, the second piece's distance is a scalar
    const unsigned vb0 = (unsigned)(((2 * wave * 16 + prow) * C + chunk * 4) * 4);

    // ---- DMA requests
    const float* const gb0 = g.G + (long long)n0 * C;
    auto issue_x = [&](auto ic, int grp) {                                  // input tile I of chunk group `grp` -> stage grp & 1
        constexpr int I = decltype(ic)::value;
        const unsigned voff = (grp < NG && ((xvalid >> I) & 1u)) ? xbase : OOB;      // (past the last group: fetch nothing, keep the counts)
        const float* base = g.x + (long long)xdelta[I];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(make_rsrc_uniform(base), (lds_ptr_t)(xs + (grp & 1) * XS + I * XT + wave * 256), 16, voff,
                                                 (unsigned)grp * 64u, 0, 0);
    };
    auto issue_b_taps = [&](int j, int prod, int grp, int buf) {            // weight piece j of (product, chunk group) -> Bs[buf]
        const float* base = gb0 + prod * (2 * C * C);                       // (the planes of G are 1024 x 512 floats apart)
        const unsigned voff = grp < NG ? vb0 : OOB;                         // (past the last group: fetch nothing, keep the counts)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(make_rsrc_uniform(base), (lds_ptr_t)(Bs + buf * BS + (2 * wave + j) * 256), 16, voff,
                                                 (unsigned)grp * 64u + (unsigned)j * (16u * C * 4u), 0, 0);
    };
    // ---- operand fragments
    const int xr = (li >> 2) & 3;
    struct Frag {
        f32x4 a, b0, b1;
    };
    struct Raw {
        f32x4 v[4];
    };
    auto read_b = [&](int buf, int h, Frag& f) {
        const float* b = Bs + buf * BS + (wc * 64 + li) * 16 + ((2 * h + lh) ^ xr) * 4;
        f.b0 = *reinterpret_cast<const f32x4*>(b);
        f.b1 = *reinterpret_cast<const f32x4*>(b + 32 * 16);
    };
    // product P's input fragments of half h: P = 0: x0 x2 x4, P = 1 .. 4: x1 x2 x3 x4, P = 5: x1 x3 x5
    auto read_x = [&](auto pc, int stage, int h, Raw& r) {
        constexpr int P = decltype(pc)::value;
        const float* a = xs + stage * XS + (wr * 32 + li) * 16 + ((2 * h + lh) ^ xr) * 4;
        constexpr int i0 = P == 0 ? 0 : 1, i1 = P == 0 ? 2 : P == 5 ? 3 : 2, i2 = P == 0 ? 4 : P == 5 ? 5 : 3;
        r.v[0] = *reinterpret_cast<const f32x4*>(a + i0 * XT);
        r.v[1] = *reinterpret_cast<const f32x4*>(a + i1 * XT);
        r.v[2] = *reinterpret_cast<const f32x4*>(a + i2 * XT);
        if constexpr (P >= 1 && P <= 4) r.v[3] = *reinterpret_cast<const f32x4*>(a + 4 * XT);
    };
    auto combine = [&](auto pc, const Raw& r) -> f32x4 {                    // the input transform (wino4_prepass_kernel)
        constexpr int P = decltype(pc)::value;
        if constexpr (P == 0) return 4.f * r.v[0] - 5.f * r.v[1] + r.v[2];
        else if constexpr (P == 1) return -4.f * (r.v[0] + r.v[1]) + r.v[2] + r.v[3];
        else if constexpr (P == 2) return 4.f * (r.v[0] - r.v[1]) - r.v[2] + r.v[3];
        else if constexpr (P == 3) return 2.f * (r.v[2] - r.v[0]) - r.v[1] + r.v[3];
        else if constexpr (P == 4) return 2.f * (r.v[0] - r.v[2]) - r.v[1] + r.v[3];
        else return 4.f * r.v[0] - 5.f * r.v[1] + r.v[2];
    };
    auto mfma2 = [&](auto pc, const Frag& f, int kk) {
        constexpr int P = decltype(pc)::value;
        acc[P][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[kk], f.b0[kk], acc[P][0], 0, 0, 0);
        acc[P][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[kk], f.b1[kk], acc[P][1], 0, 0, 0);
    };

    // ---- prologue: the six input tiles of group 0 and weight tiles 0 - 2.  Steady state: every step requests ONE input tile
    // of the next group (in the order the products need them: x0 x2 x4 | x1 x3 | x5) and the weight tile three steps ahead -- three
    // pieces per wave and step, so "all but the last three requests" = everything up to two steps ago = the next tile's operands.
    // (the prologue ends like a steady-state step: [one input tile, weight tile 2], so that step 0's "all but three" covers tile 1)
    static_for<5>([&](auto ic) { issue_x(ic, 0); });
    issue_b_taps(0, 0, 0, 0); issue_b_taps(1, 0, 0, 0);
    issue_b_taps(0, 1, 0, 1); issue_b_taps(1, 1, 0, 1);
    issue_x(std::integral_constant<int, 5>{}, 0);
    issue_b_taps(0, 2, 0, 2); issue_b_taps(1, 2, 0, 2);
    asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    Frag f0, f1;
    Raw raw;
    read_x(std::integral_constant<int, 0>{}, 0, 0, raw);
    read_b(0, 0, f0);
    f0.a = combine(std::integral_constant<int, 0>{}, raw);

    // ---- K loop: 32 chunk groups x 6 products, rotated by half a step.  Step (grp, P) = [input fragments of the second half |
    // MFMAs of the first | wait, barrier | fragments of the next tile's first half | MFMAs of the second half with this step's
    // three requests].  The look-ahead of the last group's steps reaches past the last tile: those requests fetch nothing
    // (they keep the counts), and the last step's fragments of a "next tile" are stale LDS contents that nothing uses.
    int buf = 0;                                                            // weight-ring slot of the current tile
    for (int grp = 0; grp < NG; ++grp) {
        const int stage = grp & 1;
        static_for<6>([&](auto pc) {
            constexpr int P = decltype(pc)::value;
            constexpr int PN = (P + 1) % 6, P3 = (P + 3) % 6;
            constexpr int XI = P < 3 ? 2 * P : P == 3 ? 1 : P == 4 ? 3 : 5;  // the input tile of the next group requested in this step
            // half-step = [input fragments of the next half | 2 MFMA pairs | combine | weight fragments | 2 MFMA pairs]: the sixteen
            // input registers and the eight weight registers of the incoming half are never live together (register budget)
            read_x(pc, stage, 1, raw);
            mfma2(pc, f0, 0);
            mfma2(pc, f0, 1);
            __builtin_amdgcn_sched_barrier(0);
            f1.a = combine(pc, raw);
            read_b(buf, 1, f1);
            __builtin_amdgcn_sched_barrier(0);
            mfma2(pc, f0, 2);
            mfma2(pc, f0, 3);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int bufn = buf == NBUF - 1 ? 0 : buf + 1;
            read_x(std::integral_constant<int, PN>{}, P == 5 ? stage ^ 1 : stage, 0, raw);
            __builtin_amdgcn_sched_barrier(0);
            mfma2(pc, f1, 0);
            issue_x(std::integral_constant<int, XI>{}, grp + 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma2(pc, f1, 1);
            __builtin_amdgcn_sched_barrier(0);
            f0.a = combine(std::integral_constant<int, PN>{}, raw);
            read_b(bufn, 0, f0);
            __builtin_amdgcn_sched_barrier(0);
            mfma2(pc, f1, 2);
            issue_b_taps(0, P3, grp + (P >= 3 ? 1 : 0), buf);
            __builtin_amdgcn_sched_barrier(0);
            mfma2(pc, f1, 3);
            issue_b_taps(1, P3, grp + (P >= 3 ? 1 : 0), buf);
            __builtin_amdgcn_sched_barrier(0);
            buf = bufn;
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    WINO_STAMP(1);

    // ---- epilogue: every wave owns 16 KB of the released pipeline buffers (64 KB of the block's 72)
    wino_gate_store_dma(acc, smem + wave * (2 * 32 * 64), g.cond, g.acts, g.kind, g.d, ph, fr0 + wr * 32, n0 + wc * 64, g.PR, g.BT, g.T,
                        lane);
    WINO_STAMP(2);
}

hipError_t launch_wino_fused2(const WinoFused2Args& a, hipStream_t st) {
    constexpr int BM = 64, BN = 128;
    const size_t lds = (size_t)(2 * 6 * BM * 16 + 3 * BN * 16) * sizeof(float);
    if (a.Mq % BM != 0 || a.phase_rows % BM != 0 || a.Mq % a.phase_rows != 0) return hipErrorInvalidValue;
    static PerDeviceOnce attr_set;
    if (hipError_t e = set_max_dyn_lds_once((const void*)wino4_fused2_kernel, lds, attr_set); e != hipSuccess) return e;
    const int numMt8 = (a.Mq / BM + 7) / 8 * 8;
    hipLaunchKernelGGL(wino4_fused2_kernel, dim3(numMt8 * (2 * C / BN)), dim3(256), lds, st, a);
    return hipGetLastError();
}

#ifdef TTS_WINO_STAMPS
}  // namespace
// the stamps of the last wino4_fused2_kernel launch: n records of {entry, K loop end, end, HW_ID | XCC_ID << 32}
extern "C" __attribute__((visibility("default"))) int tts_hip_debug_wino_stamps(unsigned long long* out, int n) {
    if (n < 0 || n > 8192 || hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wino_stamps), (size_t)n * 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
namespace {
#endif

inline unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// group rows per block: frame groups (dilations >= 32) B x 4 ceil(T / 16) per phase, mixed groups (dilation 16) B x ceil(T / 2)
// per p0, both padded to the 128-row tile
// (padded to the row tile of the kernel that runs them: 64 rows for the fused kernels, 128 for the three-pass form's GEMM --
//  config 2's frame groups: 1 600 rows per phase instead of 1 664, i.e. 4 % less work in three of the seven layers)
static inline int group_row_tile(int form) { return form == 2 ? 128 : 64; }
static inline int frame_group_rows(int BT, int T, int form) {
    const int g = group_row_tile(form);
    return ((BT / T) * frame_groups_per_utt(T) + g - 1) / g * g;
}
static inline int mixed_group_rows(int BT, int T, int form) {
    const int g = group_row_tile(form);
    return ((BT / T) * mixed_groups_per_utt(T) + g - 1) / g * g;
}

static inline int cond_group_rows(int BT, int T) { return ((BT / T) * cond_groups_per_utt(T) + 63) / 64 * 64; }

// Per-layer operands (on the first call that takes this path): for layers 1 .. 7 of every flow the tap combinations G
// ([6][1024][512], 12.6 MB), for all eight layers the conditioning weight planes W ([32][7][1024][80], 73 MB), for the first
// layer its tap weights ([1024][16]) -- 8.1 GB in all, the same for every form.  A failed allocation frees what this call built.
int waveglow_build_wino(tts_hip_engine* e) {
    WaveGlowDev& wg = e->wg;
    if (wg.wino_ready) return TTS_HIP_OK;
    hipStream_t st = e->stream;
    std::vector<void*> fresh;                              // this call's allocations (moved to wg.allocs on success)
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(st);
        for (void* p : fresh) (void)hipFree(p);
        for (int k = 0; k < 12; ++k)
            for (int i = 0; i < 8; ++i) wg.flow[k].layer[i].wino_G = wg.flow[k].layer[i].wino_W = wg.flow[k].layer[i].wino_T = nullptr;
        return rc;
    };
    for (int k = 0; k < 12; ++k)
        for (int i = 0; i < 8; ++i) {
            WgLayerDev& ly = wg.flow[k].layer[i];
            const long long nw = (long long)NPH * NPT * 2 * C * NMEL;
            int rc;
            if (i == 0) {                                  // (in_Bt of the first layer: the composed taps [1024][3 x 16])
                if ((rc = dev_alloc(e, (size_t)2 * C * 16, &ly.wino_T, fresh, false))) return fail(rc);
                hipLaunchKernelGGL(wino_tap_weights_kernel, dim3(blocks_for(2 * C * 16)), dim3(256), 0, st, ly.in_Bt, ly.wino_T,
                                   wg.flow[k].n_half);
            } else {
                if ((rc = dev_alloc(e, (size_t)6 * 2 * C * C, &ly.wino_G, fresh, false))) return fail(rc);
                hipLaunchKernelGGL(wino4_weights_kernel, dim3(blocks_for(2 * C * C)), dim3(256), 0, st, ly.in_Bt, ly.wino_G);
            }
            if ((rc = dev_alloc(e, (size_t)nw, &ly.wino_W, fresh, false))) return fail(rc);
            hipLaunchKernelGGL(wino_cond_weights_kernel, dim3(blocks_for(nw)), dim3(256), 0, st, ly.cond_Bt, ly.wino_W);
            if (hipError_t herr = hipGetLastError(); herr != hipSuccess)
                return fail(set_err(e, TTS_HIP_EHIP, "waveglow_build_wino: %s", hipGetErrorString(herr)));
        }
    if (hipError_t herr = hipStreamSynchronize(st); herr != hipSuccess)
        return fail(set_err(e, TTS_HIP_EHIP, "waveglow_build_wino: %s", hipGetErrorString(herr)));
    wg.allocs.insert(wg.allocs.end(), fresh.begin(), fresh.end());
    wg.wino_ready = true;
    return TTS_HIP_OK;
}

// Workspace of one call, and its mel planes (the mel does not change across layers and flows)
int waveglow_wino_begin(tts_hip_engine* e, const float* d_mel, int PR, int BT, int T, int form) {
    const bool three_pass = form == 2, need_U = form != 1;                 // form 1 transforms its inputs on the fly: no U planes
    WaveGlowDev& wg = e->wg;
    hipStream_t st = e->stream;
    const int PRq = frame_group_rows(BT, T, form), PRm = mixed_group_rows(BT, T, form), PRc = cond_group_rows(BT, T);
    // U (and the three-pass form's P): six planes of 8 PR (phase groups), 32 PRq (frame groups) or 16 PRm (mixed groups) rows
    const size_t rows = 6 * (size_t)std::max(std::max((long long)(NPH / 4) * PR, (long long)NPH * PRq), (long long)16 * PRm);
    auto room = [&](DevBuf& b, size_t bytes) -> int {       // out of memory is its own status: the caller keeps the direct form
        const hipError_t err = b.ensure(bytes);
        if (err == hipSuccess) return TTS_HIP_OK;
        if (err == hipErrorOutOfMemory) (void)hipGetLastError();
        return set_err(e, err == hipErrorOutOfMemory ? TTS_HIP_ENOMEM : TTS_HIP_EHIP, "waveglow_wino_begin: hipMalloc(%zu bytes) -> %s",
                       bytes, hipGetErrorString(err));
    };
    int rc;
    if (need_U && (rc = room(wg.wino_U, rows * C * 4))) return rc;
    if (three_pass && (rc = room(wg.wino_P, rows * 2 * C * 4))) return rc;
    if ((rc = room(wg.wino_mel, ((size_t)NPT * PRc * NMEL + PRc) * 4))) return rc;      // [mel planes | row table]
    if ((rc = room(wg.wino_taps, (size_t)NPH * PR * 16 * 4))) return rc;                // tap operand of a flow's first layer
    // the conditioning plane [32 PR][1024]; its padding rows (frame rows >= BT of a phase) are never written and feed only the
    // padding rows of `acts`: cleared once per allocation so that they hold numbers
    const size_t before = wg.wino_cond.bytes;
    if ((rc = room(wg.wino_cond, (size_t)NPH * PR * 2 * C * 4))) return rc;
    if (wg.wino_cond.bytes != before) HIPCHK(e, hipMemsetAsync(wg.wino_cond.p, 0, wg.wino_cond.bytes, st));
    hipLaunchKernelGGL(wino_cond_mel_planes_kernel, dim3(blocks_for((long long)NPT * PRc * NMEL)), dim3(256), 0, st, d_mel,
                       wg.wino_mel.f(), PRc, BT, T);
    hipLaunchKernelGGL(wino_cond_rows_kernel, dim3(blocks_for(PRc)), dim3(256), 0, st, (int*)(wg.wino_mel.f() + (size_t)NPT * PRc * NMEL),
                       PRc, BT, T);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

static WinoCondArgs cond_args(WaveGlowDev& wg, const WgLayerDev& ly, int PR, int BT, int T) {
    WinoCondArgs c{};
    c.Z = wg.wino_mel.f();
    c.W = ly.wino_W;
    c.bias = ly.in_bias;
    c.cond = wg.wino_cond.f();
    c.rows = cond_group_rows(BT, T);
    c.rowtab = (const int*)(c.Z + (size_t)NPT * c.rows * NMEL);
    c.PR = PR;
    c.BT = BT;
    c.T = T;
    return c;
}

// The first layer of a flow with h coupling channels: acts_0 = gate(taps(a0p) + cond + b) from the a0p rows the start kernel
// wrote (tail rows cleared): the tap operand, then the layer's kernel.  The same launches in every form and tile family.
int waveglow_wino_layer0(tts_hip_engine* e, const WgLayerDev& ly, int h, const float* a0p, float* acts_0, int PR, int BT, int T) {
    WaveGlowDev& wg = e->wg;
    hipStream_t st = e->stream;
    WinoCondArgs c = cond_args(wg, ly, PR, BT, T);
    c.taps = wg.wino_taps.f();
    c.Wt = ly.wino_T;
    c.acts = acts_0;
    timing_begin(e, 3);
    hipLaunchKernelGGL(wino_tap_operand_kernel, dim3(blocks_for((long long)NPH * PR * 16)), dim3(256), 0, st, a0p, wg.wino_taps.f(), h,
                       PR, BT, T);
    HIPCHK(e, (launch_wino_cond<2, 2, 3, 3, true>(c, st)));
    timing_end(e);
    return TTS_HIP_OK;
}

// One WN in-layer step (layer i >= 1 of a flow): acts_i = gate(conv_d(x) + cond + b): the conditioning plane, then the in-layer
// kernel of the form (inside one timing bracket: "one WN in-layer step")
int waveglow_wino_layer(tts_hip_engine* e, const WgLayerDev& ly, int i, const float* x, float* acts_i, int PR, int BT, int T) {
    WaveGlowDev& wg = e->wg;
    hipStream_t st = e->stream;
    const int d = 1 << i;
    float* U = wg.wino_U.f();
    float* P = wg.wino_P.f();
    const int PRq = frame_group_rows(BT, T, wg.form_mode), PRm = mixed_group_rows(BT, T, wg.form_mode);
    const bool phases = d <= 8, mixed = d == 16;
    const long long Mq = phases ? (long long)(NPH / 4) * PR : mixed ? (long long)16 * PRm : (long long)NPH * PRq;
    const WinoCondArgs c = cond_args(wg, ly, PR, BT, T);
    const bool no_prepass = wg.form_mode == 1;             // form 1 (default): input transform inside the GEMM's operand reads
    if (!no_prepass) hipLaunchKernelGGL(wino4_prepass_kernel, dim3(blocks_for(Mq * (C / 4))), dim3(256), 0, st, x, U, d, PR, BT, T, Mq);
    if (wg.form_mode != 2) {                               // fused GEMM + output transform + gate (form 2: the three passes)
        WinoFusedArgs a{};
        a.U = U;
        a.uplane = Mq * C;
        a.G = ly.wino_G;
        a.gplane = (long long)2 * C * C;
        a.cond = c.cond;
        a.acts = acts_i;
        a.Mq = (int)Mq;
        a.phase_rows = phases ? PR : mixed ? PRm : PRq;
        a.kind = phases ? 0 : mixed ? 2 : 1;
        a.d = d;
        a.PR = PR;
        a.BT = BT;
        a.T = T;
        if (no_prepass) {
            WinoFused2Args b{};
            b.x = x;
            b.G = a.G; b.gplane = a.gplane;
            b.cond = a.cond; b.acts = a.acts;
            b.Mq = a.Mq; b.phase_rows = a.phase_rows; b.kind = a.kind; b.d = a.d; b.PR = a.PR; b.BT = a.BT; b.T = a.T;
            timing_begin(e, 0);
            HIPCHK(e, (launch_wino_cond<2, 2, 3, 3>(c, st)));
            HIPCHK(e, launch_wino_fused2(b, st));
            timing_end(e);
            return TTS_HIP_OK;
        }
        timing_begin(e, 0);
        HIPCHK(e, (launch_wino_cond<2, 2, 3, 3>(c, st)));
        // form 3 (measurement): the fused kernel behind the pre-pass (64 x 128 tiles, two blocks per CU; measured at config 2
        // on one box: three passes 433 ms per step, this 415, without the pre-pass 409; 8-wave 128 x 128 blocks: 425)
        HIPCHK(e, (launch_wino_fused<2, 2, 3, 2>(a, st)));
        timing_end(e);
        return TTS_HIP_OK;
    }
    // form 2 (measurement): one z slice of the GEMM per product, K = 512, then the combine pass
    GemmArgs g{};
    g.M = (int)Mq;
    g.N = 2 * C;
    g.nphase = phases ? NPH / 4 : mixed ? 16 : NPH;
    g.phase_rows = phases ? PR : mixed ? PRm : PRq;
    g.frames = phases ? BT : mixed ? (BT / T) * mixed_groups_per_utt(T) : (BT / T) * frame_groups_per_utt(T);
    g.L = g.phase_rows;
    g.ldb = C;
    g.mode = EPI_LINEAR;
    g.act = ACT_NONE;
    g.split = 2 * C;
    g.ld0 = 2 * C;
    g.wide_epi = 1;
    g.nseg = 1;
    g.seg[0] = ASeg{U, C, 0, C, C, SEG_ROWS_Z, 0, Mq, 0};
    g.Bt = ly.wino_G;
    g.strideBz = (long long)2 * C * C;
    g.out0 = P;
    g.strideOutZ = Mq * 2 * C;
    timing_begin(e, 0);
    HIPCHK(e, (launch_wino_cond<2, 2, 3, 3>(c, st)));
    HIPCHK(e, phases && PR % 256 == 0 ? gemm_wn_wino(g, 6, st) : gemm_wn_wino_128(g, 6, st));
    timing_end(e);
    hipLaunchKernelGGL(wino4_combine_kernel, dim3(blocks_for(Mq * (C / 4))), dim3(256), 0, st, P, c.cond, acts_i, d, PR, BT, T, Mq);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}
