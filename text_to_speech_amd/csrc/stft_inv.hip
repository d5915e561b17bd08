// stft_inv.hip -- the STFT with its phase, its inverse, and Griffin-Lim phase reconstruction on gfx950.
//
// Completes the reference's utils/audio/stft.py STFT class (:194-274): `transform` returns magnitude and phase (or real and
// imaginary parts), and the windowed pseudo-inverse basis the class builds (:220-236) gets the use it was made for -- complex
// spectrogram -> audio by a frames GEMM and an overlap-add normalised by the summed squared window.  On the two sits
// Griffin-Lim (with the "fast" momentum term): per iteration one inverse-frames GEMM, one gather overlap-add straight into
// the reflect-padded rows the forward DFT GEMM reads, that GEMM, and one phasor update -- no atan2 / sin / cos in the loop.
// All rows of a batch run in one launch per part, driven by frames[b]; nothing is accumulated with atomics, so a row never
// depends on its neighbours and a repeat gives the same bits.  The WaveGlow denoiser (tts_hip_denoise) is one pass of the
// same parts -- the plan's forward DFT, a gate that lowers every bin's magnitude by strength x the model's bias spectrum and
// keeps its phase, the inverse-frames GEMM, the gather overlap-add cut to each row's length -- chained without the host.
// Time stretching (tts_hip_time_stretch) puts a phase-locked vocoder (identity phase locking, Laroche and Dolson 1999)
// between the same transform and inverse: a parallel pass over every output frame (magnitudes, peaks, each bin's nearest
// peak, the phase factors) and one workgroup per row that walks the frames and carries the synthesis phase in LDS.
// Formant matching (tts_hip_formant_match) puts the ratio of two cepstrally smoothed envelopes there: the log-magnitudes of a
// source's and the audio's spectra, one GEMM against a liftering table, and one workgroup per frame that turns the ratio into
// an energy-keeping gain on the audio's spectrum.
// include/tts_hip.h has the contract, audio_call.h the checks and the geometry (GlGeom, DnGeom, TsGeom, FmGeom), mel_stft.hip the plans and
// the forward DFT.
//
// The inverse basis has a closed form, so no SVD runs here: pinv(scale * [cos; -sin])^T has the rows
// c_k cos(2 pi k n / N) / (N scale) and -c_k sin(2 pi k n / N) / (N scale), c_0 = 1, c_{N/2} = 1 (N even), else c_k = 2
// (tests/test_stft_inv.py compares it with scipy's pinv).
#include "engine.h"
#include "audio_dev.h"
#include "gemm_f32.h"

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

using namespace ttsgemm;

namespace {

// (re, im) / |(re, im)|, (1, 0) at the origin.  Scaled by the larger component first: the squares of a tiny pair neither
// underflow nor overflow.  -> |(re, im)| from the scaled pair (the denoiser's gate; Griffin-Lim drops it)
__device__ __forceinline__ float phasor(float re, float im, float& pr, float& pi) {
    const float m = fmaxf(fabsf(re), fabsf(im));
    if (!(m > 0.f)) {
        pr = 1.f, pi = 0.f;
        return 0.f;
    }
    const float a = re / m, b = im / m;
    const float n = sqrtf(a * a + b * b);
    pr = a / n, pi = b / n;
    return m * n;
}

// transform: out0 / out1 [B][Fout][cut] from the spectrum [B * Fr][NB]; what 0 magnitude and phase, 1 real and imaginary
// parts; frames at and beyond fo[b] (null: Fout) are 0
__global__ void stft_polar_kernel(const float* __restrict__ ft, float* __restrict__ out0, float* __restrict__ out1, long long n, int Fr,
                                  int Fout, int cut, int NB, const int* __restrict__ fo, int what) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long cell = idx / cut, b = cell / Fout;
    const int f = (int)(cell % Fout), c = (int)(idx % cut);
    float v0 = 0.f, v1 = 0.f;
    if (f < (fo ? fo[b] : Fout)) {
        const long long r = b * Fr + f;
        const float re = ft[r * NB + c], im = ft[r * NB + cut + c];
        if (what == 0) {
            v0 = sqrtf(re * re + im * im);
            v1 = atan2f(im, re);
        } else {
            v0 = re, v1 = im;
        }
    }
    out0[idx] = v0;
    out1[idx] = v1;
}

// inverse: the GEMM's A operand [B * F][NB] from two planes [B][F][cut]; form 0 magnitude and phase, 1 real and imaginary
// parts.  Nothing behind a row's own frames is read; those frames and the K padding are 0.
__global__ void inv_operand_kernel(const float* __restrict__ p0, const float* __restrict__ p1, float* __restrict__ A, long long n, int F,
                                   int cut, int NB, const int* __restrict__ frames, int form) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long r = idx / NB;
    const int col = (int)(idx % NB), c = col < cut ? col : col - cut;
    float v = 0.f;
    if (col < 2 * cut && (int)(r % F) < frames[r / F]) {
        const float a = p0[r * cut + c], b = p1[r * cut + c];
        if (form == 0) v = col < cut ? a * cosf(b) : a * sinf(b);
        else v = col < cut ? a : b;
    }
    A[idx] = v;
}

// One sample of the overlap-add at untrimmed index i of row b (Fb frames): the frames that cover it summed in frame order,
// divided by the summed squared window where that is above FLT_MIN, times scale
__device__ __forceinline__ float ola_sample(const float* __restrict__ T, const float* __restrict__ win2, long long row0, int Fb, int i,
                                            int hop, int fl, float scale) {
    int f0 = i - fl + 1;
    f0 = f0 <= 0 ? 0 : (f0 + hop - 1) / hop;
    const int f1 = min(Fb - 1, i / hop);
    float acc = 0.f, ws = 0.f;
    for (int f = f0; f <= f1; ++f) {
        const int k = i - f * hop;
        acc += T[(row0 + f) * fl + k];
        ws += win2[k];
    }
    if (ws > FLT_MIN) acc /= ws;
    return acc * scale;
}

// The overlap-add as a gather, in one of two layouts.  padded != 0: y [B][NP] (+ 64 floats behind the last row) takes the
// row's S_b = hop (Fb - 1) + fl - 2 half samples reflect-padded by half on each side -- what the forward DFT reads -- and 0
// everywhere else.  padded == 0: y [B][pitch] takes the S_b samples and 0 beyond.
__global__ void ola_kernel(const float* __restrict__ T, const float* __restrict__ win2, float* __restrict__ y, long long n, int B, int F,
                           int pitch, const int* __restrict__ frames, int hop, int fl, int half, float scale, int padded) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long b = idx / pitch;
    const int p = (int)(idx % pitch);
    float v = 0.f;
    if (b < B) {
        const int Fb = frames[b], S = hop * (Fb - 1) + fl - 2 * half;
        int s = -1;
        if (padded) {
            if (p < S + 2 * half) {
                s = p - half;
                if (s < 0) s = -s;
                if (s >= S) s = 2 * (S - 1) - s;
            }
        } else if (p < S) {
            s = p;
        }
        if (s >= 0) v = ola_sample(T, win2, b * F, Fb, s + half, hop, fl, scale);
    }
    y[idx] = v;
}

// denoiser: the overlap-add in the caller's own layout y [B][N]: row b takes its first min(lens[b], S_b) samples, 0 beyond
__global__ void ola_cut_kernel(const float* __restrict__ T, const float* __restrict__ win2, float* __restrict__ y, long long n, int F, int N,
                               const int* __restrict__ frames, const int* __restrict__ lens, int hop, int fl, int half, float scale) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long b = idx / N;
    const int i = (int)(idx % N), Fb = frames[b];
    const int keep = min(lens[b], hop * (Fb - 1) + fl - 2 * half);
    y[idx] = i < keep ? ola_sample(T, win2, b * F, Fb, i + half, hop, fl, scale) : 0.f;
}

// denoiser: the inverse GEMM's operand A [B * F][NB] from the spectrum ft [B * Fr][NB]: a bin (re, im) of magnitude m keeps
// its phase and gets the magnitude max(m - s * bias[c], 0); the origin gives 0, as do the frames behind a row's own and the K
// padding.  n = B * F * (NB - cut) threads: j < cut owns the pair of bin j, j >= cut clears padding column cut + j.
__global__ void denoise_gate_kernel(const float* __restrict__ ft, const float* __restrict__ bias, float* __restrict__ A, long long n,
                                    int Fr, int F, int cut, int NB, const int* __restrict__ frames, float s) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int W = NB - cut, j = (int)(idx % W);
    const long long r = idx / W, b = r / F;
    const int f = (int)(r % F);
    float* row = A + r * NB;
    if (j >= cut) {
        row[cut + j] = 0.f;
        return;
    }
    float yr = 0.f, yi = 0.f;
    if (f < frames[b]) {
        const float* src = ft + (b * Fr + f) * NB;
        float pr, pi;
        const float m = phasor(src[j], src[cut + j], pr, pi);
        const float gated = fmaxf(m - s * bias[j], 0.f);
        yr = gated * pr, yi = gated * pi;
    }
    row[j] = yr;
    row[cut + j] = yi;
}

// ---- time stretch: the phase-locked vocoder between the transform and the inverse (include/tts_hip.h has the math)
// |(re, im)| as the header states it: two products, one sum, one square root, none of them fused
__device__ __forceinline__ float ts_abs(float re, float im) { return sqrtf(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im))); }

// k is a peak of the frame's magnitudes sm[0 .. cut): positive, above both left neighbours, not below both right ones
__device__ __forceinline__ bool ts_peak(const float* sm, int k, int cut) {
    const float v = sm[k];
    if (!(v > 0.f)) return false;
    if (k >= 1 && !(v > sm[k - 1])) return false;
    if (k >= 2 && !(v > sm[k - 2])) return false;
    if (k + 1 < cut && !(v >= sm[k + 1])) return false;
    if (k + 2 < cut && !(v >= sm[k + 2])) return false;
    return true;
}

// analysis frame i = floor(t * r) and the fraction a = (float)(t * r - i) of output frame t, in double as on the host
__device__ __forceinline__ int ts_position(int t, double r, float& a) {
    const double pos = (double)t * r, fl = floor(pos);
    a = (float)(pos - fl);
    return (int)fl;
}

constexpr int TS_THREADS = 256;         // ts_analyse_kernel: one workgroup per output frame

// The parallel pass, one workgroup per (row b, output frame t < T): everything of the vocoder that does not depend on the
// synthesis phase of frame t - 1.  m[t][k] goes to mag and to LDS; every thread marks the peaks of its run of
// ceil(cut / 256) consecutive bins; a max-scan from the left over the runs' last peaks and a min-scan from the right over
// their first peaks give each run the peak before and behind it, and a sweep inside the run the nearest one of every bin
// (a tie goes down).  Then per bin R[t][k] = P(c0[k] conj(c0[own])) and A[t-1][own] = P(X[i'+1][own] conj(X[i'][own])),
// i' = floor((t - 1) r), taken straight from the spectrum (own = k in a frame without peaks).  Analysis frames at and beyond
// fo[b] are 0 and never read; output frames at and beyond frames[b] get m = 0 and own = -1 and nothing else.
// Dynamic LDS: cut floats (m) + cut ints (the peak before a bin, then its owner).
__global__ __launch_bounds__(TS_THREADS) void ts_analyse_kernel(const float* __restrict__ ft, const int* __restrict__ fo,
                                                                const int* __restrict__ frames, const double* __restrict__ rates,
                                                                float* __restrict__ mag, int* __restrict__ owner,
                                                                float2* __restrict__ adv, float2* __restrict__ rel, int Fr, int T,
                                                                int cut, int NB) {
    extern __shared__ float ts_lds[];
    float* sm = ts_lds;
    int* sl = (int*)(ts_lds + cut);
    __shared__ int sh[16], edge[TS_THREADS];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const long long cell0 = ((long long)b * T + t) * cut;
    if (t >= frames[b]) {
        for (int k = tid; k < cut; k += TS_THREADS) mag[cell0 + k] = 0.f, owner[cell0 + k] = -1;
        return;
    }
    const int Fb = fo[b];
    const double r = rates[b];
    float a;
    const int i = ts_position(t, r, a);                         // i <= Fb - 1: (T_b - 1) r < F_b
    const float* x0 = ft + ((long long)b * Fr + i) * NB;
    const float* x1 = x0 + NB;
    const bool live1 = i + 1 < Fb;
    const float na = __fsub_rn(1.f, a);
    for (int k = tid; k < cut; k += TS_THREADS) {
        const float m0 = ts_abs(x0[k], x0[cut + k]), m1 = live1 ? ts_abs(x1[k], x1[cut + k]) : 0.f;
        const float m = __fadd_rn(__fmul_rn(na, m0), __fmul_rn(a, m1));
        sm[k] = m;
        mag[cell0 + k] = m;
    }
    __syncthreads();
    const int C = (cut + TS_THREADS - 1) / TS_THREADS, k0 = min(cut, tid * C), k1 = min(cut, k0 + C);
    int last = -1, first = INT_MAX;
    for (int k = k0; k < k1; ++k)
        if (ts_peak(sm, k, cut)) {
            last = k;
            if (first == INT_MAX) first = k;
        }
    int any, none;
    const int upto = block_scan(last, sh, any, OpMax());        // the last peak in the runs 0 .. tid
    edge[tid] = upto;
    __syncthreads();
    int before = tid ? edge[tid - 1] : -1;
    __syncthreads();
    edge[tid] = first;
    __syncthreads();
    const int mirrored = edge[TS_THREADS - 1 - tid];
    const int from = block_scan(mirrored, sh, none, OpMin());   // the first peak in the runs 255 - tid .. 255
    edge[TS_THREADS - 1 - tid] = from;
    __syncthreads();
    int behind = tid + 1 < TS_THREADS ? edge[tid + 1] : INT_MAX;
    for (int k = k0; k < k1; ++k) {
        if (ts_peak(sm, k, cut)) before = k;
        sl[k] = before;
    }
    for (int k = k1 - 1; k >= k0; --k) {
        if (ts_peak(sm, k, cut)) behind = k;
        const int lo = sl[k];
        int own = -1;
        if (any >= 0) own = lo < 0 ? behind : behind == INT_MAX ? lo : (k - lo <= behind - k ? lo : behind);
        sl[k] = own;
    }
    __syncthreads();
    float ap = 0.f;
    const int ip = t ? ts_position(t - 1, r, ap) : 0;
    const float* y0 = ft + ((long long)b * Fr + ip) * NB;
    const float* y1 = y0 + NB;
    const bool livep = ip + 1 < Fb;
    for (int k = tid; k < cut; k += TS_THREADS) {
        const int own = sl[k], p = own < 0 ? k : own;
        owner[cell0 + k] = own;
        float2 R = make_float2(1.f, 0.f), A = make_float2(1.f, 0.f);
        if (own >= 0) {
            const float cr = x0[k], ci = x0[cut + k], pr = x0[p], pi = x0[cut + p];
            phasor(cr * pr + ci * pi, ci * pr - cr * pi, R.x, R.y);
        }
        if (t && livep) {
            const float cr = y1[p], ci = y1[cut + p], pr = y0[p], pi = y0[cut + p];
            phasor(cr * pr + ci * pi, ci * pr - cr * pi, A.x, A.y);
        }
        rel[cell0 + k] = R;
        adv[cell0 + k] = A;
    }
}

constexpr int TS_CHAIN_BINS = 3;        // bins per thread of ts_chain_kernel: 3 x 1024 threads >= 2049 bins

struct TsCell {
    int own;
    float m;
    float2 adv, rel;
};

__device__ __forceinline__ TsCell ts_cell(const float* __restrict__ mag, const int* __restrict__ owner, const float2* __restrict__ adv,
                                          const float2* __restrict__ rel, long long at) {
    return TsCell{owner[at], mag[at], adv[at], rel[at]};
}

// The sequential pass, one workgroup per row walking its output frames: U[0] = P(X[0]); U[t][k] = P(U[t-1][p] A[t-1][p]
// R[t][k]), p = own[t][k] -- U[t-1] is gathered from LDS, the other two factors come from the parallel pass -- or
// U[t-1][k] A[t-1][k] in a frame without peaks; the operand of the inverse takes m[t][k] U[t][k].  U is double-buffered in
// LDS (2 x cut pairs): frame t reads the buffer frame t - 1 wrote and writes the other one, so one barrier per frame
// orders both.  Thread j owns the bins j, j + blockDim.x, ... (at most TS_CHAIN_BINS); the cells of frame t + 1 are loaded
// before the products of frame t, so no global load waits between two barriers.  Rows of A behind frames[b] and its K
// padding are left as the caller cleared them.
__global__ __launch_bounds__(1024) void ts_chain_kernel(const float* __restrict__ ft, const int* __restrict__ frames,
                                                        const float* __restrict__ mag, const int* __restrict__ owner,
                                                        const float2* __restrict__ adv, const float2* __restrict__ rel,
                                                        float* __restrict__ A, int Fr, int T, int cut, int NB) {
    extern __shared__ float2 ts_u[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, Tb = frames[b];
    const long long row0 = (long long)b * T;
    const float* x0 = ft + (long long)b * Fr * NB;
    TsCell next[TS_CHAIN_BINS];
#pragma unroll
    for (int j = 0; j < TS_CHAIN_BINS; ++j) {
        const int k = tid + j * nt;
        if (k >= cut) continue;
        float2 u;
        phasor(x0[k], x0[cut + k], u.x, u.y);
        ts_u[k] = u;
        const float m = mag[row0 * cut + k];
        A[row0 * NB + k] = m * u.x;
        A[row0 * NB + cut + k] = m * u.y;
        if (Tb > 1) next[j] = ts_cell(mag, owner, adv, rel, (row0 + 1) * cut + k);
    }
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        const float2* prev = ts_u + ((t - 1) & 1) * cut;
        float2* cur = ts_u + (t & 1) * cut;
        TsCell c[TS_CHAIN_BINS];
#pragma unroll
        for (int j = 0; j < TS_CHAIN_BINS; ++j) {
            const int k = tid + j * nt;
            if (k >= cut) continue;
            c[j] = next[j];
            if (t + 1 < Tb) next[j] = ts_cell(mag, owner, adv, rel, (row0 + t + 1) * cut + k);
        }
#pragma unroll
        for (int j = 0; j < TS_CHAIN_BINS; ++j) {
            const int k = tid + j * nt;
            if (k >= cut) continue;
            const float2 u = prev[c[j].own < 0 ? k : c[j].own], g = c[j].adv;
            float2 v = make_float2(u.x * g.x - u.y * g.y, u.x * g.y + u.y * g.x);
            if (c[j].own >= 0) {
                const float2 q = c[j].rel;
                phasor(v.x * q.x - v.y * q.y, v.x * q.y + v.y * q.x, v.x, v.y);
            }
            cur[k] = v;
            A[(row0 + t) * NB + k] = c[j].m * v.x;
            A[(row0 + t) * NB + cut + k] = c[j].m * v.y;
        }
        __syncthreads();
    }
}

// probe only: own as floats
__global__ void ts_owner_float_kernel(const int* __restrict__ owner, float* __restrict__ out, long long n) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = (float)owner[idx];
}

// ---- formant match: the cepstral envelopes of source and audio and their ratio as a gain on the audio's spectrum
// (include/tts_hip.h has the math)
// The envelope GEMM's A operand, rows [B * F][CK] of logf(max(|X|, 1e-5f)) from the spectrum ft [B * F][NB]: 0 in the frames
// behind a row's own and in the K padding.  `twin` (source NULL: X = Y) takes the same values.
__global__ void fm_logmag_kernel(const float* __restrict__ ft, float* __restrict__ A, float* __restrict__ twin, long long n, int F,
                                 int cut, int NB, int CK, const int* __restrict__ frames) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long r = idx / CK;
    const int c = (int)(idx % CK);
    float v = 0.f;
    if (c < cut && (int)(r % F) < frames[r / F]) {
        const float* src = ft + r * NB;
        v = logf(fmaxf(ts_abs(src[c], src[cut + c]), 1e-5f));
    }
    A[idx] = v;
    if (twin) twin[idx] = v;
}

constexpr int FM_THREADS = 256;         // fm_gain_kernel: one workgroup per frame

// Steps 4 - 7, one workgroup per (frame f, row b): the source's envelope Sx = env[b * F + f] read at k / beta (linear
// interpolation, the top bin held; no fused multiply-add, so beta = 1 gives Sx itself), the log gain E = that - Sy (Sy =
// env[rows + b * F + f]) clamped to +-G, g = expf(E), the frame's energies e0 = sum |Y|^2 and e1 = sum (g |Y|)^2 in a fixed
// order (each thread its bins k = tid, tid + 256, ... in turn, then block_reduce), and the operand row gain * Y with gain =
// g * sqrtf(e0 / e1) (e1 == 0: g).  Frames at and beyond frames[b] and the K padding are written 0.  gain_out (probe only)
// [B * F][cut].  Dynamic LDS: cut floats (g).
__global__ __launch_bounds__(FM_THREADS) void fm_gain_kernel(const float* __restrict__ ft, const float* __restrict__ env,
                                                             const int* __restrict__ frames, const double* __restrict__ warps,
                                                             float* __restrict__ A, float* __restrict__ gain_out, long long rows,
                                                             int F, int cut, int NB, float G) {
    extern __shared__ float fm_g[];
    __shared__ float sh[16];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long long r = (long long)b * F + f;
    float* row = A + r * NB;
    if (f >= frames[b]) {
        for (int k = tid; k < NB; k += FM_THREADS) row[k] = 0.f;
        if (gain_out)
            for (int k = tid; k < cut; k += FM_THREADS) gain_out[r * cut + k] = 0.f;
        return;
    }
    const float* Sx = env + r * cut;
    const float* Sy = env + (rows + r) * cut;
    const float* y = ft + r * NB;
    const double beta = warps[b];
    float e0 = 0.f, e1 = 0.f;
    for (int k = tid; k < cut; k += FM_THREADS) {
        const double pos = (double)k / beta, fl = floor(pos);
        const int i = (int)fl;                                  // <= 2 (cut - 1)
        float sx;
        if (i >= cut - 1) {
            sx = Sx[cut - 1];
        } else {
            const float a = (float)(pos - fl);
            sx = __fadd_rn(__fmul_rn(__fsub_rn(1.f, a), Sx[i]), __fmul_rn(a, Sx[i + 1]));
        }
        const float E = __fsub_rn(sx, Sy[k]);
        const float g = expf(fminf(fmaxf(E, -G), G));
        const float m = ts_abs(y[k], y[cut + k]), gm = __fmul_rn(g, m);
        e0 = __fadd_rn(e0, __fmul_rn(m, m));
        e1 = __fadd_rn(e1, __fmul_rn(gm, gm));
        fm_g[k] = g;
    }
    e0 = block_reduce(e0, sh, OpAdd{});
    e1 = block_reduce(e1, sh, OpAdd{});
    const float s = e1 == 0.f ? 1.f : sqrtf(e0 / e1);
    for (int k = tid; k < cut; k += FM_THREADS) {               // a thread reads back the g of its own bins only
        const float gain = __fmul_rn(fm_g[k], s);
        row[k] = gain * y[k];
        row[cut + k] = gain * y[cut + k];
        if (gain_out) gain_out[r * cut + k] = gain;
    }
    for (int k = 2 * cut + tid; k < NB; k += FM_THREADS) row[k] = 0.f;
}

// log-mel input: E [B * F][EK] = exp(spec [B * F][nmel]) on a row's own frames, 0 beyond and in the K padding
__global__ void gl_exp_kernel(const float* __restrict__ spec, float* __restrict__ E, long long n, int F, int nmel, int EK,
                              const int* __restrict__ frames) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long r = idx / EK;
    const int j = (int)(idx % EK);
    E[idx] = j < nmel && (int)(r % F) < frames[r / F] ? expf(spec[r * nmel + j]) : 0.f;
}

// target [B * F][cut] = src (clamp: max(0, src)) on a row's own frames, else 0; the first operand S p_0 with p_0 = P(init)
// (init [B * F][cut][2]; null: (1, 0))
__global__ void gl_init_kernel(const float* src, float* target, const float* __restrict__ init, float* __restrict__ A, long long n, int F,
                               int cut, int NB, const int* __restrict__ frames, int clamp) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long r = idx / cut;
    const int c = (int)(idx % cut);
    float S = 0.f, pr = 1.f, pi = 0.f;
    if ((int)(r % F) < frames[r / F]) {
        S = src[idx];
        if (clamp) S = fmaxf(S, 0.f);
        if (init) phasor(init[2 * idx], init[2 * idx + 1], pr, pi);
    }
    target[idx] = S;
    A[r * NB + c] = S * pr;
    A[r * NB + cut + c] = S * pi;
}

// The phase update: c = Y - alpha t_prev, t_prev = Y, p = P(c), next operand S p (0 behind a row's frames); `ph` (probe
// only) takes p
__global__ void gl_phase_kernel(const float* __restrict__ ft, float* __restrict__ tprev, const float* __restrict__ target,
                                float* __restrict__ A, float* __restrict__ ph, long long n, int F, int cut, int NB,
                                const int* __restrict__ frames, float alpha) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long r = idx / cut;
    const int c = (int)(idx % cut);
    const long long ir = r * NB + c, ii = ir + cut;
    const float yr = ft[ir], yi = ft[ii];
    const float cr = yr - alpha * tprev[ir], ci = yi - alpha * tprev[ii];
    tprev[ir] = yr;
    tprev[ii] = yi;
    float pr, pi;
    phasor(cr, ci, pr, pi);
    const bool own = (int)(r % F) < frames[r / F];
    const float S = own ? target[idx] : 0.f;
    A[ir] = S * pr;
    A[ii] = S * pi;
    if (ph) ph[ir] = pr, ph[ii] = pi;
}

// the windowed inverse basis and the squared window of a plan, on first use
int inv_tables(tts_hip_engine* e, tts_hip_mel_fn* fn) {
    if (fn->inv_Bt) return TTS_HIP_OK;
    const MelPlan& p = fn->p;
    const int N = p.fl;
    const double scale = (double)p.fl / p.hop;
    std::vector<float> bt((size_t)N * p.NB, 0.f), w2(N);
    for (int n = 0; n < N; ++n) {
        for (int k = 0; k < p.cut; ++k) {
            const double ck = (k == 0 || 2 * k == N) ? 1.0 : 2.0;
            const double ang = 2.0 * M_PI * (double)(((long long)k * n) % N) / N;          // exact phase reduction
            bt[(size_t)n * p.NB + k] = (float)((double)(float)(ck * std::cos(ang) / (N * scale)) * fn->win[n]);
            bt[(size_t)n * p.NB + p.cut + k] = (float)((double)(float)(-ck * std::sin(ang) / (N * scale)) * fn->win[n]);
        }
        w2[n] = (float)(fn->win[n] * fn->win[n]);
    }
    if (int rc = upload(e, w2.data(), w2.size(), &fn->win2, fn->allocs)) return rc;
    return upload(e, bt.data(), bt.size(), &fn->inv_Bt, fn->allocs);
}

// the plan's own mel inversion, on first use
int minv_table(tts_hip_engine* e, const char* name, tts_hip_mel_fn* fn) {
    if (fn->minv_state == 0) {
        std::vector<double> Minv;
        if (!mel_min_norm_inverse(fn->p, Minv)) {
            fn->minv_state = -1;
        } else {
            const int EK = up_to(fn->p.nmel, 32), cut = fn->p.cut;
            std::vector<float> bt((size_t)cut * EK, 0.f);
            for (int j = 0; j < fn->p.nmel; ++j)
                for (int c = 0; c < cut; ++c) bt[(size_t)c * EK + j] = (float)Minv[(size_t)j * cut + c];
            if (int rc = upload(e, bt.data(), bt.size(), &fn->minv_Bt, fn->allocs)) return rc;
            fn->minv_state = 1;
        }
    }
    if (fn->minv_state < 0)
        return set_err(e, TTS_HIP_EINVAL, "%s: the plan's filterbank has no minimum-norm inverse (a mel channel without a bin)", name);
    return TTS_HIP_OK;
}

struct GlBufs {
    int* info;
    float *target, *operand, *tprev, *phasor, *tframes, *padded, *gathered, *spectrum, *expmel, *minv;
};

int gl_bufs(tts_hip_engine* e, const GlGeom& g, GlBufs* w) {
    HIPCHK(e, e->stft.inv_ws.ensure(g.total));
    char* base = (char*)e->stft.inv_ws.p;
    *w = GlBufs{(int*)(base + g.off_info),        (float*)(base + g.off_target),   (float*)(base + g.off_operand),
                (float*)(base + g.off_tprev),     (float*)(base + g.off_phasor),   (float*)(base + g.off_tframes),
                (float*)(base + g.off_padded),    (float*)(base + g.off_gathered), (float*)(base + g.off_spectrum),
                (float*)(base + g.off_expmel),    (float*)(base + g.off_minv)};
    e->audio_info_h.assign(g.frames.begin(), g.frames.end());
    return stage_row_info(e, w->info);
}

// tframes [B * F][filter_length] = operand x inverse basis
int inverse_frames(tts_hip_engine* e, const tts_hip_mel_fn& fn, const GlGeom& g, const GlBufs& w) {
    const MelPlan& p = fn.p;
    HIPCHK(e, gemm_small(gemm_linear(w.operand, p.NB, p.NB, fn.inv_Bt, p.NB, p.fl, g.B * g.F, w.tframes), 1, e->stream));
    return TTS_HIP_OK;
}

int overlap_add(tts_hip_engine* e, const tts_hip_mel_fn& fn, const GlGeom& g, const GlBufs& w, float* y, bool padded) {
    const MelPlan& p = fn.p;
    const int pitch = padded ? g.NP : (int)g.Sout;
    const long long n = (long long)g.B * pitch + (padded ? 64 : 0);
    hipLaunchKernelGGL(ola_kernel, dim3(blocks(n, 256)), dim3(256), 0, e->stream, w.tframes, fn.win2, y, n, g.B, g.F, pitch, w.info, p.hop,
                       p.fl, p.half, (float)((double)p.fl / p.hop), padded ? 1 : 0);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

// device pointers only, the call already checked (g).  stop_k / stop_what >= 0 (the probe): return right after that stage of
// that iteration with *view describing it.  With tts_hip_kernel_timing on, the four parts of an iteration are timed as kinds
// 0 (inverse-frames GEMM), 1 (overlap-add), 2 (forward DFT, its gather included) and 3 (phase update)
int gl_exec(tts_hip_engine* e, tts_hip_mel_fn& fn, const GlGeom& g, const float* d_spec, int kind, const double* Minv,
            const float* d_init, int n_iters, double momentum, float* d_audio, int stop_k, int stop_what, StageView* view) {
    const MelPlan& p = fn.p;
    hipStream_t st = e->stream;
    GlBufs w;
    if (int rc = gl_bufs(e, g, &w)) return rc;
    const long long rows = (long long)g.B * g.F, cells = rows * p.cut;
    auto stop_at = [&](int it, int stage, const float* ptr, size_t nrows, size_t width, size_t pitch) {
        const bool hit = stop_what == stage && (stage == GL_TARGET || stop_k == it);
        if (hit && view) *view = StageView{ptr, nrows, width, pitch};
        return hit;
    };
    HIPCHK(e, hipMemsetAsync(w.tprev, 0, (size_t)rows * p.NB * 4, st));
    HIPCHK(e, hipMemsetAsync(w.operand, 0, (size_t)rows * p.NB * 4, st));
    const float* src = d_spec;
    if (kind == 1) {
        const float* minv_Bt = fn.minv_Bt;
        if (Minv) {                                     // the caller's [n_mel][cut] in double -> [cut][EK] fp32
            e->stft.minv_h.assign((size_t)p.cut * g.EK, 0.f);
            for (int j = 0; j < p.nmel; ++j)
                for (int c = 0; c < p.cut; ++c) e->stft.minv_h[(size_t)c * g.EK + j] = (float)Minv[(size_t)j * p.cut + c];
            HIPCHK(e, hipMemcpyAsync(w.minv, e->stft.minv_h.data(), e->stft.minv_h.size() * 4, hipMemcpyHostToDevice, st));
            minv_Bt = w.minv;
        }
        const long long n = rows * g.EK;
        hipLaunchKernelGGL(gl_exp_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d_spec, w.expmel, n, g.F, p.nmel, g.EK, w.info);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, gemm_small(gemm_linear(w.expmel, g.EK, g.EK, minv_Bt, g.EK, p.cut, (int)rows, w.target), 1, st));
        src = w.target;
    }
    hipLaunchKernelGGL(gl_init_kernel, dim3(blocks(cells, 256)), dim3(256), 0, st, src, w.target, d_init, w.operand, cells, g.F, p.cut,
                       p.NB, w.info, kind == 1 ? 1 : 0);
    HIPCHK(e, hipGetLastError());
    if (stop_at(0, GL_TARGET, w.target, (size_t)rows, p.cut, p.cut)) return TTS_HIP_OK;
    const float alpha = (float)(momentum / (1.0 + momentum));
    for (int it = 0;; ++it) {
        if (stop_at(it, GL_OPERAND, w.operand, (size_t)rows, 2 * p.cut, p.NB)) return TTS_HIP_OK;
        timing_begin(e, 0);
        if (int rc = inverse_frames(e, fn, g, w)) return rc;
        timing_end(e);
        if (stop_at(it, GL_FRAMES, w.tframes, (size_t)rows, p.fl, p.fl)) return TTS_HIP_OK;
        if (it == n_iters && stop_what != GL_SIGNAL) return overlap_add(e, fn, g, w, d_audio, false);
        timing_begin(e, 1);
        if (int rc = overlap_add(e, fn, g, w, w.padded, true)) return rc;
        timing_end(e);
        if (stop_at(it, GL_SIGNAL, w.padded, g.B, g.PW, g.NP)) return TTS_HIP_OK;
        timing_begin(e, 2);
        if (int rc = mel_dft_gemm(e, fn, w.padded, w.gathered, w.spectrum, g.B, g.F, g.NP)) return rc;
        timing_end(e);
        if (stop_at(it, GL_SPECTRUM, w.spectrum, (size_t)rows, 2 * p.cut, p.NB)) return TTS_HIP_OK;
        float* ph = stop_what == GL_PHASOR && stop_k == it ? w.phasor : nullptr;
        timing_begin(e, 3);
        hipLaunchKernelGGL(gl_phase_kernel, dim3(blocks(cells, 256)), dim3(256), 0, st, w.spectrum, w.tprev, w.target, w.operand, ph, cells,
                           g.F, p.cut, p.NB, w.info, alpha);
        HIPCHK(e, hipGetLastError());
        timing_end(e);
        if (stop_at(it, GL_PHASOR, w.phasor, (size_t)rows, 2 * p.cut, p.NB)) return TTS_HIP_OK;
    }
}

// tts_hip_griffin_lim (what = -1), its probe (what = a stage of iteration k) and the _async form (stream, device pointers)
int gl_call(tts_hip_engine* e, const char* name, const float* spec, int B, int F, int C, const int32_t* frames, const tts_hip_mel_fn* fn,
            int input_kind, const double* Minv, const float* init, int n_iters, double momentum, int k, int what, float* out, int mem,
            bool async, void* stream) {
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    GlGeom g;
    char why[256];
    if (input_kind < 0) return set_err(e, TTS_HIP_EINVAL, "%s: input_kind %d not 0 (magnitude) or 1 (log-mel)", name, input_kind);
    if (int rc = stft_inv_check(name, fn ? &fn->p : nullptr, spec, spec, out, B, F, C, frames, input_kind, n_iters, momentum, mem, what, k,
                                &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    tts_hip_mel_fn* plan = const_cast<tts_hip_mel_fn*>(fn);
    HIPCHK(e, hipSetDevice(e->device));
    if (input_kind == 1 && !Minv)
        if (int rc = minv_table(e, name, plan)) return rc;
    if (int rc = inv_tables(e, plan)) return rc;
    const size_t rows = (size_t)B * F;
    if (async) {
        StreamScope scope(e, stream);
        return gl_exec(e, *plan, g, spec, input_kind, Minv, init, n_iters, momentum, out, -1, -1, nullptr);
    }
    AudioStage io(e, mem);
    const int in = io.in(spec, rows * C * 4);
    const int in2 = io.in(init, rows * fn->p.cut * 8);
    const size_t n_audio = (size_t)B * g.Sout * 4;
    const int res = what >= 0 ? io.scratch(n_audio) : io.out(out, n_audio);
    if (int rc = io.begin()) return rc;
    StageView view{};
    if (int rc = gl_exec(e, *plan, g, io.ptr<const float>(in), input_kind, Minv, io.ptr<const float>(in2), n_iters, momentum,
                         io.ptr<float>(res), k, what, &view))
        return rc;
    if (what >= 0)
        if (int rc = copy_stage_out(e, view, out, mem)) return rc;
    const int rc = io.finish();
    timing_collect(e);
    return rc;
}

// device pointers only, the call already checked (g).  stop >= 0 (the probe): return right after that stage with *view
// describing it.  With tts_hip_kernel_timing on, the four parts are timed under Griffin-Lim's kinds: 2 (forward DFT: pad,
// gather where the plan has one, GEMM), 3 (gate), 0 (inverse-frames GEMM) and 1 (overlap-add)
int dn_exec(tts_hip_engine* e, tts_hip_mel_fn& fn, const DnGeom& g, const float* d_audio, int B, int N, const float* d_bias,
            float strength, float* d_out, int stop, StageView* view) {
    const MelPlan& p = fn.p;
    hipStream_t st = e->stream;
    const int F = g.inv.F;
    const long long rows = (long long)B * F;
    StageView spec{};
    timing_begin(e, 2);
    // every row's length goes to the device (lengths NULL: N), so the last kernel can cut to it
    if (int rc = mel_fn_exec(e, fn, g.fwd, d_audio, B, N, true, nullptr, MEL_SPECTRUM, &spec)) return rc;
    timing_end(e);
    if (stop == DN_SPECTRUM) return *view = spec, TTS_HIP_OK;
    const int* d_lens = (const int*)((const char*)e->stft.ws.p + g.fwd.off_info);
    GlBufs w;
    if (int rc = gl_bufs(e, g.inv, &w)) return rc;
    timing_begin(e, 3);
    const long long n = rows * (p.NB - p.cut);
    hipLaunchKernelGGL(denoise_gate_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, (const float*)spec.p, d_bias, w.operand, n, g.fwd.Fr, F,
                       p.cut, p.NB, w.info, strength);
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    if (stop == DN_OPERAND) return *view = StageView{w.operand, (size_t)rows, (size_t)2 * p.cut, (size_t)p.NB}, TTS_HIP_OK;
    timing_begin(e, 0);
    if (int rc = inverse_frames(e, fn, g.inv, w)) return rc;
    timing_end(e);
    if (stop == DN_FRAMES) return *view = StageView{w.tframes, (size_t)rows, (size_t)p.fl, (size_t)p.fl}, TTS_HIP_OK;
    timing_begin(e, 1);
    const long long cells = (long long)B * N;
    hipLaunchKernelGGL(ola_cut_kernel, dim3(blocks(cells, 256)), dim3(256), 0, st, w.tframes, fn.win2, d_out, cells, F, N, w.info, d_lens,
                       p.hop, p.fl, p.half, (float)((double)p.fl / p.hop));
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    return TTS_HIP_OK;
}

// tts_hip_denoise (what = -1), its probe (what = a stage) and the _async form (stream, device pointers)
int dn_call(tts_hip_engine* e, const char* name, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
            const float* bias, double strength, int what, float* out, int mem, bool async, void* stream) {
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    DnGeom g;
    char why[256];
    if (int rc = denoise_check(name, fn ? &fn->p : nullptr, audio, B, N, lengths, bias, strength, out, mem, what, &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    tts_hip_mel_fn* plan = const_cast<tts_hip_mel_fn*>(fn);
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = inv_tables(e, plan)) return rc;
    if (async) {
        StreamScope scope(e, stream);
        return dn_exec(e, *plan, g, audio, B, N, bias, (float)strength, out, -1, nullptr);
    }
    const size_t n_audio = (size_t)B * N * 4;
    AudioStage io(e, mem);
    const int in = io.in(audio, n_audio), ib = io.in(bias, (size_t)fn->p.cut * 4);
    const int res = what >= 0 ? io.scratch(n_audio) : io.out(out, n_audio);
    if (int rc = io.begin()) return rc;
    StageView view{};
    if (int rc = dn_exec(e, *plan, g, io.ptr<const float>(in), B, N, io.ptr<const float>(ib), (float)strength, io.ptr<float>(res), what,
                         &view))
        return rc;
    if (what >= 0)
        if (int rc = copy_stage_out(e, view, out, mem)) return rc;
    const int rc = io.finish();
    timing_collect(e);
    return rc;
}

// device pointers only, the call already checked (g).  stop >= 0 (the probe): return right after that stage with *view
// describing it.  With tts_hip_kernel_timing on, the five parts are timed as kinds 2 (forward DFT: pad, gather where the plan
// has one, GEMM), 3 (parallel pass), 4 (chain), 0 (inverse-frames GEMM) and 1 (overlap-add)
int ts_exec(tts_hip_engine* e, tts_hip_mel_fn& fn, const TsGeom& g, const float* d_audio, int B, int N, float* d_out, int stop,
            StageView* view) {
    const MelPlan& p = fn.p;
    hipStream_t st = e->stream;
    const int T = g.inv.F;
    const long long rows = (long long)B * T, cells = rows * p.cut;
    StageView spec{};
    timing_begin(e, 2);
    if (int rc = mel_fn_exec(e, fn, g.fwd, d_audio, B, N, true, nullptr, MEL_SPECTRUM, &spec)) return rc;
    timing_end(e);
    if (stop == TS_SPECTRUM) return *view = spec, TTS_HIP_OK;
    const int* d_fo = (const int*)((const char*)e->stft.ws.p + g.fwd.off_info) + B;    // mel_fn_exec left [lens | fout] there
    GlBufs w;
    if (int rc = gl_bufs(e, g.inv, &w)) return rc;
    char* base = (char*)e->stft.inv_ws.p;
    const double* d_rates = (const double*)(base + g.off_rowinfo);
    const int* d_S = (const int*)(d_rates + B);
    float* mag = (float*)(base + g.off_mag);
    int* owner = (int*)(base + g.off_owner);
    float2 *adv = (float2*)(base + g.off_adv), *rel = (float2*)(base + g.off_rel);
    e->audio_info_h.resize((size_t)3 * B);                      // [rates as doubles | S]
    memcpy(e->audio_info_h.data(), g.rates.data(), (size_t)B * 8);
    memcpy(e->audio_info_h.data() + 2 * B, g.S.data(), (size_t)B * 4);
    if (int rc = stage_row_info(e, (int*)(base + g.off_rowinfo))) return rc;
    HIPCHK(e, hipMemsetAsync(w.operand, 0, (size_t)rows * p.NB * 4, st));
    timing_begin(e, 3);
    hipLaunchKernelGGL(ts_analyse_kernel, dim3(T, B), dim3(TS_THREADS), (size_t)p.cut * 8, st, (const float*)spec.p, d_fo, w.info, d_rates,
                       mag, owner, adv, rel, g.fwd.Fr, T, p.cut, p.NB);
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    if (stop == TS_MAGNITUDE) return *view = StageView{mag, (size_t)rows, (size_t)p.cut, (size_t)p.cut}, TTS_HIP_OK;
    if (stop == TS_OWNER) {                                     // as floats, in the time frames' buffer (fl >= cut per row)
        hipLaunchKernelGGL(ts_owner_float_kernel, dim3(blocks(cells, 256)), dim3(256), 0, st, owner, w.tframes, cells);
        HIPCHK(e, hipGetLastError());
        return *view = StageView{w.tframes, (size_t)rows, (size_t)p.cut, (size_t)p.cut}, TTS_HIP_OK;
    }
    timing_begin(e, 4);
    const int nt = std::min(1024, up_to(p.cut, 64));
    hipLaunchKernelGGL(ts_chain_kernel, dim3(B), dim3(nt), (size_t)p.cut * 16, st, (const float*)spec.p, w.info, mag, owner, adv, rel,
                       w.operand, g.fwd.Fr, T, p.cut, p.NB);
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    if (stop == TS_OPERAND) return *view = StageView{w.operand, (size_t)rows, (size_t)2 * p.cut, (size_t)p.NB}, TTS_HIP_OK;
    timing_begin(e, 0);
    if (int rc = inverse_frames(e, fn, g.inv, w)) return rc;
    timing_end(e);
    if (stop == TS_FRAMES) return *view = StageView{w.tframes, (size_t)rows, (size_t)p.fl, (size_t)p.fl}, TTS_HIP_OK;
    timing_begin(e, 1);
    const long long n = (long long)B * g.M;
    hipLaunchKernelGGL(ola_cut_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, w.tframes, fn.win2, d_out, n, T, g.M, w.info, d_S, p.hop,
                       p.fl, p.half, (float)((double)p.fl / p.hop));
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    return TTS_HIP_OK;
}

// tts_hip_time_stretch (what = -1), its probe (what = a stage) and the _async form (stream, device pointers)
int ts_call(tts_hip_engine* e, const char* name, const float* audio, int B, int N, const int32_t* lengths, const double* rates,
            const tts_hip_mel_fn* fn, int what, float* out, int M, int mem, bool async, void* stream) {
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    TsGeom g;
    char why[256];
    if (int rc = time_stretch_check(name, fn ? &fn->p : nullptr, audio, B, N, lengths, rates, out, M, mem, what, &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    tts_hip_mel_fn* plan = const_cast<tts_hip_mel_fn*>(fn);
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = inv_tables(e, plan)) return rc;
    if (async) {
        StreamScope scope(e, stream);
        return ts_exec(e, *plan, g, audio, B, N, out, -1, nullptr);
    }
    const size_t n_out = (size_t)B * M * 4;
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4);
    const int res = what >= 0 ? io.scratch(n_out) : io.out(out, n_out);
    if (int rc = io.begin()) return rc;
    StageView view{};
    if (int rc = ts_exec(e, *plan, g, io.ptr<const float>(in), B, N, io.ptr<float>(res), what, &view)) return rc;
    if (what >= 0)
        if (int rc = copy_stage_out(e, view, out, mem)) return rc;
    const int rc = io.finish();
    timing_collect(e);
    return rc;
}

// the liftering table of a plan for the cut Q, on first use; a call with another Q rebuilds it in place
int lift_table(tts_hip_engine* e, tts_hip_mel_fn* fn, int Q) {
    if (fn->lift_Q == Q) return TTS_HIP_OK;
    const MelPlan& p = fn->p;
    std::vector<double> L;
    fm_lifter_table(p.fl, Q, L);
    std::vector<float> bt((size_t)p.cut * p.MAGK, 0.f);         // Bt [N = cut][K = MAGK]: row k holds L[.][k]
    for (int j = 0; j < p.cut; ++j)
        for (int k = 0; k < p.cut; ++k) bt[(size_t)k * p.MAGK + j] = (float)L[(size_t)j * p.cut + k];
    if (!fn->lift_Bt)
        if (int rc = dev_alloc(e, bt.size(), &fn->lift_Bt, fn->allocs, false)) return rc;
    fn->lift_Q = 0;
    HIPCHK(e, hipDeviceSynchronize());                          // an earlier call may still read the table of another Q
    HIPCHK(e, hipMemcpy(fn->lift_Bt, bt.data(), bt.size() * sizeof(float), hipMemcpyHostToDevice));
    fn->lift_Q = Q;
    return TTS_HIP_OK;
}

// device pointers only, the call already checked (g); d_source null: the audio itself.  stop >= 0 (the probe): return right
// after that stage with *view describing it.  With tts_hip_kernel_timing on, the parts are timed as kinds 2 (forward DFT: pad,
// gather where the plan has one, GEMM; twice with a source), 3 (log-magnitudes and the envelope GEMM), 4 (gain), 0
// (inverse-frames GEMM) and 1 (overlap-add)
int fm_exec(tts_hip_engine* e, tts_hip_mel_fn& fn, const FmGeom& g, const float* d_audio, const float* d_source, int B, int N,
            float* d_out, int stop, StageView* view) {
    const MelPlan& p = fn.p;
    hipStream_t st = e->stream;
    const int F = g.inv.F, CK = p.MAGK;
    const long long rows = (long long)B * F, n = rows * CK;
    GlBufs w;
    if (int rc = gl_bufs(e, g.inv, &w)) return rc;
    char* base = (char*)e->stft.inv_ws.p;
    const double* d_warps = (const double*)(base + g.off_warps);
    float *logmag = (float*)(base + g.off_logmag), *env = (float*)(base + g.off_env), *gain = (float*)(base + g.off_gain);
    e->audio_info_h.resize((size_t)2 * B);                      // the warps as doubles
    memcpy(e->audio_info_h.data(), g.warps.data(), (size_t)B * 8);
    if (int rc = stage_row_info(e, (int*)(base + g.off_warps))) return rc;
    StageView spec{};
    if (d_source) {                                             // the mel workspace holds one spectrum at a time
        timing_begin(e, 2);
        if (int rc = mel_fn_exec(e, fn, g.fwd, d_source, B, N, true, nullptr, MEL_SPECTRUM, &spec)) return rc;
        timing_end(e);
        timing_begin(e, 3);
        hipLaunchKernelGGL(fm_logmag_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, (const float*)spec.p, logmag, (float*)nullptr, n, F,
                           p.cut, p.NB, CK, w.info);
        HIPCHK(e, hipGetLastError());
        timing_end(e);
    }
    timing_begin(e, 2);
    if (int rc = mel_fn_exec(e, fn, g.fwd, d_audio, B, N, true, nullptr, MEL_SPECTRUM, &spec)) return rc;
    timing_end(e);
    const float* Y = (const float*)spec.p;                      // stays in the mel workspace until the gain kernel has read it
    const int* d_lens = (const int*)((const char*)e->stft.ws.p + g.fwd.off_info);
    timing_begin(e, 3);
    hipLaunchKernelGGL(fm_logmag_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, Y, logmag + n, d_source ? (float*)nullptr : logmag, n,
                       F, p.cut, p.NB, CK, w.info);
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    if (stop == FM_LOGMAG) return *view = StageView{logmag, (size_t)(2 * rows), (size_t)p.cut, (size_t)CK}, TTS_HIP_OK;
    timing_begin(e, 3);
    HIPCHK(e, gemm_small(gemm_linear(logmag, CK, CK, fn.lift_Bt, CK, p.cut, (int)(2 * rows), env), 1, st));
    timing_end(e);
    if (stop == FM_ENVELOPE) return *view = StageView{env, (size_t)(2 * rows), (size_t)p.cut, (size_t)p.cut}, TTS_HIP_OK;
    timing_begin(e, 4);
    hipLaunchKernelGGL(fm_gain_kernel, dim3(F, B), dim3(FM_THREADS), (size_t)p.cut * 4, st, Y, env, w.info, d_warps, w.operand,
                       stop == FM_GAIN ? gain : (float*)nullptr, rows, F, p.cut, p.NB, g.G);
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    if (stop == FM_GAIN) return *view = StageView{gain, (size_t)rows, (size_t)p.cut, (size_t)p.cut}, TTS_HIP_OK;
    if (stop == FM_OPERAND) return *view = StageView{w.operand, (size_t)rows, (size_t)2 * p.cut, (size_t)p.NB}, TTS_HIP_OK;
    timing_begin(e, 0);
    if (int rc = inverse_frames(e, fn, g.inv, w)) return rc;
    timing_end(e);
    if (stop == FM_FRAMES) return *view = StageView{w.tframes, (size_t)rows, (size_t)p.fl, (size_t)p.fl}, TTS_HIP_OK;
    timing_begin(e, 1);
    const long long cells = (long long)B * N;
    hipLaunchKernelGGL(ola_cut_kernel, dim3(blocks(cells, 256)), dim3(256), 0, st, w.tframes, fn.win2, d_out, cells, F, N, w.info, d_lens,
                       p.hop, p.fl, p.half, (float)((double)p.fl / p.hop));
    HIPCHK(e, hipGetLastError());
    timing_end(e);
    return TTS_HIP_OK;
}

// tts_hip_formant_match (what = -1), its probe (what = a stage) and the _async form (stream, device pointers)
int fm_call(tts_hip_engine* e, const char* name, const float* audio, const float* source, int B, int N, const int32_t* lengths,
            const tts_hip_mel_fn* fn, const double* warps, int Q, double max_gain_db, int what, float* out, int mem, bool async,
            void* stream) {
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    FmGeom g;
    char why[256];
    if (int rc = formant_match_check(name, fn ? &fn->p : nullptr, audio, B, N, lengths, warps, Q, max_gain_db, out, mem, what, &g, why,
                                     sizeof why))
        return set_err(e, rc, "%s", why);
    tts_hip_mel_fn* plan = const_cast<tts_hip_mel_fn*>(fn);
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = inv_tables(e, plan)) return rc;
    if (int rc = lift_table(e, plan, Q)) return rc;
    if (async) {
        StreamScope scope(e, stream);
        return fm_exec(e, *plan, g, audio, source, B, N, out, -1, nullptr);
    }
    const size_t n_audio = (size_t)B * N * 4;
    AudioStage io(e, mem);
    const int in = io.in(audio, n_audio), is = io.in(source, n_audio);
    const int res = what >= 0 ? io.scratch(n_audio) : io.out(out, n_audio);
    if (int rc = io.begin()) return rc;
    StageView view{};
    if (int rc = fm_exec(e, *plan, g, io.ptr<const float>(in), io.ptr<const float>(is), B, N, io.ptr<float>(res), what, &view)) return rc;
    if (what >= 0)
        if (int rc = copy_stage_out(e, view, out, mem)) return rc;
    const int rc = io.finish();
    timing_collect(e);
    return rc;
}

}  // namespace

int tts_hip_formant_match(tts_hip_engine* e, const float* audio, const float* source, int B, int N, const int32_t* lengths,
                          const tts_hip_mel_fn* fn, const double* warps, int lifter, double max_gain_db, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    return fm_call(e, "formant_match", audio, source, B, N, lengths, fn, warps, lifter, max_gain_db, -1, out, mem, false, nullptr);
}

int tts_hip_formant_match_async(tts_hip_engine* e, const float* audio, const float* source, int B, int N, const int32_t* lengths,
                                const tts_hip_mel_fn* fn, const double* warps, int lifter, double max_gain_db, float* out,
                                void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    return fm_call(e, "formant_match_async", audio, source, B, N, lengths, fn, warps, lifter, max_gain_db, -1, out, TTS_HIP_MEM_DEVICE,
                   true, stream);
}

int tts_hip_formant_match_probe(tts_hip_engine* e, const float* audio, const float* source, int B, int N, const int32_t* lengths,
                                const tts_hip_mel_fn* fn, const double* warps, int lifter, double max_gain_db, int what, float* out,
                                int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (what < 0) return set_err(e, TTS_HIP_EINVAL, "formant_match_probe: no stage %d (0 .. %d)", what, FM_STAGES - 1);
    return fm_call(e, "formant_match_probe", audio, source, B, N, lengths, fn, warps, lifter, max_gain_db, what, out, mem, false,
                   nullptr);
}

long long tts_hip_time_stretch_samples(const tts_hip_mel_fn* fn, int n_samples, double rate) {
    return fn ? ts_row_samples(fn->p, n_samples, rate) : -1;
}

int tts_hip_time_stretch_frames(const tts_hip_mel_fn* fn, int n_samples, double rate) {
    return fn ? ts_row_frames(fn->p, n_samples, rate) : -1;
}

int tts_hip_time_stretch(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const double* rates,
                         const tts_hip_mel_fn* fn, float* out, int M, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    return ts_call(e, "time_stretch", audio, B, N, lengths, rates, fn, -1, out, M, mem, false, nullptr);
}

int tts_hip_time_stretch_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const double* rates,
                               const tts_hip_mel_fn* fn, float* out, int M, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    return ts_call(e, "time_stretch_async", audio, B, N, lengths, rates, fn, -1, out, M, TTS_HIP_MEM_DEVICE, true, stream);
}

int tts_hip_time_stretch_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const double* rates,
                               const tts_hip_mel_fn* fn, int what, float* out, int M, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (what < 0) return set_err(e, TTS_HIP_EINVAL, "time_stretch_probe: no stage %d (0 .. %d)", what, TS_STAGES - 1);
    return ts_call(e, "time_stretch_probe", audio, B, N, lengths, rates, fn, what, out, M, mem, false, nullptr);
}

long long tts_hip_mel_fn_samples(const tts_hip_mel_fn* fn, int frames) { return fn ? stft_samples(fn->p, frames) : -1; }

int tts_hip_stft_transform(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                           int what, float* out0, float* out1, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    const char* name = "stft_transform";
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    MelGeom g;
    char why[256];
    if (!out1) return set_err(e, TTS_HIP_EINVAL, "%s: bad argument", name);
    if (int rc = mel_call_check(name, fn ? &fn->p : nullptr, audio, B, N, lengths, out0, mem, &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    if (fn->p.kind != TTS_HIP_MEL_TACOTRON) return set_err(e, TTS_HIP_EINVAL, "%s: refused for a Whisper plan", name);
    if (what < 0 || what > 1) return set_err(e, TTS_HIP_EINVAL, "%s: what %d not 0 (magnitude, phase) or 1 (real, imaginary)", name, what);
    HIPCHK(e, hipSetDevice(e->device));
    const MelPlan& p = fn->p;
    const size_t n_out = (size_t)B * g.Fout * p.cut;
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4);
    const int o0 = io.out(out0, n_out * 4), o1 = io.out(out1, n_out * 4);
    if (int rc = io.begin()) return rc;
    StageView view{};
    if (int rc = mel_fn_exec(e, *fn, g, io.ptr<const float>(in), B, N, lengths != nullptr, nullptr, MEL_SPECTRUM, &view)) return rc;
    // ragged: mel_fn_exec left [lens | fout] at the head of its workspace
    const int* d_fo = lengths ? (const int*)((const char*)e->stft.ws.p + g.off_info) + B : nullptr;
    hipLaunchKernelGGL(stft_polar_kernel, dim3(blocks((long long)n_out, 256)), dim3(256), 0, e->stream, (const float*)view.p,
                       io.ptr<float>(o0), io.ptr<float>(o1), (long long)n_out, g.Fr, g.Fout, p.cut, p.NB, d_fo, what);
    HIPCHK(e, hipGetLastError());
    return io.finish();
}

int tts_hip_stft_inverse(tts_hip_engine* e, const float* plane0, int B, int F, const float* plane1, const int32_t* frames,
                         const tts_hip_mel_fn* fn, int form, float* audio, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    const char* name = "stft_inverse";
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    GlGeom g;
    char why[256];
    if (int rc = stft_inv_check(name, fn ? &fn->p : nullptr, plane0, plane1, audio, B, F, fn ? fn->p.cut : 0, frames, -1, 0, 0.0, mem, -1,
                                0, &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    if (form < 0 || form > 1) return set_err(e, TTS_HIP_EINVAL, "%s: form %d not 0 (magnitude, phase) or 1 (real, imaginary)", name, form);
    tts_hip_mel_fn* plan = const_cast<tts_hip_mel_fn*>(fn);
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = inv_tables(e, plan)) return rc;
    const MelPlan& p = fn->p;
    const size_t n_in = (size_t)B * F * p.cut * 4;
    AudioStage io(e, mem);
    const int i0 = io.in(plane0, n_in), i1 = io.in(plane1, n_in);
    const int res = io.out(audio, (size_t)B * g.Sout * 4);
    if (int rc = io.begin()) return rc;
    GlBufs w;
    if (int rc = gl_bufs(e, g, &w)) return rc;
    const long long n = (long long)B * F * p.NB;
    hipLaunchKernelGGL(inv_operand_kernel, dim3(blocks(n, 256)), dim3(256), 0, e->stream, io.ptr<const float>(i0), io.ptr<const float>(i1),
                       w.operand, n, F, p.cut, p.NB, w.info, form);
    HIPCHK(e, hipGetLastError());
    if (int rc = inverse_frames(e, *plan, g, w)) return rc;
    if (int rc = overlap_add(e, *plan, g, w, io.ptr<float>(res), false)) return rc;
    return io.finish();
}

int tts_hip_griffin_lim(tts_hip_engine* e, const float* spec, int B, int F, int C, const int32_t* frames, const tts_hip_mel_fn* fn,
                        int input_kind, const double* Minv, const float* init, int n_iters, double momentum, float* audio, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    return gl_call(e, "griffin_lim", spec, B, F, C, frames, fn, input_kind, Minv, init, n_iters, momentum, 0, -1, audio, mem, false,
                   nullptr);
}

int tts_hip_griffin_lim_async(tts_hip_engine* e, const float* spec, int B, int F, int C, const int32_t* frames,
                              const tts_hip_mel_fn* fn, int input_kind, const double* Minv, const float* init, int n_iters,
                              double momentum, float* audio, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    return gl_call(e, "griffin_lim_async", spec, B, F, C, frames, fn, input_kind, Minv, init, n_iters, momentum, 0, -1, audio,
                   TTS_HIP_MEM_DEVICE, true, stream);
}

int tts_hip_griffin_lim_probe(tts_hip_engine* e, const float* spec, int B, int F, int C, const int32_t* frames,
                              const tts_hip_mel_fn* fn, int input_kind, const double* Minv, const float* init, int n_iters,
                              double momentum, int k, int what, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (what < 0) return set_err(e, TTS_HIP_EINVAL, "griffin_lim_probe: no stage %d (0 .. %d)", what, GL_STAGES - 1);
    return gl_call(e, "griffin_lim_probe", spec, B, F, C, frames, fn, input_kind, Minv, init, n_iters, momentum, k, what, out, mem, false,
                   nullptr);
}

int tts_hip_denoise(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                    const float* bias, double strength, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    return dn_call(e, "denoise", audio, B, N, lengths, fn, bias, strength, -1, out, mem, false, nullptr);
}

int tts_hip_denoise_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                          const float* bias, double strength, float* out, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    return dn_call(e, "denoise_async", audio, B, N, lengths, fn, bias, strength, -1, out, TTS_HIP_MEM_DEVICE, true, stream);
}

int tts_hip_denoise_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                          const float* bias, double strength, int what, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (what < 0) return set_err(e, TTS_HIP_EINVAL, "denoise_probe: no stage %d (0 .. %d)", what, DN_STAGES - 1);
    return dn_call(e, "denoise_probe", audio, B, N, lengths, fn, bias, strength, what, out, mem, false, nullptr);
}
