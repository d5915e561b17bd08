// resample.hip -- FFT resampling on gfx950: scipy.signal.resample(x, M) (window=None) per row, any N and M.
//
// utils/audio/audio_processing.py:30-35 resamples with scipy.signal.resample(audio, int(len(audio) / rate * target_rate)):
// X = rfft_N(x); Y = X[0 .. n//2] (n = min(N, M)) zero-padded to M//2 + 1 bins, its bin n/2 doubled (M < N) or halved
// (M > N) when n is even; y = irfft_M(Y) * (M / N).  Both transforms have arbitrary lengths, so each is a Bluestein chain:
// with the chirp w_j = exp(-i pi j^2 / K) (phase j^2 mod 2K in 64-bit integers, sine and cosine in fp64, rounded once),
// DFT_K(a)[k] = w_k * sum_j (a_j w_j) conj(w_{k-j}), a circular convolution of power-of-two length L taken with complex
// fp32 FFTs: FFT(signal), FFT(filter), product, inverse FFT.
//   forward  (K = N): only bins 0 .. N//2 are kept, so L >= N + N//2 avoids wrap-around;
//   inverse  (K = M): irfft_M(Y)[j] = Re(DFT_M(conj(Z))[j]) / M with Z the Hermitian extension of Y (imaginary parts of
//            bin 0 and, M even, bin M/2 dropped, as numpy does); all M outputs are needed, so L >= 2M - 1.
// The cheap steps ride in the FFT passes: the chirp pre-multiply and the zero padding in the first pass's loads, the
// pointwise product with the filter's spectrum in the inverse FFT's loads, the post-chirp and 1/L in its last stores, the
// spectrum fix-up (truncate / zero-pad, Nyquist x2 or x0.5, Hermitian extension, conjugate) in the loads of the second
// chain, and the M/N scale in the final stores.  The filter spectrum is a second line of the same forward FFT.
//
// FFT: radix-4 Stockham (a radix-2 stage when log2 P is odd) on up to 8192 complex fp32 points in LDS (64 KiB), 256 threads.
// L <= 8192 is one workgroup per line; a larger L = 8192 * L2 is the four-step split: L2-point FFTs down the columns (8192 /
// L2 adjacent columns per workgroup), the twiddle W_L^(n1 k2), then 8192-point FFTs along the rows.  The forward transform
// leaves its spectrum in that transposed order and the inverse transform (the same passes reversed) takes it back, so
// the pointwise product never needs the natural order.  Twiddles: W_8192^j as a float2 table built in fp64 on the host;
// the four-step ones from sincospi in fp64 per element.
//
// Rows of a batch with the same pair (L_fwd, L_inv) share one chain of launches; every row's work depends only on its own
// N_b and M_b, so a row's result is bitwise a one-row call's.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

namespace {

constexpr int PMAX = 8192, LOG_PMAX = 13;          // points per workgroup (64 KiB of LDS)
constexpr int NT = 256;                            // threads per workgroup

enum { LD_PLAIN, LD_FWD_IN, LD_PROD, LD_INV_IN };
enum { ST_PLAIN, ST_FWD_OUT, ST_INV_OUT };

struct RsPass {
    int P, logP, nl, lognl;     // points per line, lines per workgroup
    int L;                      // transform length of the stage (line stride of U)
    int sstride, estride;       // offset of element j of sub-line s: s * sstride + j * estride
    int twiddle;                // four-step: multiply output (s, j) by W_L^(+-s j)
    int G;                      // rows of the group (stage lines: G signals, then G filters for the forward FFTs)
    const int* rows;            // [G] batch row of each group row
    const int* nlen;            // [B] N_b
    const int* mlen;            // [B] M_b
    float2* U;                  // [lines][L]
    float2* X;                  // [G][xstride] rfft bins 0 .. N_b // 2 of each row
    int xstride;
    const float* in;            // [B][N]
    long long in_ld;
    float* out;                 // [B][M]
    long long out_ld;
};

__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 conjf2(float2 a) { return make_float2(a.x, -a.y); }

// exp(-i pi j^2 / K), the phase reduced exactly (j^2 mod 2K, 64-bit) and evaluated in fp64
__device__ inline float2 chirp(long long j, int K) {
    const unsigned long long r = (unsigned long long)(j * j) % (2ull * (unsigned long long)K);
    double s, c;
    sincospi((double)r / (double)K, &s, &c);
    return make_float2((float)c, (float)-s);
}

// Bluestein filter of a K-point transform on L points, K_out outputs wanted: conj(w_j) for j < K_out, conj(w_(L-j)) for
// L - j < K, zero between (L >= K + K_out - 1, so the two ends never meet)
__device__ inline float2 chirp_filter(int j, int K, int K_out, int L) {
    if (j < K_out) return conjf2(chirp(j, K));
    if (L - j < K) return conjf2(chirp(L - j, K));
    return make_float2(0.f, 0.f);
}

// W_L^(e) with sign -1 (forward) or +1 (inverse), fp64, L a power of two
__device__ inline float2 twiddle_L(long long e, int L, bool inv) {
    double s, c;
    sincospi(2.0 * (double)e / (double)L, &s, &c);
    return make_float2((float)c, inv ? (float)s : (float)-s);
}

template <bool INV>
__device__ inline void radix4(float2& a0, float2& a1, float2& a2, float2& a3) {
    const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
    // forward: X1 = d02 - i d13, X3 = d02 + i d13; inverse: the other way round
    const float2 mi = INV ? make_float2(-d13.y, d13.x) : make_float2(d13.y, -d13.x);    // (-+i) * d13
    a0 = make_float2(s02.x + s13.x, s02.y + s13.y);
    a2 = make_float2(s02.x - s13.x, s02.y - s13.y);
    a1 = make_float2(d02.x + mi.x, d02.y + mi.y);
    a3 = make_float2(d02.x - mi.x, d02.y - mi.y);
}

// Stockham FFT of `nl` lines of P = 2^logP points at lds[c * P + j] (nl * P <= PMAX), in place with a barrier between the
// reads and the writes of each stage.  Caller has synchronised after filling lds; returns synchronised.
template <bool INV>
__device__ void lds_fft(float2* lds, int logP, int nl, const float2* __restrict__ tw) {
    const int P = 1 << logP, tid = threadIdx.x;
    int Ns = 1, logNs = 0;
    for (; logNs + 2 <= logP; logNs += 2, Ns <<= 2) {
        const int q = P >> 2, nbf = nl * q;
        float2 v[PMAX / 4 / NT][4];
#pragma unroll
        for (int i = 0; i < PMAX / 4 / NT; ++i) {
            const int t = tid + i * NT;
            if (t < nbf) {
                const int line = t >> (logP - 2), jj = t & (q - 1), k = jj & (Ns - 1);
                const float2* base = lds + line * P;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[i][r] = base[jj + r * q];
                if (Ns > 1) {
                    const int step = k << (LOG_PMAX - logNs - 2);      // W_(4 Ns)^k = W_8192^(k * 8192 / (4 Ns))
#pragma unroll
                    for (int r = 1; r < 4; ++r) {
                        float2 w = tw[r * step];
                        if (INV) w.y = -w.y;
                        v[i][r] = cmul(v[i][r], w);
                    }
                }
                radix4<INV>(v[i][0], v[i][1], v[i][2], v[i][3]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PMAX / 4 / NT; ++i) {
            const int t = tid + i * NT;
            if (t < nbf) {
                const int line = t >> (logP - 2), jj = t & (q - 1), k = jj & (Ns - 1);
                float2* base = lds + line * P + ((jj >> logNs) << (logNs + 2)) + k;
#pragma unroll
                for (int r = 0; r < 4; ++r) base[r * Ns] = v[i][r];
            }
        }
        __syncthreads();
    }
    if (logNs < logP) {                                                 // one radix-2 stage (log2 P odd)
        const int h = P >> 1, nbf = nl * h;
        float2 v[PMAX / 2 / NT][2];
#pragma unroll
        for (int i = 0; i < PMAX / 2 / NT; ++i) {
            const int t = tid + i * NT;
            if (t < nbf) {
                const int line = t >> (logP - 1), jj = t & (h - 1), k = jj & (Ns - 1);
                const float2* base = lds + line * P;
                v[i][0] = base[jj];
                v[i][1] = base[jj + h];
                if (Ns > 1) {
                    float2 w = tw[k << (LOG_PMAX - logNs - 1)];
                    if (INV) w.y = -w.y;
                    v[i][1] = cmul(v[i][1], w);
                }
                const float2 a = v[i][0], b = v[i][1];
                v[i][0] = make_float2(a.x + b.x, a.y + b.y);
                v[i][1] = make_float2(a.x - b.x, a.y - b.y);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PMAX / 2 / NT; ++i) {
            const int t = tid + i * NT;
            if (t < nbf) {
                const int line = t >> (logP - 1), jj = t & (h - 1), k = jj & (Ns - 1);
                float2* base = lds + line * P + ((jj >> logNs) << (logNs + 1)) + k;
                base[0] = v[i][0];
                base[Ns] = v[i][1];
            }
        }
        __syncthreads();
    }
}

// One FFT pass over the lines of a group: load (LD) -> P-point FFT per line in LDS -> optional four-step twiddle -> store
// (ST).  blockIdx.x = stage line, blockIdx.y = block of nl sub-lines.  Offsets within a line are < L <= 2^26.
template <int LD, int ST, bool INV>
__global__ __launch_bounds__(NT) void rs_fft_kernel(RsPass p, const float2* __restrict__ tw) {
    __shared__ float2 lds[PMAX];
    const int line = blockIdx.x, row = line < p.G ? line : line - p.G, b = p.rows[row];
    const int Nb = p.nlen[b], Mb = p.mlen[b];
    const int s0 = blockIdx.y * p.nl, total = p.nl << p.logP;
    const bool sfast = p.estride != 1;                  // strided pass: adjacent threads on adjacent columns
    float2* U = p.U + (size_t)line * p.L;
    for (int e = threadIdx.x; e < total; e += NT) {
        const int c = sfast ? (e & (p.nl - 1)) : (e >> p.logP), j = sfast ? (e >> p.lognl) : (e & (p.P - 1));
        const int off = (s0 + c) * p.sstride + j * p.estride;
        float2 v;
        if (LD == LD_PLAIN) {
            v = U[off];
        } else if (LD == LD_PROD) {
            v = cmul(U[off], p.U[(size_t)(line + p.G) * p.L + off]);
        } else if (LD == LD_FWD_IN) {                   // a_j = x_j w_j (j < N_b), or the filter of the N_b-point DFT
            if (line < p.G)
                v = off < Nb ? cmul(make_float2(p.in[(size_t)b * p.in_ld + off], 0.f), chirp(off, Nb)) : make_float2(0.f, 0.f);
            else
                v = chirp_filter(off, Nb, Nb / 2 + 1, p.L);
        } else {                                        // LD_INV_IN: conj(Z_j) w_j, or the filter of the M_b-point DFT
            if (line < p.G) {
                v = make_float2(0.f, 0.f);
                if (off < Mb) {
                    const bool mirror = off > Mb / 2;
                    const int k = mirror ? Mb - off : off, n = min(Nb, Mb);
                    if (k <= n / 2) {
                        float2 y = p.X[(size_t)row * p.xstride + k];
                        if ((n & 1) == 0 && k == n / 2 && Mb != Nb) {     // M == N (rates differ, lengths equal): kept
                            const float f = Mb < Nb ? 2.f : 0.5f;
                            y = make_float2(y.x * f, y.y * f);
                        }
                        if (k == 0 || ((Mb & 1) == 0 && k == Mb / 2)) y.y = 0.f;
                        v = cmul(mirror ? y : conjf2(y), chirp(off, Mb));
                    }
                }
            } else {
                v = chirp_filter(off, Mb, Mb, p.L);
            }
        }
        lds[(c << p.logP) + j] = v;
    }
    __syncthreads();
    lds_fft<INV>(lds, p.logP, p.nl, tw);
    for (int e = threadIdx.x; e < total; e += NT) {
        const int c = sfast ? (e & (p.nl - 1)) : (e >> p.logP), j = sfast ? (e >> p.lognl) : (e & (p.P - 1));
        const int s = s0 + c, off = s * p.sstride + j * p.estride;
        float2 v = lds[(c << p.logP) + j];
        if (p.twiddle) v = cmul(v, twiddle_L((long long)s * j, p.L, INV));
        if (ST == ST_PLAIN) {
            U[off] = v;
        } else if (ST == ST_FWD_OUT) {                  // X_k = w_k c_k / L for the bins 0 .. N_b // 2
            if (off <= Nb / 2) {
                const float inv_l = 1.f / (float)p.L;
                const float2 x = cmul(v, chirp(off, Nb));
                p.X[(size_t)row * p.xstride + off] = make_float2(x.x * inv_l, x.y * inv_l);
            }
        } else {                                        // ST_INV_OUT: y_j = Re(w_j c_j) / L / M * (M / N)
            if (off < Mb) {
                const float scale = (float)((double)Mb / (double)Nb / (double)Mb / (double)p.L);
                const float2 w = chirp(off, Mb);
                p.out[(size_t)b * p.out_ld + off] = (v.x * w.x - v.y * w.y) * scale;
            }
        }
    }
}

// out[b, M_b:M] = 0; blockIdx.x = row
__global__ void rs_zero_tail_kernel(float* out, long long M, const int* mlen) {
    const int b = blockIdx.x;
    for (long long j = mlen[b] + (long long)blockIdx.y * blockDim.x + threadIdx.x; j < M; j += (long long)gridDim.y * blockDim.x)
        out[(size_t)b * M + j] = 0.f;
}

}  // namespace

void resample_free(tts_hip_engine* e) {
    ResampleDev& r = e->resamp;
    r.tw.release();
    r.ws.release();
}

namespace {

// W_8192^j = exp(-2 pi i j / 8192), j < 8192, evaluated in fp64 and rounded to float2 once; built on first use
int rs_twiddles(tts_hip_engine* e) {
    ResampleDev& r = e->resamp;
    if (r.tw.p) return TTS_HIP_OK;
    std::vector<float> h(2 * PMAX);
    for (int j = 0; j < PMAX; ++j) {
        const double a = 2.0 * M_PI * (double)j / PMAX;
        h[2 * j] = (float)std::cos(a);
        h[2 * j + 1] = (float)-std::sin(a);
    }
    HIPCHK(e, r.tw.ensure(h.size() * 4));
    hipError_t err = hipMemcpy(r.tw.p, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        r.tw.release();
        HIPCHK(e, err);
    }
    return TTS_HIP_OK;
}

// one Bluestein FFT (LD -> ST) of `lines` lines of 2^logL points: one pass in LDS, or the four-step pair
template <int LD, int ST, bool INV>
hipError_t rs_fft(RsPass p, int logL, int lines, const float2* tw, hipStream_t st) {
    p.L = 1 << logL;
    if (logL <= LOG_PMAX) {
        p.P = p.L;
        p.logP = logL;
        p.nl = 1;
        p.lognl = 0;
        p.sstride = 0;
        p.estride = 1;
        p.twiddle = 0;
        hipLaunchKernelGGL((rs_fft_kernel<LD, ST, INV>), dim3(lines, 1), dim3(NT), 0, st, p, tw);
        return hipGetLastError();
    }
    const int log2 = logL - LOG_PMAX;                   // L = 8192 (row length L1) x L2 rows
    RsPass col = p, row = p;
    col.P = 1 << log2;                                  // columns: L2 points, stride L1, 8192 / L2 adjacent columns
    col.logP = log2;
    col.nl = PMAX >> log2;
    col.lognl = LOG_PMAX - log2;
    col.sstride = 1;
    col.estride = PMAX;
    row.P = PMAX;                                       // rows: 8192 contiguous points
    row.logP = LOG_PMAX;
    row.nl = 1;
    row.lognl = 0;
    row.sstride = PMAX;
    row.estride = 1;
    const dim3 grid(lines, 1u << log2);                 // both passes: L / 8192 workgroups per line
    if (!INV) {                                         // columns (with the loads) and twiddle, then rows
        col.twiddle = 1;
        row.twiddle = 0;
        hipLaunchKernelGGL((rs_fft_kernel<LD, ST_PLAIN, INV>), grid, dim3(NT), 0, st, col, tw);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL((rs_fft_kernel<LD_PLAIN, ST, INV>), grid, dim3(NT), 0, st, row, tw);
    } else {                                            // rows (with the loads) and twiddle, then columns
        row.twiddle = 1;
        col.twiddle = 0;
        hipLaunchKernelGGL((rs_fft_kernel<LD, ST_PLAIN, INV>), grid, dim3(NT), 0, st, row, tw);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL((rs_fft_kernel<LD_PLAIN, ST, INV>), grid, dim3(NT), 0, st, col, tw);
    }
    return hipGetLastError();
}

// device pointers only; arguments validated by rs_check.  spectra (tts_hip_resample_probe; [B][N // 2 + 1] bins, device): every
// group stops after its forward chain and its rows' bins 0 .. N_b // 2 go there, zeros behind them; d_out is not touched
int resample_run(tts_hip_engine* e, const float* d_in, int B, int N, const std::vector<int>& lens, const std::vector<int>& mlens,
                 float* d_out, int M, float2* spectra = nullptr) {
    ResampleDev& r = e->resamp;
    if (int rc = rs_twiddles(e)) return rc;
    hipStream_t st = e->stream;
    // group the rows by (L_fwd, L_inv); workspace = the largest group's [2G][max L] complex lines + [G][max N_b//2 + 1] bins
    std::map<std::pair<int, int>, std::vector<int>> groups;
    for (int b = 0; b < B; ++b) {
        const RsLens l = rs_lens(lens[b], mlens[b]);
        groups[{l.logf, l.logi}].push_back(b);
    }
    size_t lines = 0;
    std::vector<int> xstride;
    for (auto& g : groups) {
        int xs = 0;
        for (int b : g.second) xs = std::max(xs, lens[b] / 2 + 1);
        xstride.push_back(xs);
        const size_t G = g.second.size();
        const size_t L = (size_t)1 << std::max(g.first.first, g.first.second);
        lines = std::max(lines, al256(2 * G * L * 8) + al256(G * (size_t)xs * 8));
    }
    Carve ws;
    const size_t off_info = ws.take((size_t)3 * B * 4), off_lines = ws.take(lines);
    HIPCHK(e, r.ws.ensure(ws.o));
    int* d_info = (int*)((char*)r.ws.p + off_info);
    char* base = (char*)r.ws.p + off_lines;
    // [0, B) N_b, [B, 2B) M_b, [2B, 3B) the batch rows of each group in turn
    std::vector<int>& info_h = e->audio_info_h;
    info_h.assign((size_t)3 * B, 0);
    for (int b = 0; b < B; ++b) {
        info_h[b] = lens[b];
        info_h[B + b] = mlens[b];
    }
    int k = 2 * B;
    for (auto& g : groups)
        for (int b : g.second) info_h[k++] = b;
    if (int rc = stage_row_info(e, d_info)) return rc;
    const float2* tw = (const float2*)r.tw.p;
    const size_t sp_ld = (size_t)N / 2 + 1;
    if (spectra) HIPCHK(e, hipMemsetAsync(spectra, 0, (size_t)B * sp_ld * 8, st));
    int first = 2 * B, gi = 0;
    for (auto& g : groups) {
        const int G = (int)g.second.size(), logf = g.first.first, logi = g.first.second;
        const size_t L = (size_t)1 << std::max(logf, logi);
        RsPass p{};
        p.G = G;
        p.rows = d_info + first;
        p.nlen = d_info;
        p.mlen = d_info + B;
        p.U = (float2*)base;
        p.X = (float2*)(base + al256(2 * (size_t)G * L * 8));
        p.xstride = xstride[gi];
        p.in = d_in;
        p.in_ld = N;
        p.out = d_out;
        p.out_ld = M;
        // rfft_N: FFT of signal and filter lines, then the inverse FFT of their product -> X (bins 0 .. N_b // 2)
        HIPCHK(e, (rs_fft<LD_FWD_IN, ST_PLAIN, false>(p, logf, 2 * G, tw, st)));
        HIPCHK(e, (rs_fft<LD_PROD, ST_FWD_OUT, true>(p, logf, G, tw, st)));
        if (spectra) {                                  // the probe's copy-out, in place of the second chain
            for (int i = 0; i < G; ++i) {
                const int b = g.second[i];
                HIPCHK(e, hipMemcpyAsync(spectra + (size_t)b * sp_ld, p.X + (size_t)i * p.xstride, ((size_t)lens[b] / 2 + 1) * 8,
                                         hipMemcpyDeviceToDevice, st));
            }
        } else {
            // irfft_M of the fixed-up spectrum: the same chain on L_inv, the stage buffer reused
            HIPCHK(e, (rs_fft<LD_INV_IN, ST_PLAIN, false>(p, logi, 2 * G, tw, st)));
            HIPCHK(e, (rs_fft<LD_PROD, ST_INV_OUT, true>(p, logi, G, tw, st)));
        }
        first += G;
        ++gi;
    }
    if (spectra) return TTS_HIP_OK;
    bool ragged = false;
    for (int b = 0; b < B; ++b) ragged |= mlens[b] != M;
    if (ragged) {
        hipLaunchKernelGGL(rs_zero_tail_kernel, dim3(B, (unsigned)std::min(4096, (M + 255) / 256)), dim3(256), 0, st, d_out,
                           (long long)M, d_info + B);
        HIPCHK(e, hipGetLastError());
    }
    return TTS_HIP_OK;
}

// rate == target_rate: the rows as they are (zero beyond lengths[b]), copies only, nothing launched
int rs_copy_rows(tts_hip_engine* e, const float* in, int B, int N, const std::vector<int>& lens, float* out, hipMemcpyKind kind,
                 hipStream_t st) {
    for (int b = 0; b < B; ++b) {
        const size_t o = (size_t)b * N, L = (size_t)lens[b];
        if (kind == hipMemcpyHostToHost) {
            std::memcpy(out + o, in + o, L * 4);
            std::memset(out + o + L, 0, (N - L) * 4);
        } else {
            HIPCHK(e, hipMemcpyAsync(out + o, in + o, L * 4, kind, st));
            if (L < (size_t)N) HIPCHK(e, hipMemsetAsync(out + o + L, 0, (N - L) * 4, st));
        }
    }
    return TTS_HIP_OK;
}

}  // namespace

int tts_hip_resample_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate,
                           int target_rate, float* out, int M, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    std::vector<int> lens, mlens;
    char why[256];
    if (int rc = rs_check("resample_async", audio, B, N, lengths, rate, target_rate, out, M, TTS_HIP_MEM_DEVICE, lens, mlens, why,
                          sizeof why))
        return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    StreamScope scope(e, stream);
    if (rate == target_rate) return rs_copy_rows(e, audio, B, N, lens, out, hipMemcpyDeviceToDevice, e->stream);
    return resample_run(e, audio, B, N, lens, mlens, out, M);
}

int tts_hip_resample(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int target_rate,
                     float* out, int M, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    std::vector<int> lens, mlens;
    char why[256];
    if (int rc = rs_check("resample", audio, B, N, lengths, rate, target_rate, out, M, mem, lens, mlens, why, sizeof why))
        return set_err(e, rc, "%s", why);
    if (rate == target_rate && mem == TTS_HIP_MEM_HOST) return rs_copy_rows(e, audio, B, N, lens, out, hipMemcpyHostToHost, nullptr);
    HIPCHK(e, hipSetDevice(e->device));
    if (rate == target_rate) {
        if (int rc = rs_copy_rows(e, audio, B, N, lens, out, hipMemcpyDeviceToDevice, e->stream)) return rc;
        HIPCHK(e, hipStreamSynchronize(e->stream));
        return TTS_HIP_OK;
    }
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4), res = io.out(out, (size_t)B * M * 4);
    if (int rc = io.begin()) return rc;
    if (int rc = resample_run(e, io.ptr<const float>(in), B, N, lens, mlens, io.ptr<float>(res), M)) return rc;
    return io.finish();
}

// Test hook: resample_run on the same arguments (the same groups and launches) up to the end of the forward chain, then every
// row's rfft bins 0 .. N_b // 2 out of the workspace to `spectrum` [B][N // 2 + 1][2].
int tts_hip_resample_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int target_rate,
                           float* spectrum, int M, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    std::vector<int> lens, mlens;
    char why[256];
    if (int rc = rs_check("resample_probe", audio, B, N, lengths, rate, target_rate, spectrum, M, mem, lens, mlens, why, sizeof why))
        return set_err(e, rc, "%s", why);
    if (rate == target_rate) return set_err(e, TTS_HIP_EINVAL, "resample_probe: rate == target_rate = %d runs no transform", rate);
    HIPCHK(e, hipSetDevice(e->device));
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4), res = io.out(spectrum, (size_t)B * (N / 2 + 1) * 8);
    if (int rc = io.begin()) return rc;
    if (int rc = resample_run(e, io.ptr<const float>(in), B, N, lens, mlens, nullptr, M, io.ptr<float2>(res))) return rc;
    return io.finish();
}

// Test hook: rs_fft<LD_PLAIN, ST_PLAIN> on `lines` lines of 2^logL complex points, host memory in and out.
int tts_hip_resample_fft_probe(tts_hip_engine* e, const float* in, int lines, int logL, int inverse, float* out) {
    if (!e) return TTS_HIP_EINVAL;
    char why[256];
    if (int rc = rs_fft_probe_check("resample_fft_probe", in, lines, logL, out, why, sizeof why)) return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    ResampleDev& r = e->resamp;
    if (int rc = rs_twiddles(e)) return rc;
    hipStream_t st = e->stream;
    const size_t bytes = ((size_t)lines << logL) * 8;
    Carve ws;
    const size_t off_info = ws.take(((size_t)lines + 2) * 4), off_lines = ws.take(bytes);
    HIPCHK(e, r.ws.ensure(ws.o));
    int* d_info = (int*)((char*)r.ws.p + off_info);
    // the kernel reads rows / nlen / mlen whatever it loads: every line is "row 0" of one sample in, one out
    e->audio_info_h.assign((size_t)lines + 2, 0);
    e->audio_info_h[lines] = e->audio_info_h[lines + 1] = 1;
    if (int rc = stage_row_info(e, d_info)) return rc;
    RsPass p{};
    p.G = lines;
    p.rows = d_info;
    p.nlen = d_info + lines;
    p.mlen = d_info + lines + 1;
    p.U = (float2*)((char*)r.ws.p + off_lines);
    HIPCHK(e, hipMemcpyAsync(p.U, in, bytes, hipMemcpyHostToDevice, st));
    if (inverse)
        HIPCHK(e, (rs_fft<LD_PLAIN, ST_PLAIN, true>(p, logL, lines, (const float2*)r.tw.p, st)));
    else
        HIPCHK(e, (rs_fft<LD_PLAIN, ST_PLAIN, false>(p, logL, lines, (const float2*)r.tw.p, st)));
    HIPCHK(e, hipMemcpyAsync(out, p.U, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return TTS_HIP_OK;
}
