// audio_proc.hip -- waveform clean-up on gfx950: spectral-gating noise reduction and window-method silence trimming.
//
// reduce_noise replaces utils/audio/noisereducev1.py:175-290 with the defaults utils/audio/audio_processing.py:65-83 uses
// (n_fft = win = 2048, hop 512, n_grad_freq 2, n_grad_time 4, n_std_thresh 1.5, prop_decrease 1, pad_clipping on, librosa
// centre padding with zeros).  Both DFTs are dense products on the fp32 MFMA GEMM (gemm_f32.h), like mel_stft.hip: the
// frames are overlapping rows (stride = hop) of the padded signal and are never materialised; the inverse basis carries the
// irfft scaling and the synthesis window, and the overlap-add is a gather (<= 4 frames per sample, no atomics).
// trim_silence replaces audio_processing.py:274-370 (method 'window': power 2, triangular window, adaptive thresholds,
// max_trim_factor 5): np.convolve(x^2, window, 'valid') as a direct fp64 sum, then the thresholds and indices per row.
//
// Every row b has its own length L_b <= N; nothing reads across a row's end, and a row's result equals a one-row call on
// audio[b, :L_b].
#include "engine.h"
#include "audio_dev.h"
#include "gemm_f32.h"

#include <cfloat>
#include <cmath>
#include <cstring>

using namespace ttsgemm;
using namespace rn;                          // NFFT, HOP, HALF, NBIN, NK (audio_call.h)

namespace {

constexpr int TRIM_OUT = 1024;               // conv outputs per block of the trim convolution (256 threads x 4)
constexpr int TRIM_JC = 1024;                // window taps staged in LDS per pass

// per-row facts shared by the kernels: [0] L_b, [1] F_b signal frames, [2] noise clip length, [3] noise frames
struct RowInfo {
    const int* p;
    int B;
    __device__ int len(int b) const { return p[b]; }
    __device__ int frames(int b) const { return p[B + b]; }
    __device__ int nlen(int b) const { return p[2 * B + b]; }
    __device__ int nframes(int b) const { return p[3 * B + b]; }
};

// dst[b][p] = src[b][p - 1024] for p - 1024 in [0, len_b), else 0; rows of dst are NPd floats apart and the `total`
// extent covers B * NPd plus the slack read by the last frames
__global__ void audio_pad_rows_kernel(const float* __restrict__ src, long long src_ld, const int* __restrict__ lens,
                                      float* __restrict__ dst, int NPd, int B, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int b = (int)(idx / NPd), p = (int)(idx % NPd);
    float v = 0.f;
    if (b < B) {
        const int s = p - HALF;
        if (s >= 0 && s < lens[b]) v = src[b * src_ld + s];
    }
    dst[idx] = v;
}

// |X|^2 with its two roundings spelled out.  Left to the compiler, re * re + im * im contracts one way in a loop's unrolled
// body and another way in its remainder, so the same cell gave row maxima one ulp apart under two grid sizes (signal and
// noise launch), and the two top_db floors that must tie did not.
__device__ __forceinline__ float power_of(float re, float im) { return __fmaf_rn(re, re, __fmul_rn(im, im)); }

// pmax[b] = max |X|^2 over the row's frames f < F_b (fp32 bit patterns of non-negative values order as unsigned)
__global__ void audio_power_max_kernel(const float* __restrict__ S, int Fr, const int* __restrict__ fcount,
                                       unsigned* __restrict__ pmax) {
    const int b = blockIdx.y;
    const long long n = (long long)fcount[b] * NBIN;
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long f = i / NBIN, k = i % NBIN;
        const float* row = S + ((long long)b * Fr + f) * NK;
        const float re = row[k], im = row[NBIN + k];
        m = fmaxf(m, power_of(re, im));
    }
    __shared__ float wm[4];
    m = block_reduce(m, wm, OpMax());
    if (threadIdx.x == 0) atomicMax(pmax + b, __float_as_uint(m));
}

// librosa.amplitude_to_db(|X|, ref=1, amin=1e-20, top_db=80) (noisereducev1.py:66-67): 10 log10(max(p, 1e-40)) clamped in
// the log domain (1e-40 is an fp32 denormal that flushes to zero), then max(v, rowmax - 80).  The logarithm is taken in
// double and rounded once: 10.f * log10f(p) rounds twice on top of log10f's own error, which near -100 dB is 2e-5 dB.
__device__ __forceinline__ float power_db(float p) { return fmaxf((float)(10.0 * log10((double)p)), -400.f); }

// thresh[b][k] = mean + 1.5 std (population) of the noise clip's dB over its frames (noisereducev1.py:244-247), fp64 sums
__global__ void audio_noise_thresh_kernel(const float* __restrict__ Sn, int Frn, RowInfo info,
                                          const unsigned* __restrict__ pmax_n, float* __restrict__ thresh) {
    const int b = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= NBIN) return;
    const int F = info.nframes(b);
    const float floor_db = power_db(__uint_as_float(pmax_n[b])) - 80.f;
    const float* base = Sn + (long long)b * Frn * NK;
    double s = 0.0;
    for (int f = 0; f < F; ++f) {
        const float re = base[(long long)f * NK + k], im = base[(long long)f * NK + NBIN + k];
        s += (double)fmaxf(power_db(power_of(re, im)), floor_db);
    }
    const double mean = s / F;
    double q = 0.0;
    for (int f = 0; f < F; ++f) {
        const float re = base[(long long)f * NK + k], im = base[(long long)f * NK + NBIN + k];
        const double d = (double)fmaxf(power_db(power_of(re, im)), floor_db) - mean;
        q += d * d;
    }
    thresh[b * NBIN + k] = (float)(mean + 1.5 * sqrt(q / F));
}

// mask[b][f][k] = dB(X) < thresh[b][k] for f < F_b, else 0 (noisereducev1.py:252-259)
__global__ void audio_gate_mask_kernel(const float* __restrict__ S, int Fr, RowInfo info, const unsigned* __restrict__ pmax,
                                       const float* __restrict__ thresh, uint8_t* __restrict__ mask) {
    const int b = blockIdx.z, f = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= NBIN) return;
    uint8_t v = 0;
    if (f < info.frames(b)) {
        const float* row = S + ((long long)b * Fr + f) * NK;
        const float re = row[k], im = row[NBIN + k];
        const float db = fmaxf(power_db(power_of(re, im)), power_db(__uint_as_float(pmax[b])) - 80.f);
        v = db < thresh[b * NBIN + k] ? 1 : 0;
    }
    mask[((long long)b * Fr + f) * NBIN + k] = v;
}

// probe only: the mask as 0.f / 1.f
__global__ void audio_mask_f32_kernel(const uint8_t* __restrict__ mask, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)mask[i];
}

// X *= 1 - smooth(mask): the 5 x 9 filter outer([1,2,3,2,1]/3, [1,2,3,4,5,4,3,2,1]/5)/15 (noisereducev1.py:81-106) as an
// integer stencil over 225, zero outside bins 0..1024 and frames 0..F_b-1 (fftconvolve 'same', :142); frames >= F_b -> 0
__global__ void audio_gate_apply_kernel(float* __restrict__ S, int Fr, RowInfo info, const uint8_t* __restrict__ mask) {
    const int b = blockIdx.z, f = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= NBIN) return;
    const int F = info.frames(b);
    float* row = S + ((long long)b * Fr + f) * NK;
    if (f >= F) {
        row[k] = 0.f;
        row[NBIN + k] = 0.f;
        return;
    }
    const int wf[5] = {1, 2, 3, 2, 1};
    const int wt[9] = {1, 2, 3, 4, 5, 4, 3, 2, 1};
    int acc = 0;
    for (int dt = -4; dt <= 4; ++dt) {
        const int ff = f + dt;
        if (ff < 0 || ff >= F) continue;
        const uint8_t* mr = mask + ((long long)b * Fr + ff) * NBIN;
        int s = 0;
        for (int df = -2; df <= 2; ++df) {
            const int kk = k + df;
            if (kk >= 0 && kk < NBIN) s += wf[df + 2] * mr[kk];
        }
        acc += wt[dt + 4] * s;
    }
    const float g = (float)(225 - acc) / 225.f;
    row[k] *= g;
    row[NBIN + k] *= g;
}

// out[b][t] = sum_f frames[f][p - 512 f] / wss(p), p = t + 1024 (librosa.istft centre trim + fix_length(L_b)), over the
// row's frames f < F_b; t >= L_b -> 0
__global__ void audio_overlap_add_kernel(const float* __restrict__ T, int Fr, RowInfo info, const double* __restrict__ win2,
                                         float* __restrict__ out, int N) {
    const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    float v = 0.f;
    if (t < info.len(b)) {
        const int p = t + HALF, F = info.frames(b);
        const int f_lo = p >= NFFT ? (p - NFFT) / HOP + 1 : 0;
        const int f_hi = min(p / HOP, F - 1);
        double y = 0.0, w = 0.0;
        for (int f = f_lo; f <= f_hi; ++f) {
            const int n = p - f * HOP;
            y += (double)T[((long long)b * Fr + f) * NFFT + n];
            w += win2[n];
        }
        v = (float)(w > (double)FLT_MIN ? y / w : y);
    }
    out[(long long)b * N + t] = v;
}

// normalize_audio(x, max_val=1.) (audio_processing.py:50-62) over the row's own L_b samples: x - mean, / max|x| unless <= 1e-9.
// In double, rounded once (the reference normalises the float64 result of reduce_noise): a mean rounded to fp32 is off by up
// to 2^-25 |mean|, which the division by m = max|x - mean| turns into 2^-25 |mean| / m of full scale.
__global__ __launch_bounds__(1024) void audio_renormalize_kernel(float* __restrict__ x, int N, RowInfo info) {
    __shared__ double sh[16];
    const int b = blockIdx.x, L = info.len(b);
    float* r = x + (long long)b * N;
    double s = 0.0;
    for (int t = threadIdx.x; t < L; t += blockDim.x) s += r[t];
    const double mean = block_reduce(s, sh, OpAdd()) / L;
    double m = 0.0;
    for (int t = threadIdx.x; t < L; t += blockDim.x) m = fmax(m, fabs((double)r[t] - mean));
    m = block_reduce(m, sh, OpMax());
    const double sc = m > 1e-9 ? 1.0 / m : 1.0;
    for (int t = threadIdx.x; t < L; t += blockDim.x) r[t] = (float)(((double)r[t] - mean) * sc);
}

// conv[b][k] = sum_j x[k + j]^2 * w[W - 1 - j], k <= L_b - W (np.convolve 'valid' with L_b >= W; squares rounded to fp32
// like np.power on float32, products and sums in fp64).  256 threads x 4 consecutive outputs; the squared samples and the
// reversed window pass through LDS in chunks of TRIM_JC taps, one b128 operand read per 4 taps.
__global__ __launch_bounds__(256) void audio_trim_conv_kernel(const float* __restrict__ x, int N, RowInfo info,
                                                              const double* __restrict__ wrev, int W, int Wp,
                                                              double* __restrict__ conv, int Cst) {
    __shared__ __attribute__((aligned(16))) float xs[TRIM_OUT + TRIM_JC + 4];
    __shared__ double ws[TRIM_JC];
    const int b = blockIdx.y, L = info.len(b);
    if (L < W) return;
    const int nout = L - W + 1, k0 = blockIdx.x * TRIM_OUT;
    if (k0 >= nout) return;
    const float* r = x + (long long)b * N;
    const int t = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < Wp; j0 += TRIM_JC) {
        __syncthreads();
        for (int i = t; i < TRIM_OUT + TRIM_JC + 4; i += 256) {
            const long long s = (long long)k0 + j0 + i;
            const float v = s < L ? r[s] : 0.f;
            xs[i] = v * v;
        }
        for (int i = t; i < TRIM_JC; i += 256) ws[i] = j0 + i < Wp ? wrev[j0 + i] : 0.0;
        __syncthreads();
        const int jn = min(TRIM_JC, Wp - j0);             // multiple of 4
        f32x4 c = *(const f32x4*)&xs[4 * t];
        double cur[4] = {c[0], c[1], c[2], c[3]};
        for (int jj = 0; jj < jn; jj += 4) {
            const f32x4 q = *(const f32x4*)&xs[4 * t + jj + 4];
            const double nx[4] = {q[0], q[1], q[2], q[3]};
            const double v[4] = {ws[jj], ws[jj + 1], ws[jj + 2], ws[jj + 3]};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int i = o + u;
                    acc[o] = fma(i < 4 ? cur[i] : nx[i - 4], v[u], acc[o]);
                }
#pragma unroll
            for (int i = 0; i < 4; ++i) cur[i] = nx[i];
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int k = k0 + 4 * t + o;
        if (k < nout) conv[(long long)b * Cst + k] = acc[o];
    }
}

// rows shorter than the window: np.convolve swaps the operands, conv[k] = sum_m x[m]^2 w[k + L - 1 - m], k <= W - L
__global__ void audio_trim_conv_short_kernel(const float* __restrict__ x, int N, RowInfo info, const double* __restrict__ w,
                                             int W, double* __restrict__ conv, int Cst) {
    const int b = blockIdx.y, L = info.len(b);
    if (L >= W) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > W - L) return;
    const float* r = x + (long long)b * N;
    double s = 0.0;
    for (int m = 0; m < L; ++m) {
        const float v = r[m] * r[m];
        s = fma((double)v, w[k + L - 1 - m], s);
    }
    conv[(long long)b * Cst + k] = s;
}

struct TrimParams {
    int W;              // window taps (2 * (wl // 2))
    int wl;             // window_length (mean spans and margins)
    double threshold, add_start, add_end;
    int mode;           // 0 start_end, 1 start, 2 end
};

// thresholds and indices of trim_silence_window (audio_processing.py:340-370), one block per row
__global__ __launch_bounds__(1024) void audio_trim_bounds_kernel(const double* __restrict__ conv, int Cst, RowInfo info,
                                                                 TrimParams P, int* __restrict__ start, int* __restrict__ end) {
    __shared__ double sh[16];
    __shared__ int shi[16];
    const int b = blockIdx.x, L = info.len(b);
    const int nc = L >= P.W ? L - P.W + 1 : P.W - L + 1;
    const double* c = conv + (long long)b * Cst;
    const bool do_end = P.mode != 1, do_start = P.mode != 2;
    // np.mean(conv[-wl:]), np.mean(conv[:wl])
    const int e0 = max(0, nc - P.wl), s1 = min(P.wl, nc);
    double se = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        if (i >= e0) se += c[i];
        if (i < s1) ss += c[i];
    }
    se = block_reduce(se, sh, OpAdd());
    ss = block_reduce(ss, sh, OpAdd());
    const double th_end = fmin(P.threshold, fmax(se / (nc - e0) * 5.0, P.threshold / 50.0));
    const double th_start = fmin(P.threshold, fmax(ss / s1 * 5.0, P.threshold / 50.0));
    int last = -1, first = 0x7fffffff;
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        const double v = c[i];
        if (v > th_end) last = max(last, i);
        if (v > th_start) first = min(first, i);
    }
    last = block_reduce(last, shi, OpMax());
    first = block_reduce(first, shi, OpMin());
    if (threadIdx.x != 0) return;
    long long s = 0, e = L;
    if (do_end && last >= 0) e = std::min<long long>(L, (long long)last + (long long)((double)P.wl * P.add_end));
    if (do_start && first != 0x7fffffff) s = std::max<long long>(0, (long long)first - (long long)((double)P.wl * P.add_start));
    if (!(std::max<long long>(0, e - s) > L / 5)) {     // max_trim_factor 5: keep the whole row
        s = 0;
        e = L;
    }
    start[b] = (int)s;
    end[b] = (int)e;
}

// np.linspace(start, stop, num) element i (numpy: i * step + start, last element = stop)
double np_linspace(double a, double z, int num, int i) {
    if (num == 1) return a;
    if (i == num - 1) return z;
    const double step = (z - a) / (num - 1);
    const double y = (double)i * step;
    return y + a;
}

}  // namespace

void audioproc_free(tts_hip_engine* e) {
    AudioProcDev& a = e->aproc;
    for (void* p : a.allocs) (void)hipFree(p);
    a.allocs.clear();
    a.fwd_Bt = a.inv_Bt = nullptr;
    a.win2 = nullptr;
    a.ws.release();
    a.trim_win.release();
    a.trim_wl = -1;
}

namespace {

// DFT bases (built once, on first use, in fp64 with exact phase reduction): forward rows 0..1024 = cos * hann, 1025..2049 =
// -sin * hann, 2050..2079 = 0 ([NK][2048]); inverse [2048][NK] = the irfft terms (1/2048, x2 for bins 1..1023, imaginary
// parts of bins 0 and 1024 dropped) times the synthesis window; win2 = hann^2 (librosa window_sumsquare)
int audioproc_bases(tts_hip_engine* e) {
    AudioProcDev& a = e->aproc;
    if (a.fwd_Bt) return TTS_HIP_OK;
    std::vector<double> win(NFFT), c(NFFT), s(NFFT);
    for (int n = 0; n < NFFT; ++n) {
        win[n] = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / NFFT);     // scipy.signal.get_window('hann', 2048, fftbins=True)
        c[n] = std::cos(2.0 * M_PI * n / NFFT);
        s[n] = std::sin(2.0 * M_PI * n / NFFT);
    }
    std::vector<float> fwd((size_t)NK * NFFT, 0.f), inv((size_t)NFFT * NK, 0.f);
    for (int k = 0; k < NBIN; ++k) {
        const double ck = (k == 0 || k == NFFT / 2) ? 1.0 : 2.0;
        for (int n = 0; n < NFFT; ++n) {
            const int kn = (int)(((long long)k * n) % NFFT);          // exact phase reduction
            fwd[(size_t)k * NFFT + n] = (float)(c[kn] * win[n]);
            fwd[(size_t)(NBIN + k) * NFFT + n] = (float)(-s[kn] * win[n]);
            inv[(size_t)n * NK + k] = (float)(ck * c[kn] * win[n] / NFFT);
            if (k != 0 && k != NFFT / 2) inv[(size_t)n * NK + NBIN + k] = (float)(-ck * s[kn] * win[n] / NFFT);
        }
    }
    std::vector<double> w2(NFFT);
    for (int n = 0; n < NFFT; ++n) w2[n] = win[n] * win[n];
    float* p = nullptr;
    int rc = upload(e, fwd.data(), fwd.size(), &p, a.allocs);
    if (rc) return rc;
    a.fwd_Bt = p;
    rc = upload(e, inv.data(), inv.size(), &p, a.allocs);
    if (rc) return rc;
    a.inv_Bt = p;
    rc = upload(e, (const float*)w2.data(), w2.size() * 2, &p, a.allocs);
    if (rc) return rc;
    a.win2 = (double*)p;
    return TTS_HIP_OK;
}

// a DFT as one dense product: out[M][Nout] = A (rows lda apart, K wide) x Bt[Nout][K]^T
hipError_t dft_gemm(const float* A, long long lda, int K, const float* Bt, int Nout, int M, float* out, hipStream_t st) {
    return gemm_big(gemm_linear(A, lda, K, Bt, K, Nout, M, out), 1, st);
}

enum { RN_PADDED, RN_NOISE_PADDED, RN_SPECTRUM, RN_NOISE_SPECTRUM, RN_POWER_MAX, RN_THRESHOLD, RN_MASK, RN_GATED, RN_FRAMES,
       RN_STAGES };

// device pointers only; `lengths` / `noise_lens` already validated on the host.  stop (tts_hip_reduce_noise_probe): one of
// RN_* returns right after the launch that completes that stage with *stop_out describing what it wrote (the mask as fp32 in
// the not yet used frame buffer T; d_out is not touched); -1 runs everything.
int reduce_noise_run(tts_hip_engine* e, const float* d_audio, int B, int N, const std::vector<int>& lens,
                     const float* d_noise, int noise_len, int renorm, float* d_out, int stop = -1, StageView* stop_out = nullptr) {
    AudioProcDev& a = e->aproc;
    auto stop_at = [&](int stage, const void* p, size_t rows, size_t width, size_t pitch) {
        if (stop == stage && stop_out) *stop_out = StageView{p, rows, width, pitch};
        return stop == stage;
    };
    int rc = audioproc_bases(e);
    if (rc) return rc;
    const RnGeom g = rn_geom(B, N, noise_len);
    hipStream_t st = e->stream;
    HIPCHK(e, a.ws.ensure(g.total));
    char* base = (char*)a.ws.p;
    int* d_info = (int*)(base + g.off_info);
    unsigned* pmax = (unsigned*)(base + g.off_pmax);
    float* thr = (float*)(base + g.off_thr);
    float* P = (float*)(base + g.off_P);
    float* Q = (float*)(base + g.off_Q);
    float* S = (float*)(base + g.off_S);
    float* Sn = (float*)(base + g.off_Sn);
    float* T = (float*)(base + g.off_T);
    uint8_t* mask = (uint8_t*)(base + g.off_mask);
    // row facts: L_b, F_b, noise clip length, noise frames (the default clip is audio[b, :min(noise_len, L_b)])
    std::vector<int>& info_h = e->audio_info_h;
    info_h.assign((size_t)4 * B, 0);
    for (int b = 0; b < B; ++b) {
        const int L = lens[b], nl = d_noise ? noise_len : std::min(noise_len, L);
        info_h[b] = L;
        info_h[B + b] = 1 + (L + HOP) / HOP;
        info_h[2 * B + b] = nl;
        info_h[3 * B + b] = 1 + nl / HOP;
    }
    if (int rc = stage_row_info(e, d_info)) return rc;
    HIPCHK(e, hipMemsetAsync(pmax, 0, (size_t)2 * B * 4, st));
    const RowInfo info{d_info, B};
    {
        const long long n = (long long)B * g.NP + NFFT;
        hipLaunchKernelGGL(audio_pad_rows_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d_audio, (long long)N, d_info, P,
                           g.NP, B, n);
        HIPCHK(e, hipGetLastError());
        const long long nq = (long long)B * g.NQ + NFFT;
        hipLaunchKernelGGL(audio_pad_rows_kernel, dim3(blocks(nq, 256)), dim3(256), 0, st, d_noise ? d_noise : d_audio,
                           (long long)(d_noise ? noise_len : N), d_info + 2 * B, Q, g.NQ, B, nq);
        HIPCHK(e, hipGetLastError());
    }
    if (stop_at(RN_PADDED, P, B, g.NP, g.NP) || stop_at(RN_NOISE_PADDED, Q, B, g.NQ, g.NQ)) return TTS_HIP_OK;
    // forward DFTs: frame (b, f) is row b * Fr + f of the hop-strided view of the padded rows
    HIPCHK(e, dft_gemm(P, HOP, NFFT, a.fwd_Bt, NK, B * g.Fr, S, st));
    HIPCHK(e, dft_gemm(Q, HOP, NFFT, a.fwd_Bt, NK, B * g.Frn, Sn, st));
    if (stop_at(RN_SPECTRUM, S, (size_t)B * g.Fr, 2 * NBIN, NK) || stop_at(RN_NOISE_SPECTRUM, Sn, (size_t)B * g.Frn, 2 * NBIN, NK))
        return TTS_HIP_OK;
    hipLaunchKernelGGL(audio_power_max_kernel, dim3(64, B), dim3(256), 0, st, S, g.Fr, d_info + B, pmax);
    HIPCHK(e, hipGetLastError());
    hipLaunchKernelGGL(audio_power_max_kernel, dim3(8, B), dim3(256), 0, st, Sn, g.Frn, d_info + 3 * B, pmax + B);
    HIPCHK(e, hipGetLastError());
    if (stop_at(RN_POWER_MAX, pmax, 1, (size_t)2 * B, (size_t)2 * B)) return TTS_HIP_OK;
    hipLaunchKernelGGL(audio_noise_thresh_kernel, dim3(blocks(NBIN, 256), B), dim3(256), 0, st, Sn, g.Frn, info, pmax + B, thr);
    HIPCHK(e, hipGetLastError());
    if (stop_at(RN_THRESHOLD, thr, B, NBIN, NBIN)) return TTS_HIP_OK;
    hipLaunchKernelGGL(audio_gate_mask_kernel, dim3(blocks(NBIN, 256), g.Fr, B), dim3(256), 0, st, S, g.Fr, info, pmax, thr, mask);
    HIPCHK(e, hipGetLastError());
    if (stop == RN_MASK) {
        const long long n = (long long)B * g.Fr * NBIN;
        hipLaunchKernelGGL(audio_mask_f32_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, mask, T, n);
        HIPCHK(e, hipGetLastError());
        stop_at(RN_MASK, T, (size_t)B * g.Fr, NBIN, NBIN);
        return TTS_HIP_OK;
    }
    hipLaunchKernelGGL(audio_gate_apply_kernel, dim3(blocks(NBIN, 256), g.Fr, B), dim3(256), 0, st, S, g.Fr, info, mask);
    HIPCHK(e, hipGetLastError());
    if (stop_at(RN_GATED, S, (size_t)B * g.Fr, 2 * NBIN, NK)) return TTS_HIP_OK;
    HIPCHK(e, dft_gemm(S, NK, NK, a.inv_Bt, NFFT, B * g.Fr, T, st));
    if (stop_at(RN_FRAMES, T, (size_t)B * g.Fr, NFFT, NFFT)) return TTS_HIP_OK;
    hipLaunchKernelGGL(audio_overlap_add_kernel, dim3(blocks(N, 256), B), dim3(256), 0, st, T, g.Fr, info, a.win2, d_out, N);
    HIPCHK(e, hipGetLastError());
    if (renorm) {
        hipLaunchKernelGGL(audio_renormalize_kernel, dim3(B), dim3(1024), 0, st, d_out, N, info);
        HIPCHK(e, hipGetLastError());
    }
    return TTS_HIP_OK;
}

}  // namespace

int tts_hip_reduce_noise_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths,
                               const float* noise, int noise_len, int renormalize, float* out, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    std::vector<int> lens;
    char why[256];
    if (int rc = rn_check("reduce_noise_async", audio, B, N, lengths, noise_len, out, TTS_HIP_MEM_DEVICE, lens, why, sizeof why))
        return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    StreamScope scope(e, stream);
    return reduce_noise_run(e, audio, B, N, lens, noise, noise_len, renormalize, out);
}

namespace {

// tts_hip_reduce_noise (what = -1) and tts_hip_reduce_noise_probe (what = a stage, `out` takes that stage) are one call
int reduce_noise_sync(tts_hip_engine* e, const char* name, const float* audio, int B, int N, const int32_t* lengths,
                      const float* noise, int noise_len, int renormalize, int what, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    std::vector<int> lens;
    char why[256];
    if (int rc = rn_check(name, audio, B, N, lengths, noise_len, out, mem, lens, why, sizeof why)) return set_err(e, rc, "%s", why);
    if (what < -1 || what >= RN_STAGES) return set_err(e, TTS_HIP_EINVAL, "%s: no stage %d (0 .. %d)", name, what, RN_STAGES - 1);
    HIPCHK(e, hipSetDevice(e->device));
    const size_t n = (size_t)B * N;
    AudioStage io(e, mem);
    const int in = io.in(audio, n * 4), nz = io.in(noise, noise ? (size_t)B * noise_len * 4 : 0);
    // a probe never produces the ordinary result: `out` takes the stage straight from the workspace
    const int res = what >= 0 ? -1 : io.out(out, n * 4);
    if (int rc = io.begin()) return rc;
    if (what >= 0) {
        StageView s{};
        if (int rc = reduce_noise_run(e, io.ptr<const float>(in), B, N, lens, io.ptr<const float>(nz), noise_len, 0, nullptr, what, &s))
            return rc;
        if (int rc = copy_stage_out(e, s, out, mem)) return rc;
    } else if (int rc = reduce_noise_run(e, io.ptr<const float>(in), B, N, lens, io.ptr<const float>(nz), noise_len, renormalize,
                                         io.ptr<float>(res))) {
        return rc;
    }
    return io.finish();
}

}  // namespace

int tts_hip_reduce_noise(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const float* noise,
                         int noise_len, int renormalize, float* out, int mem) {
    return reduce_noise_sync(e, "reduce_noise", audio, B, N, lengths, noise, noise_len, renormalize, -1, out, mem);
}

// Test hook: reduce_noise_run on the same arguments up to stage `what`, then the stage's logical extent to `out`.
int tts_hip_reduce_noise_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const float* noise,
                               int noise_len, int what, float* out, int mem) {
    if (e && what < 0) return set_err(e, TTS_HIP_EINVAL, "reduce_noise_probe: no stage %d (0 .. %d)", what, RN_STAGES - 1);
    return reduce_noise_sync(e, "reduce_noise_probe", audio, B, N, lengths, noise, noise_len, 0, what, out, mem);
}

namespace {

// tts_hip_trim_silence (conv_out NULL) and tts_hip_trim_silence_probe (conv_out takes the convolution rows [B][max(N, W) + 1]
// in place of the thresholds and indices) are one call
int trim_silence_call(tts_hip_engine* e, const char* name, const float* audio, int B, int N, const int32_t* lengths,
                      int window_length, double threshold, double add_start, double add_end, int mode, int32_t* start,
                      int32_t* end, double* conv_out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    std::vector<int> lens;
    TrimGeom g{};
    char why[256];
    if (int rc = trim_check(name, audio, conv_out || (start && end), B, N, lengths, window_length, threshold, add_start, add_end,
                            mode, mem, lens, &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    const int h = window_length / 2, W = g.W, Wp = g.Wp, Cst = g.Cst;
    HIPCHK(e, hipSetDevice(e->device));
    AudioProcDev& a = e->aproc;
    hipStream_t st = e->stream;
    // window: concat(linspace(0, 1, h), linspace(1, 0, h)) / h, uploaded with its reversal (+ zero taps up to Wp)
    if (a.trim_wl != window_length) {
        std::vector<double> w(W), hw((size_t)W + Wp, 0.0);
        for (int i = 0; i < h; ++i) {
            w[i] = np_linspace(0.0, 1.0, h, i) / h;
            w[h + i] = np_linspace(1.0, 0.0, h, i) / h;
        }
        for (int i = 0; i < W; ++i) {
            hw[i] = w[i];
            hw[W + i] = w[W - 1 - i];
        }
        HIPCHK(e, a.trim_win.ensure(hw.size() * 8));
        HIPCHK(e, hipMemcpyAsync(a.trim_win.p, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipStreamSynchronize(st));
        a.trim_wl = window_length;
    }
    const double* d_w = (const double*)a.trim_win.p;
    Carve ws;
    const size_t off_conv = ws.take((size_t)B * Cst * 8), off_info = ws.take((size_t)B * 4);
    HIPCHK(e, a.ws.ensure(ws.o));
    double* conv = (double*)((char*)a.ws.p + off_conv);
    int* d_info = (int*)((char*)a.ws.p + off_info);
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4);
    const int s_out = io.out(conv_out ? nullptr : start, (size_t)B * 4), e_out = io.out(conv_out ? nullptr : end, (size_t)B * 4);
    if (int rc = io.begin()) return rc;
    const float* d_in = io.ptr<const float>(in);
    e->audio_info_h.assign(lens.begin(), lens.end());
    if (int rc = stage_row_info(e, d_info)) return rc;
    const RowInfo info{d_info, B};
    if (N >= W) {
        hipLaunchKernelGGL(audio_trim_conv_kernel, dim3(blocks(N - W + 1, TRIM_OUT), B), dim3(256), 0, st, d_in, N, info,
                           d_w + W, W, Wp, conv, Cst);
        HIPCHK(e, hipGetLastError());
    }
    if (g.min_len < W) {
        hipLaunchKernelGGL(audio_trim_conv_short_kernel, dim3(blocks(W - g.min_len + 1, 256), B), dim3(256), 0, st, d_in, N, info,
                           d_w, W, conv, Cst);
        HIPCHK(e, hipGetLastError());
    }
    if (conv_out) {
        HIPCHK(e, hipMemcpyAsync(conv_out, conv, (size_t)B * Cst * 8,
                                 mem == TTS_HIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
        return io.finish();
    }
    const TrimParams P{W, window_length, threshold, add_start, add_end, mode};
    hipLaunchKernelGGL(audio_trim_bounds_kernel, dim3(B), dim3(1024), 0, st, conv, Cst, info, P, io.ptr<int>(s_out),
                       io.ptr<int>(e_out));
    HIPCHK(e, hipGetLastError());
    return io.finish();
}

}  // namespace

int tts_hip_trim_silence(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int window_length,
                         double threshold, double add_start, double add_end, int mode, int32_t* start, int32_t* end, int mem) {
    return trim_silence_call(e, "trim_silence", audio, B, N, lengths, window_length, threshold, add_start, add_end, mode, start,
                             end, nullptr, mem);
}

// Test hook: the convolution launches of tts_hip_trim_silence on the same rows, then the rows they wrote to `conv`.
int tts_hip_trim_silence_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int window_length,
                               double* conv, int mem) {
    if (e && !conv) return set_err(e, TTS_HIP_EINVAL, "trim_silence_probe: bad argument");
    return trim_silence_call(e, "trim_silence_probe", audio, B, N, lengths, window_length, 0.1, 0.0, 0.0, 0, nullptr, nullptr,
                             conv, mem);
}
