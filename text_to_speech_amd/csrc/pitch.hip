// pitch.hip -- YIN pitch tracks of a ragged batch of recordings, and two F0 tracks compared along a warping path, on gfx950.
//
// The math is pinned in include/tts_hip.h (tts_hip_pitch, tts_hip_f0_error) and restated in float64 by tests/pitch_ref.py; the
// calls' checks and workspaces are csrc/pitch_call.h.
//   pitch_kernel     one workgroup per (frame, row).  The frame's W + tau_max samples lie in LDS (zeros outside the row).  A
//                    thread owns four consecutive lags 4 tid .. 4 tid + 3 and walks j four at a time: x[j .. j + 3] is one
//                    16-byte read at an address every lane shares (a broadcast), x[j + 4 tid + 4 .. + 7] one 16-byte read at
//                    lane stride 16 (conflict-free), the four values before it are kept from the step before -- 32 bytes of LDS
//                    for 16 terms of the difference (the reads are volatile LDS vector loads, or the optimizer splits them).
//                    Each d(tau) is one float32 chain over j in order.  S(tau): the thread's
//                    four lags in order on top of the exclusive block_scan of the threads' totals.  The pick is one
//                    block_reduce with OpMin over a key that puts every qualifying lag (by tau) before every other (by d',
//                    then tau); thread 0 walks down to the local minimum and interpolates in double.
//   f0_error_kernel  one workgroup per row: where the path ends (OpMin over the first pair out of range), then the counts and
//                    the double sums of c and c^2 through block_reduce.
// Nothing depends on the rows beside a row or on the batch size: a row alone gives the bits it gives in any batch.
#include "audio_dev.h"
#include "engine.h"
#include "pitch_call.h"

namespace {

constexpr int L = kPitchLagsPerThread;
constexpr int kFrameFloats = kPitchMaxWin + kPitchMaxLag + 8;      // the reads of the last owner's last step end 7 floats behind W + tau_max
constexpr int kMaxThreads = ((kPitchMaxLag + 1 + L - 1) / L + 63) / 64 * 64;      // 320
constexpr int kLagBits = 11;         // of the pick's key: a lag is at most 1024
static_assert(kPitchMaxLag < (1 << kLagBits), "a lag fits the key's low bits");
typedef float quad __attribute__((ext_vector_type(4)));      // one ds_read_b128
typedef __attribute__((address_space(3))) quad lds_quad;       // ... in LDS (a generic pointer would make it a flat load)
static_assert(L == 4, "the 16-byte reads of pitch_kernel are four lags wide");

struct PitchArgs {
    const float* audio;              // [B][N]
    const int* lens;                 // [B]
    float* out;                      // [3][B][F], or the probe's result
    int B, N, F, rate, hop, win, tau_min, tau_max;
    float threshold;
    int what;                        // -1 the call, else the probe's stage
};

// blockIdx.x = (row, frame)
__global__ __launch_bounds__(kMaxThreads) void pitch_kernel(PitchArgs g) {
    __shared__ __attribute__((aligned(16))) float x[kFrameFloats];
    __shared__ float dp[kMaxThreads * L];        // d'(tau) of every lag the threads own
    __shared__ float shf[16];
    __shared__ unsigned long long shk[16];
    const int t = blockIdx.x % g.F, b = blockIdx.x / g.F, tid = threadIdx.x;
    const int len = g.lens[b], Fb = 1 + len / g.hop, W = g.win, lags = g.tau_max + 1;
    const size_t BF = (size_t)g.B * g.F, bt = (size_t)b * g.F + t;
    if (t >= Fb) {                               // zeros at and behind F_b (uniform for the workgroup)
        if (g.what == TTS_HIP_PITCH_DIFF || g.what == TTS_HIP_PITCH_CMND) {
            for (int k = tid; k < lags; k += blockDim.x) g.out[bt * lags + k] = 0.f;
        } else if (tid < (g.what < 0 ? 3 : 2)) {
            g.out[tid * BF + bt] = 0.f;
        }
        return;
    }
    // the frame: x[i] = sample s + i of the row, 0 outside [0, len) and behind the W + tau_max samples a difference may touch
    const int s = t * g.hop - W / 2, used = W + g.tau_max, fill = (used + 8 + 3) & ~3;
    const float* row = g.audio + (size_t)b * g.N;
    for (int i = tid; i < fill && i < kFrameFloats; i += blockDim.x) {
        const int n = s + i;
        x[i] = i < used && n >= 0 && n < len ? row[n] : 0.f;
    }
    __syncthreads();

    const int tau0 = L * tid;
    float d[L] = {0.f, 0.f, 0.f, 0.f};
    if (tau0 < lags) {
        const int W4 = W & ~3;
        // volatile: the optimizer otherwise takes the 16-byte reads apart into the float pairs its packed instructions want,
        // ds_read2_b32 at lane stride 16 -- 4-way bank conflicts that cost more than the arithmetic
        quad lo = *(const volatile lds_quad*)(x + tau0);         // x[j + tau0 .. + 3]
        for (int j = 0; j < W4; j += 4) {
            const quad xj = *(const volatile lds_quad*)(x + j);  // the same address in every lane
            const quad hi = *(const volatile lds_quad*)(x + j + tau0 + 4);
            const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            const float xs[4] = {xj.x, xj.y, xj.z, xj.w};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const float df = xs[u] - w[u + l];
                    d[l] = fmaf(df, df, d[l]);
                }
            lo = hi;
        }
        for (int j = W4; j < W; ++j)                          // W is no multiple of four: the last one to three terms
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const float df = x[j] - x[j + tau0 + l];
                d[l] = fmaf(df, df, d[l]);
            }
    }
    if (g.what == TTS_HIP_PITCH_DIFF) {
#pragma unroll
        for (int l = 0; l < L; ++l)
            if (tau0 + l < lags) g.out[bt * lags + tau0 + l] = d[l];
        return;
    }

    // S(tau) = d(1) + ... + d(tau): lag 0 adds its exact zero; lags behind tau_max add nothing
    float p[L], run = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        run += tau0 + l < lags ? d[l] : 0.f;
        p[l] = run;
    }
    float total;
    // the exclusive prefix is the inclusive one of the thread before (not inclusive - run: that would round again)
    const float incl = block_scan(run, shf, total, OpAdd());
    dp[tid] = incl;
    __syncthreads();
    const float base = tid ? dp[tid - 1] : 0.f;
    __syncthreads();
    float q[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const int tau = tau0 + l;
        const float S = base + p[l];
        q[l] = tau == 0 || S == 0.f ? 1.f : d[l] * (float)tau / S;
        dp[tau] = q[l];
    }
    __syncthreads();
    if (g.what == TTS_HIP_PITCH_CMND) {
#pragma unroll
        for (int l = 0; l < L; ++l)
            if (tau0 + l < lags) g.out[bt * lags + tau0 + l] = q[l];
        return;
    }

    // the pick: a qualifying lag's key is its tau; any other lag's key lies above all of those and orders by d', then tau
    unsigned long long key = ~0ull;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const int tau = tau0 + l;
        if (tau < g.tau_min || tau > g.tau_max) continue;
        const unsigned long long k = q[l] < g.threshold ? (unsigned long long)tau
                                                        : ((1ull + __float_as_uint(q[l])) << kLagBits) | (unsigned)tau;
        key = k < key ? k : key;
    }
    key = block_reduce(key, shk, OpMin());
    if (tid == 0) {
        const bool voiced = key < (1ull << kLagBits);
        int tau = (int)(key & ((1ull << kLagBits) - 1));
        if (voiced)
            while (tau + 1 <= g.tau_max && dp[tau + 1] < dp[tau]) ++tau;
        if (g.what == TTS_HIP_PITCH_PICK) {
            g.out[bt] = voiced ? 1.f : 0.f;
            g.out[BF + bt] = (float)tau;
            return;
        }
        double delta = 0.0;
        if (tau - 1 >= 1 && tau + 1 <= g.tau_max) {
            const double a = dp[tau - 1], m = dp[tau], c = dp[tau + 1], den = a - 2.0 * m + c;
            if (den > 0.0) delta = (a - c) / (2.0 * den);
        }
        const double period = (double)tau + delta;
        g.out[bt] = voiced ? (float)((double)g.rate / period) : 0.f;
        g.out[BF + bt] = (float)period;
        g.out[2 * BF + bt] = dp[tau];
    }
}

struct F0Args {
    const float *a, *b;              // [B][Fa], [B][Fb]
    const int* lens;                 // [2][B]
    const int32_t* path;             // [B][P][2] or null
    float* stats;                    // [6][B]
    int B, Fa, Fb, P;
    float gross;
};

// blockIdx.x = row
__global__ __launch_bounds__(256) void f0_error_kernel(F0Args g) {
    __shared__ double shd[16];
    __shared__ int shi[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int la = g.lens[b], lb = g.lens[g.B + b];
    const int32_t* path = g.path ? g.path + (size_t)b * g.P * 2 : nullptr;
    int n = la < lb ? la : lb;                   // the diagonal
    if (path) {                                  // the path ends at its first pair out of range
        int bad = g.P;
        for (int k = tid; k < g.P; k += 256) {
            const int i = path[2 * k], j = path[2 * k + 1];
            if (i < 0 || i >= la || j < 0 || j >= lb) {
                bad = k;
                break;
            }
        }
        n = block_reduce(bad, shi, OpMin());
    }
    const float* fa = g.a + (size_t)b * g.Fa;
    const float* fb = g.b + (size_t)b * g.Fb;
    int both = 0, one = 0, gross = 0;
    double sum = 0.0, sq = 0.0;
    for (int k = tid; k < n; k += 256) {
        const int i = path ? path[2 * k] : k, j = path ? path[2 * k + 1] : k;
        const float va = fa[i], vb = fb[j];
        const bool ua = va > 0.f, ub = vb > 0.f;
        if (ua && ub) {
            const double c = 1200.0 * log2((double)va / (double)vb);
            ++both;
            sum += c;
            sq += c * c;
            if (fabs(c) > (double)g.gross) ++gross;
        } else if (ua != ub) {
            ++one;
        }
    }
    both = block_reduce(both, shi, OpAdd());
    one = block_reduce(one, shi, OpAdd());
    gross = block_reduce(gross, shi, OpAdd());
    sum = block_reduce(sum, shd, OpAdd());
    sq = block_reduce(sq, shd, OpAdd());
    if (tid == 0) {
        const size_t B = (size_t)g.B;
        g.stats[b] = (float)n;
        g.stats[B + b] = (float)both;
        g.stats[2 * B + b] = both ? (float)sqrt(sq / (double)both) : 0.f;
        g.stats[3 * B + b] = both ? (float)(sum / (double)both) : 0.f;
        g.stats[4 * B + b] = (float)one;
        g.stats[5 * B + b] = (float)gross;
    }
}

// (The request already passed pitch_check.)  Enqueued on e->stream, which is drained before returning.
int pitch_impl(tts_hip_engine* e, const PitchCall& c) {
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const PitchLayout l = pitch_layout(c);
    HIPCHK(e, e->pitch.ws.ensure(l.bytes));
    char* ws = (char*)e->pitch.ws.p;
    const bool host = c.mem == TTS_HIP_MEM_HOST;

    std::vector<int32_t>& lens = e->pitch.lens_h;
    lens.resize((size_t)c.B);
    for (int b = 0; b < c.B; ++b) lens[b] = c.lengths ? c.lengths[b] : c.N;
    HIPCHK(e, hipMemcpyAsync(ws + l.lens, lens.data(), (size_t)c.B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (host) HIPCHK(e, hipMemcpyAsync(ws + l.in, c.audio, (size_t)c.B * c.N * sizeof(float), hipMemcpyHostToDevice, st));

    PitchArgs g{};
    g.audio = host ? (const float*)(ws + l.in) : c.audio;
    g.lens = (const int*)(ws + l.lens);
    g.out = host ? (float*)(ws + l.out) : c.out;
    g.B = c.B, g.N = c.N, g.F = l.F, g.rate = c.rate, g.hop = c.hop, g.win = c.win, g.tau_min = c.tau_min, g.tau_max = c.tau_max;
    g.threshold = c.threshold;
    g.what = c.probe ? c.what : -1;
    timing_begin(e, 0);
    // B * F floats of `out` passed the byte limit: the grid stays below 2^29 workgroups
    hipLaunchKernelGGL(pitch_kernel, dim3((unsigned)((size_t)c.B * l.F)), dim3((unsigned)l.threads), 0, st, g);
    timing_end(e);
    HIPCHK(e, hipGetLastError());
    if (host) HIPCHK(e, hipMemcpyAsync(c.out, g.out, l.out_elems * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return TTS_HIP_OK;
}

int pitch_entry(tts_hip_engine* e, const PitchCall& c) {
    if (!e) return TTS_HIP_EINVAL;
    char why[256] = "";
    if (const int rc = pitch_check(c, why, sizeof why)) return set_err(e, rc, "%s", why);
    StreamScope scope(e, c.stream);
    return pitch_impl(e, c);
}

// (The request already passed f0_error_check.)
int f0_error_impl(tts_hip_engine* e, const F0ErrorCall& c) {
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const F0ErrorLayout l = f0_error_layout(c);
    HIPCHK(e, e->pitch.ws.ensure(l.bytes));
    char* ws = (char*)e->pitch.ws.p;
    const bool host = c.mem == TTS_HIP_MEM_HOST;
    const size_t B = (size_t)c.B;

    std::vector<int32_t>& lens = e->pitch.lens_h;
    lens.resize(2 * B);
    for (int b = 0; b < c.B; ++b) lens[b] = c.len_a ? c.len_a[b] : c.Fa, lens[B + b] = c.len_b ? c.len_b[b] : c.Fb;
    HIPCHK(e, hipMemcpyAsync(ws + l.lens, lens.data(), 2 * B * sizeof(int32_t), hipMemcpyHostToDevice, st));

    F0Args g{};
    g.a = c.f0_a, g.b = c.f0_b, g.path = c.path, g.stats = c.stats;
    if (host) {
        HIPCHK(e, hipMemcpyAsync(ws + l.in_a, c.f0_a, B * c.Fa * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(ws + l.in_b, c.f0_b, B * c.Fb * sizeof(float), hipMemcpyHostToDevice, st));
        g.a = (const float*)(ws + l.in_a), g.b = (const float*)(ws + l.in_b), g.stats = (float*)(ws + l.stats);
        if (c.path) {
            HIPCHK(e, hipMemcpyAsync(ws + l.path, c.path, B * c.P * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
            g.path = (const int32_t*)(ws + l.path);
        }
    }
    g.lens = (const int*)(ws + l.lens);
    g.B = c.B, g.Fa = c.Fa, g.Fb = c.Fb, g.P = c.P, g.gross = c.gross_cents;
    timing_begin(e, 1);
    hipLaunchKernelGGL(f0_error_kernel, dim3((unsigned)B), dim3(256), 0, st, g);      // B <= 2^18 (B * (Fa + Fb) <= 2^19)
    timing_end(e);
    HIPCHK(e, hipGetLastError());
    if (host) HIPCHK(e, hipMemcpyAsync(c.stats, g.stats, kF0Stats * B * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return TTS_HIP_OK;
}

}  // namespace

void pitch_free(tts_hip_engine* e) { e->pitch.ws.release(); }

extern "C" int tts_hip_pitch(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop, int win,
                             int tau_min, int tau_max, float threshold, float* out, int mem, void* stream) {
    return pitch_entry(e, PitchCall{"pitch", audio, B, N, lengths, rate, hop, win, tau_min, tau_max, threshold, false, -1, out, mem, stream});
}

extern "C" int tts_hip_pitch_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop,
                                   int win, int tau_min, int tau_max, float threshold, int what, float* out, int mem, void* stream) {
    return pitch_entry(e, PitchCall{"pitch_probe", audio, B, N, lengths, rate, hop, win, tau_min, tau_max, threshold, true, what, out, mem,
                                    stream});
}

extern "C" int tts_hip_f0_error(tts_hip_engine* e, const float* f0_a, const float* f0_b, int B, int Fa, int Fb, const int32_t* len_a,
                                const int32_t* len_b, const int32_t* path, int P, float gross_cents, float* stats, int mem,
                                void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    const F0ErrorCall c{"f0_error", f0_a, f0_b, B, Fa, Fb, len_a, len_b, path, P, gross_cents, stats, mem, stream};
    char why[256] = "";
    if (const int rc = f0_error_check(c, why, sizeof why)) return set_err(e, rc, "%s", why);
    StreamScope scope(e, c.stream);
    return f0_error_impl(e, c);
}
