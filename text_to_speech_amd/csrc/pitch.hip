// pitch.hip -- YIN and probabilistic-YIN pitch tracks of a ragged batch of recordings, and two F0 tracks compared along a warping
// path, on gfx950.
//
// The math is pinned in include/tts_hip.h (tts_hip_pitch, tts_hip_pyin, tts_hip_f0_error) and restated in float64 by
// tests/pitch_ref.py and tests/pyin_ref.py; the calls' checks and workspaces are csrc/pitch_call.h.  The frame stages (frame_load,
// frame_difference, frame_cmnd, parabolic_delta) are device functions that pitch_kernel and pyin_obs_kernel share.
//   pitch_kernel     one workgroup per (frame, row).  The frame's W + tau_max samples lie in LDS (zeros outside the row).  A
//                    thread owns four consecutive lags 4 tid .. 4 tid + 3 and walks j four at a time: x[j .. j + 3] is one
//                    16-byte read at an address every lane shares (a broadcast), x[j + 4 tid + 4 .. + 7] one 16-byte read at
//                    lane stride 16 (conflict-free), the four values before it are kept from the step before -- 32 bytes of LDS
//                    for 16 terms of the difference (the reads are volatile LDS vector loads, or the optimizer splits them).
//                    Each d(tau) is one float32 chain over j in order.  S(tau): the thread's
//                    four lags in order on top of the exclusive block_scan of the threads' totals.  The pick is one
//                    block_reduce with OpMin over a key that puts every qualifying lag (by tau) before every other (by d',
//                    then tau); thread 0 walks down to the local minimum and interpolates in double.
//   pyin_obs_kernel  one workgroup per (frame, row), d' as above.  Trough flags from the neighbours, the smallest trough d' before
//                    each lag by block_scan (OpMin), p from the cumulative prior in LDS, the least trough by the keyed
//                    block_reduce; the troughs compacted in lag order, and the first trough of each bin sums the bin (bins fall
//                    as lags rise): obs, cand, v.  No atomics.
//   pyin_viterbi_kernel  one workgroup per row, a thread per bin (its voiced and its unvoiced state): the log-domain recursion
//                    over double-buffered, padded scores in LDS, the frame's maximum subtracted every frame, uint16
//                    backpointers in the workspace; one lane follows them back, all threads write the planes.
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

// The frame (t, b) into x: x[i] = sample s + i of the row, 0 outside [0, len) and behind the W + tau_max samples a difference may
// touch.  Ends on a barrier.
__device__ __forceinline__ void frame_load(const PitchArgs& g, int b, int t, int len, float* x) {
    const int tid = threadIdx.x, W = g.win;
    const int s = t * g.hop - W / 2, used = W + g.tau_max, fill = (used + 8 + 3) & ~3;
    const float* row = g.audio + (size_t)b * g.N;
    for (int i = tid; i < fill && i < kFrameFloats; i += blockDim.x) {
        const int n = s + i;
        x[i] = i < used && n >= 0 && n < len ? row[n] : 0.f;
    }
    __syncthreads();
}

// d of the thread's four lags 4 tid .. 4 tid + 3 from the frame in x, added to the zeros in d: one float32 chain over j in order each
__device__ __forceinline__ void frame_difference(const PitchArgs& g, const float* x, float (&d)[L]) {
    const int tid = threadIdx.x, W = g.win, lags = g.tau_max + 1;
    const int tau0 = L * tid;
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
}

// d' of the thread's four lags into q and into dp[tau] (every lag the threads own).  Ends on a barrier.
__device__ __forceinline__ void frame_cmnd(const PitchArgs& g, const float (&d)[L], float* dp, float* shf, float (&q)[L]) {
    const int tid = threadIdx.x, lags = g.tau_max + 1, tau0 = L * tid;
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
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const int tau = tau0 + l;
        const float S = base + p[l];
        q[l] = tau == 0 || S == 0.f ? 1.f : d[l] * (float)tau / S;
        dp[tau] = q[l];
    }
    __syncthreads();
}

// a, m, c = d'(tau - 1), d'(tau), d'(tau + 1): the parabola's vertex relative to tau, 0 where a neighbour is outside [1, tau_max]
__device__ __forceinline__ double parabolic_delta(const float* dp, int tau, int tau_max) {
    double delta = 0.0;
    if (tau - 1 >= 1 && tau + 1 <= tau_max) {
        const double a = dp[tau - 1], m = dp[tau], c = dp[tau + 1], den = a - 2.0 * m + c;
        if (den > 0.0) delta = (a - c) / (2.0 * den);
    }
    return delta;
}

// blockIdx.x = (row, frame)
__global__ __launch_bounds__(kMaxThreads) void pitch_kernel(PitchArgs g) {
    __shared__ __attribute__((aligned(16))) float x[kFrameFloats];
    __shared__ float dp[kMaxThreads * L];        // d'(tau) of every lag the threads own
    __shared__ float shf[16];
    __shared__ unsigned long long shk[16];
    const int t = blockIdx.x % g.F, b = blockIdx.x / g.F, tid = threadIdx.x;
    const int len = g.lens[b], Fb = 1 + len / g.hop, lags = g.tau_max + 1;
    const size_t BF = (size_t)g.B * g.F, bt = (size_t)b * g.F + t;
    if (t >= Fb) {                               // zeros at and behind F_b (uniform for the workgroup)
        if (g.what == TTS_HIP_PITCH_DIFF || g.what == TTS_HIP_PITCH_CMND) {
            for (int k = tid; k < lags; k += blockDim.x) g.out[bt * lags + k] = 0.f;
        } else if (tid < (g.what < 0 ? 3 : 2)) {
            g.out[tid * BF + bt] = 0.f;
        }
        return;
    }
    frame_load(g, b, t, len, x);
    const int tau0 = L * tid;
    float d[L] = {0.f, 0.f, 0.f, 0.f};
    frame_difference(g, x, d);
    if (g.what == TTS_HIP_PITCH_DIFF) {
#pragma unroll
        for (int l = 0; l < L; ++l)
            if (tau0 + l < lags) g.out[bt * lags + tau0 + l] = d[l];
        return;
    }
    float q[L];
    frame_cmnd(g, d, dp, shf, q);
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
        const double period = (double)tau + parabolic_delta(dp, tau, g.tau_max);
        g.out[bt] = voiced ? (float)((double)g.rate / period) : 0.f;
        g.out[BF + bt] = (float)period;
        g.out[2 * BF + bt] = dp[tau];
    }
}

// ---- probabilistic YIN
constexpr int kMaxTroughs = kPitchMaxLag / 2 + 8;      // troughs lie at least two lags apart
static_assert(2 * kPyinMaxBins <= kFrameFloats, "obs and cand of a frame lie where its samples lay");
static_assert(2 * kPyinMaxBins <= 65536, "a state fits a uint16 backpointer");

struct OpMaxF {                      // the maximum of scores of either sign
    template <class T> __device__ static T id() { return std::numeric_limits<T>::lowest(); }
    template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

struct PyinArgs {
    PitchArgs p;                     // the frame grid; p.out is unused
    const float* cum;                // [n_thresh + 1]
    const float* tables;             // log triangle [max_step + 1], log norm [n_bins], log(1 - switch), log(switch)
    float *obs, *cand;               // [B][F][n_bins]
    float* vprob;                    // [B][F]
    uint16_t* back;                  // [B][F][2 n_bins]
    int32_t* path;                   // [B][F]
    float* out;                      // [3][B][F], or the probe's result
    double fmin;
    int n_thresh, n_bins, bps, max_step;
    float no_trough;
    int what;                        // -1 the call, else the probe's stage
};

// how many of the thresholds s_i = float32(i) / float32(n), i = 1 .. n, are <= v: an estimate, put right by the comparisons the
// rule is stated in (a NaN ends both loops)
__device__ __forceinline__ int thresholds_at_most(float v, int n) {
    const float fn = (float)n;
    int k = (int)fminf(fmaxf(v * fn, 0.f), fn);
    while (k < n && __fdiv_rn((float)(k + 1), fn) <= v) ++k;
    while (k > 0 && __fdiv_rn((float)k, fn) > v) --k;
    return k;
}

// blockIdx.x = (row, frame).  The troughs of d', their probabilities and bins; obs, cand and v of the frame.
__global__ __launch_bounds__(kMaxThreads) void pyin_obs_kernel(PyinArgs a) {
    __shared__ __attribute__((aligned(16))) float x[kFrameFloats];      // the samples; then scratch; then obs | cand
    __shared__ float dp[kMaxThreads * L];
    __shared__ float cum[kPyinMaxThresh + 1];
    __shared__ float tp[kMaxTroughs], tper[kMaxTroughs];                // the troughs by ascending lag: p, period
    __shared__ int tbin[kMaxTroughs];                                   // ... and bin
    __shared__ float shf[16];
    __shared__ unsigned long long shk[16];
    __shared__ int shi[16];
    const PitchArgs& g = a.p;
    const int t = blockIdx.x % g.F, b = blockIdx.x / g.F, tid = threadIdx.x, nb = a.n_bins;
    const int len = g.lens[b], Fb = 1 + len / g.hop, lags = g.tau_max + 1;
    const size_t BF = (size_t)g.B * g.F, bt = (size_t)b * g.F + t;
    if (t >= Fb) {                               // the probes: zeros at and behind F_b; the decode reads none of these frames
        if (a.what == TTS_HIP_PYIN_TROUGH)
            for (int k = tid; k < lags; k += blockDim.x) a.out[bt * lags + k] = 0.f;
        if (a.what == TTS_HIP_PYIN_OBS)
            for (int k = tid; k < nb; k += blockDim.x) a.out[bt * nb + k] = a.out[(BF + bt) * nb + k] = 0.f;
        return;
    }
    for (int k = tid; k <= a.n_thresh; k += blockDim.x) cum[k] = a.cum[k];
    frame_load(g, b, t, len, x);
    const int tau0 = L * tid;
    float d[L] = {0.f, 0.f, 0.f, 0.f}, q[L];
    frame_difference(g, x, d);
    frame_cmnd(g, d, dp, shf, q);                // its barriers are behind every read of x: x is free

    // troughs, and the smallest d' of the troughs before each lag
    bool tr[L];
    float before[L], run = OpMin::id<float>();
    int mine = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const int tau = tau0 + l;
        tr[l] = tau >= g.tau_min && tau <= g.tau_max && q[l] < dp[tau - 1] && (tau == g.tau_max || q[l] <= dp[tau + 1]);
        before[l] = run;
        if (tr[l]) run = q[l] < run ? q[l] : run, ++mine;
    }
    float all;
    const float incl = block_scan(run, shf, all, OpMin());
    x[tid] = incl;
    __syncthreads();
    const float base = tid ? x[tid - 1] : OpMin::id<float>();
    __syncthreads();
    // the trough of smallest d', the smallest lag on ties (d' >= 0: its bits order as it does)
    unsigned long long key = ~0ull;
#pragma unroll
    for (int l = 0; l < L; ++l)
        if (tr[l]) {
            const unsigned long long k = ((unsigned long long)__float_as_uint(q[l]) << kLagBits) | (unsigned)(tau0 + l);
            key = k < key ? k : key;
        }
    key = block_reduce(key, shk, OpMin());
    const int tau_least = key == ~0ull ? -1 : (int)(key & ((1ull << kLagBits) - 1));
    float p[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        p[l] = 0.f;
        if (!tr[l]) continue;
        const float m = base < before[l] ? base : before[l];
        const int lo = thresholds_at_most(q[l], a.n_thresh);
        if (q[l] < m) p[l] = cum[thresholds_at_most(m, a.n_thresh)] - cum[lo];
        if (tau0 + l == tau_least) p[l] = __fadd_rn(p[l], __fmul_rn(a.no_trough, cum[lo]));
    }
    if (a.what == TTS_HIP_PYIN_TROUGH) {
#pragma unroll
        for (int l = 0; l < L; ++l)
            if (tau0 + l < lags) a.out[bt * lags + tau0 + l] = p[l];
        return;
    }

    // the troughs side by side, in the order of their lags: a thread's follow those of the threads before it
    int troughs;
    int k = block_scan(mine, shi, troughs, OpAdd()) - mine;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        if (!tr[l] || k >= kMaxTroughs) continue;
        const int tau = tau0 + l;
        const double period = (double)tau + parabolic_delta(dp, tau, g.tau_max);
        const double pos = 12.0 * a.bps * log2((double)g.rate / period / a.fmin), r = floor(pos + 0.5);
        tp[k] = p[l];
        tper[k] = (float)period;
        tbin[k] = !(r >= 0.0) ? 0 : r > (double)(nb - 1) ? nb - 1 : (int)r;
        ++k;
    }
    troughs = troughs < kMaxTroughs ? troughs : kMaxTroughs;
    float *obs = x, *cand = x + kPyinMaxBins;
    for (int j = tid; j < nb; j += blockDim.x) obs[j] = cand[j] = 0.f;
    __syncthreads();
    // periods grow with the lag (troughs two lags apart, |delta| <= 1/2), so bins fall: a bin's troughs are neighbours, and the
    // first of them sums the bin by ascending lag
    for (int h = tid; h < troughs; h += blockDim.x) {
        const int bin = tbin[h];
        if (h && tbin[h - 1] == bin) continue;
        float sum = tp[h], best = tp[h], per = tper[h];
        for (int n = h + 1; n < troughs && tbin[n] == bin; ++n) {
            sum = __fadd_rn(sum, tp[n]);
            if (tp[n] > best) best = tp[n], per = tper[n];
        }
        obs[bin] = sum;
        cand[bin] = per;
    }
    __syncthreads();
    float part = 0.f;
    for (int j = tid; j < nb; j += blockDim.x) {
        a.obs[bt * nb + j] = obs[j];
        a.cand[bt * nb + j] = cand[j];
        if (a.what == TTS_HIP_PYIN_OBS) a.out[bt * nb + j] = obs[j], a.out[(BF + bt) * nb + j] = cand[j];
        part = __fadd_rn(part, obs[j]);
    }
    part = block_reduce(part, shf, OpAdd());
    if (tid == 0) a.vprob[bt] = fminf(part, 1.f);
}

// blockIdx.x = row; thread j owns bin j: its voiced state j and its unvoiced state n_bins + j.  The scores of the frame before
// lie in LDS with log norm(i) already taken off, double-buffered and padded by max_step bins; a frame costs two windowed maxima
// (the offset k is the same in every lane: the triangle is a broadcast read), the choice between them,
// the frame's maximum through block_reduce and one barrier more.  One lane follows the predecessors back (the compromise of
// mel_dtw's path), then every thread writes frames of the result.
__global__ __launch_bounds__(kPyinMaxBins) void pyin_viterbi_kernel(PyinArgs a) {
    __shared__ float sv[2][3 * kPyinMaxBins], su[2][3 * kPyinMaxBins];      // bin i at [max_step + i]; the lowest float on either side
    __shared__ float ltri[kPyinMaxBins + 1];
    __shared__ float shf[16];
    __shared__ int shi[16];
    const PitchArgs& g = a.p;
    const int b = blockIdx.x, j = threadIdx.x, nb = a.n_bins, ms = a.max_step, S = 2 * nb;
    const int len = g.lens[b], Fb = 1 + len / g.hop, F = g.F;
    const size_t BF = (size_t)g.B * F, row = (size_t)b * F;
    const bool own = j < nb;
    for (int k = j; k <= ms; k += blockDim.x) ltri[k] = a.tables[k];
    for (int k = j; k < nb + 2 * ms; k += blockDim.x)            // max_step bins of padding: a window needs no bounds, and lowest + w = lowest
        sv[0][k] = sv[1][k] = su[0][k] = su[1][k] = OpMaxF::id<float>();
    const float lnorm = own ? a.tables[ms + 1 + j] : 0.f, lkeep = a.tables[ms + 1 + nb], lswitch = a.tables[ms + 2 + nb];
    const float tiny = 0x1p-100f;
    __syncthreads();
    float dv = 0.f, du = 0.f;
    float obs_next = own ? a.obs[row * nb + j] : 0.f, v_next = a.vprob[row];      // a frame ahead: the loads are off the recursion's path
    for (int t = 0; t < Fb; ++t) {
        const size_t bt = row + t;
        int bv = j, bu = nb + j;                 // frame 0 has no predecessor: the state itself
        const float obs_t = obs_next, v_t = v_next;
        if (t + 1 < Fb) {
            if (own) obs_next = a.obs[(bt + 1) * nb + j];
            v_next = a.vprob[bt + 1];
        }
        if (own) {
            const float ov = logf(fmaxf(obs_t, tiny));
            const float ou = logf(fmaxf(__fdiv_rn(1.f - v_t, (float)nb), tiny));
            if (t > 0) {
                const float *pv = sv[(t - 1) & 1] + ms + j, *pu = su[(t - 1) & 1] + ms + j;      // [k]: bin j + k
                float mv = OpMaxF::id<float>(), mu = mv;
                int kv = 0, ku = 0;
#pragma unroll 4
                for (int k = -ms; k <= ms; ++k) {                // ascending, strictly greater: ties stay with the smallest index;
                    const float w = ltri[k < 0 ? -k : k];        // the padding never is (and k = 0 is a bin)
                    const float cv = pv[k] + w, cu = pu[k] + w;
                    if (cv > mv) mv = cv, kv = k;
                    if (cu > mu) mu = cu, ku = k;
                }
                const int iv = j + kv, iu = j + ku;
                // a voiced predecessor has the smaller index: it keeps a tie
                const float vv = mv + lkeep, uv = mu + lswitch, vu = mv + lswitch, uu = mu + lkeep;
                dv = ov + (uv > vv ? uv : vv), bv = uv > vv ? nb + iu : iv;
                du = ou + (uu > vu ? uu : vu), bu = uu > vu ? nb + iu : iv;
            } else {
                dv = ov, du = ou;
            }
        }
        const float top = block_reduce(own ? (dv > du ? dv : du) : OpMaxF::id<float>(), shf, OpMaxF());
        if (own) {
            dv -= top, du -= top;
            sv[t & 1][ms + j] = dv - lnorm;
            su[t & 1][ms + j] = du - lnorm;
            a.back[bt * S + j] = (uint16_t)bv;
            a.back[bt * S + nb + j] = (uint16_t)bu;
            if (a.what == TTS_HIP_PYIN_DELTA) a.out[bt * S + j] = dv, a.out[bt * S + nb + j] = du;
            if (a.what == TTS_HIP_PYIN_BACK) a.out[bt * S + j] = (float)bv, a.out[bt * S + nb + j] = (float)bu;
        }
        __syncthreads();
    }
    if (a.what == TTS_HIP_PYIN_DELTA || a.what == TTS_HIP_PYIN_BACK) {       // zeros at and behind F_b
        for (size_t k = (size_t)Fb * S + j; k < (size_t)F * S; k += blockDim.x) a.out[row * S + k] = 0.f;
        return;
    }
    // the last state: the frame's maximum became an exact 0, the smallest such state (none if a NaN came in: state 0)
    int last = own ? (dv == 0.f ? j : du == 0.f ? nb + j : S) : S;
    last = block_reduce(last, shi, OpMin());     // its barriers: every backpointer of the row is written
    if (j == 0) {
        int s = last < S ? last : 0;
        for (int t = Fb - 1; t >= 0; --t) {
            a.path[row + t] = s;
            s = a.back[(row + t) * S + s];       // a state below 2 n_bins, whatever came in
        }
    }
    __syncthreads();
    for (int t = j; t < F; t += blockDim.x) {
        const size_t bt = row + t;
        if (t >= Fb) {
            a.out[bt] = 0.f;
            if (a.what < 0) a.out[BF + bt] = a.out[2 * BF + bt] = 0.f;
            continue;
        }
        const int s = a.path[bt], bin = s >= nb ? s - nb : s;
        if (a.what == TTS_HIP_PYIN_PATH) {
            a.out[bt] = (float)s;
            continue;
        }
        const float c = a.cand[bt * nb + bin];
        const double pitch = c > 0.f ? (double)g.rate / (double)c : a.fmin * exp2((double)bin / (12.0 * a.bps));
        a.out[bt] = s < nb ? (float)pitch : 0.f;
        a.out[BF + bt] = (float)pitch;
        a.out[2 * BF + bt] = a.vprob[bt];
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

// (The request already passed pyin_check.)  The observation kernel, then -- unless the probe asks for a stage of the first -- the
// decode, both on e->stream, which is drained before returning.
int pyin_impl(tts_hip_engine* e, const PyinCall& c) {
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const PitchCall& pc = c.p;
    const PyinLayout l = pyin_layout(c);
    HIPCHK(e, e->pitch.ws.ensure(l.bytes));
    char* ws = (char*)e->pitch.ws.p;
    const bool host = pc.mem == TTS_HIP_MEM_HOST;

    std::vector<int32_t>& lens = e->pitch.lens_h;
    lens.resize((size_t)pc.B);
    for (int b = 0; b < pc.B; ++b) lens[b] = pc.lengths ? pc.lengths[b] : pc.N;
    std::vector<float>& tab = e->pitch.tables_h;
    const size_t n_cum = (size_t)c.n_thresh + 1, n_tab = (size_t)c.max_step + 1 + c.n_bins + 2;
    tab.resize(n_cum + n_tab);
    pyin_tables(c, tab.data(), tab.data() + n_cum);
    HIPCHK(e, hipMemcpyAsync(ws + l.lens, lens.data(), (size_t)pc.B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(ws + l.cum, tab.data(), n_cum * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(ws + l.tables, tab.data() + n_cum, n_tab * sizeof(float), hipMemcpyHostToDevice, st));
    if (host) HIPCHK(e, hipMemcpyAsync(ws + l.in, pc.audio, (size_t)pc.B * pc.N * sizeof(float), hipMemcpyHostToDevice, st));

    PyinArgs a{};
    PitchArgs& g = a.p;
    g.audio = host ? (const float*)(ws + l.in) : pc.audio;
    g.lens = (const int*)(ws + l.lens);
    g.B = pc.B, g.N = pc.N, g.F = l.F, g.rate = pc.rate, g.hop = pc.hop, g.win = pc.win, g.tau_min = pc.tau_min, g.tau_max = pc.tau_max;
    g.what = -1;
    a.cum = (const float*)(ws + l.cum), a.tables = (const float*)(ws + l.tables);
    a.obs = (float*)(ws + l.obs), a.cand = (float*)(ws + l.cand), a.vprob = (float*)(ws + l.vprob);
    a.back = (uint16_t*)(ws + l.back), a.path = (int32_t*)(ws + l.path);
    a.out = host ? (float*)(ws + l.out) : pc.out;
    a.fmin = c.fmin, a.n_thresh = c.n_thresh, a.n_bins = c.n_bins, a.bps = c.bps, a.max_step = c.max_step, a.no_trough = c.no_trough_prob;
    a.what = c.probe ? c.what : -1;
    timing_begin(e, 2);
    // B * F floats of `out` passed the byte limit: the grid stays below 2^29 workgroups
    hipLaunchKernelGGL(pyin_obs_kernel, dim3((unsigned)((size_t)pc.B * l.F)), dim3((unsigned)l.threads), 0, st, a);
    timing_end(e);
    HIPCHK(e, hipGetLastError());
    if (a.what != TTS_HIP_PYIN_TROUGH && a.what != TTS_HIP_PYIN_OBS) {
        timing_begin(e, 3);
        hipLaunchKernelGGL(pyin_viterbi_kernel, dim3((unsigned)pc.B), dim3((unsigned)l.vit_threads), 0, st, a);
        timing_end(e);
        HIPCHK(e, hipGetLastError());
    }
    if (host) HIPCHK(e, hipMemcpyAsync(pc.out, a.out, l.out_elems * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return TTS_HIP_OK;
}

int pyin_entry(tts_hip_engine* e, const PyinCall& c) {
    if (!e) return TTS_HIP_EINVAL;
    char why[256] = "";
    if (const int rc = pyin_check(c, why, sizeof why)) return set_err(e, rc, "%s", why);
    StreamScope scope(e, c.p.stream);
    return pyin_impl(e, c);
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

extern "C" int tts_hip_pyin(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop, int win,
                            int tau_min, int tau_max, const float* prior, int n_thresh, float no_trough_prob, double fmin, int bps,
                            int n_bins, int max_step, float switch_prob, float* out, int mem, void* stream) {
    return pyin_entry(e, PyinCall{PitchCall{"pyin", audio, B, N, lengths, rate, hop, win, tau_min, tau_max, 0.5f, false, -1, out, mem, stream},
                                  prior, n_thresh, no_trough_prob, fmin, bps, n_bins, max_step, switch_prob, false, -1});
}

extern "C" int tts_hip_pyin_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop,
                                  int win, int tau_min, int tau_max, const float* prior, int n_thresh, float no_trough_prob,
                                  double fmin, int bps, int n_bins, int max_step, float switch_prob, int what, float* out, int mem,
                                  void* stream) {
    return pyin_entry(e, PyinCall{PitchCall{"pyin_probe", audio, B, N, lengths, rate, hop, win, tau_min, tau_max, 0.5f, false, -1, out, mem,
                                            stream},
                                  prior, n_thresh, no_trough_prob, fmin, bps, n_bins, max_step, switch_prob, true, what});
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
