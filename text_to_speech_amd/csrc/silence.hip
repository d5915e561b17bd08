// silence.hip -- silence removal on gfx950: the rms, threshold and mean-window trim methods of
// utils/audio/audio_processing.py (:100-200, :385-394, :372-383), sample for sample, with the kept samples compacted on
// the device.
//
// Every method ends in the same two steps: a per-sample keep mask, then a stable per-row compaction (counts per tile of
// SIL_TILE samples -> exclusive scan of the tile counts -> scatter of the kept samples, zeros behind them).  What differs is
// how the mask comes about:
//   rms          per-block fp32 peak -> silent flags -> (one workgroup per row, block-wide scans over the flags) maximal
//                silent runs that last min_silence, merged where the voice between them is shorter than min_voice_time ->
//                a sorted list of dropped sample intervals and a tail cut -> mask
//   threshold    row mean (fp64 sum, rounded to fp32), first / last sample off the mean by more than the threshold -> the
//                same interval list (one leading interval, one tail cut) -> mask
//   mean-window  fp64 prefix sums of the fp32 squares (the same tile scan) -> box sums as prefix differences -> their mean
//                -> mask
// The double-precision decisions of the rms method (link, trailing end) are compiled with fp contraction off: the reference
// rounds every product before it subtracts, and an fma decides a gap of exactly min_voice_time the other way.
// The whole call is enqueued on the stream; no stage reads anything back on the host.  Every row b has its own length
// L_b <= N; nothing at or beyond L_b is read.
#include "engine.h"
#include "audio_dev.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SIL_PER = 8;                   // consecutive samples per thread of a SIL_TILE workgroup (audio_call.h)

// ---------------------------------------------------------------------------------------------- shared: scan and compaction
// Exclusive sum scan over the workgroup's threads (audio_dev.h's block_scan, shifted by one thread): the sum of the threads
// before this one, 0 for the first; `total` as block_scan's.  An inclusive value less the thread's own is the same number
// for integers only: in floating point the difference keeps the rounding of sums that held the own value, which is large
// against a small sum before it (a quiet start followed by voice).  This one adds non-negative terms only.
template <class T>
__device__ T sil_scan_exclusive(T v, T* sh, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    T base = T(0), all = T(0);
    for (int i = 0; i < nw; ++i) {
        if (i < w) base += sh[i];
        all += sh[i];
    }
    __syncthreads();
    total = all;
    const T before = __shfl_up(v, 1);
    return lane == 0 ? base : base + before;
}

// off[b][k] = sum of val[b][0..k) over the row's tiles k < ceil(L_b / SIL_TILE), total[b] = their sum (one workgroup per row;
// chunks of blockDim tiles, carried).  Serves the tile counts of the compaction (int) and the tile sums of squares (double).
template <class T>
__global__ __launch_bounds__(1024) void sil_row_scan_kernel(const T* __restrict__ val, T* __restrict__ off, int NT,
                                                            const int* __restrict__ lens, T* __restrict__ total) {
    __shared__ T sh[16];
    const int b = blockIdx.x, nt = (lens[b] + SIL_TILE - 1) / SIL_TILE;
    T carry = T(0);
    for (int c0 = 0; c0 < nt; c0 += blockDim.x) {
        const int k = c0 + threadIdx.x;
        const T v = k < nt ? val[(long long)b * NT + k] : T(0);
        T all;
        const T before = sil_scan_exclusive(v, sh, all);
        if (k < nt) off[(long long)b * NT + k] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0 && total) total[b] = carry;
}

// cnt[b][tile] = kept samples of the tile
__global__ __launch_bounds__(256) void sil_tile_count_kernel(const uint8_t* __restrict__ mask, int N, int NT,
                                                             const int* __restrict__ lens, int* __restrict__ cnt) {
    __shared__ int sh[16];
    const int b = blockIdx.y, L = lens[b], t0 = blockIdx.x * SIL_TILE + threadIdx.x * SIL_PER;
    if (blockIdx.x * SIL_TILE >= L) return;
    int c = 0;
#pragma unroll
    for (int u = 0; u < SIL_PER; ++u)
        if (t0 + u < L) c += mask[(long long)b * N + t0 + u];
    const int all = block_reduce(c, sh, OpAdd());
    if (threadIdx.x == 0) cnt[b * NT + blockIdx.x] = all;
}

// out[b][off + rank] = x[b][t] for the kept samples of the tile, in order; out[b][t] = 0 for t >= out_len[b] (all of [0, N))
__global__ __launch_bounds__(256) void sil_scatter_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int N,
                                                          int NT, const int* __restrict__ lens, const int* __restrict__ off,
                                                          const int* __restrict__ out_len, float* __restrict__ out) {
    __shared__ int sh[16];
    const int b = blockIdx.y, L = lens[b], t0 = blockIdx.x * SIL_TILE + threadIdx.x * SIL_PER;
    const long long row = (long long)b * N;
    const int kept = out_len[b];
    if (blockIdx.x * SIL_TILE < L) {            // uniform per workgroup
        float v[SIL_PER];
        bool k[SIL_PER];
        int c = 0;
#pragma unroll
        for (int u = 0; u < SIL_PER; ++u) {
            k[u] = t0 + u < L && mask[row + t0 + u] != 0;
            v[u] = k[u] ? x[row + t0 + u] : 0.f;
            c += k[u];
        }
        int all;
        int pos = off[b * NT + blockIdx.x] + block_scan(c, sh, all, OpAdd()) - c;
#pragma unroll
        for (int u = 0; u < SIL_PER; ++u)
            if (k[u]) out[row + pos++] = v[u];
    }
#pragma unroll
    for (int u = 0; u < SIL_PER; ++u)
        if (t0 + u < N && t0 + u >= kept) out[row + t0 + u] = 0.f;
}

// What the rms and threshold methods hand to the mask: per row `n` dropped intervals [d0, d1) sorted by d0 (an empty one
// has d1 <= d0) and a tail cut (nothing at or beyond it is kept).  mask[b][t] = t < cut and t in no interval.
struct Intervals {
    int* d0;            // [B][cap]
    int* d1;            // [B][cap]
    int* n;             // [B]
    int* cut;           // [B]
    int cap;
};

__global__ void sil_interval_mask_kernel(Intervals iv, int N, const int* __restrict__ lens, uint8_t* __restrict__ mask) {
    const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lens[b]) return;
    const int* d0 = iv.d0 + (long long)b * iv.cap;
    int lo = 0, hi = iv.n[b];                   // the last interval whose d0 <= t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d0[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    bool keep = t < iv.cut[b];
    if (lo > 0 && t < iv.d1[(long long)b * iv.cap + lo - 1]) keep = false;
    mask[(long long)b * N + t] = keep ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- rms method
struct RmsParams {
    int bs, rb, mode;           // block size and replace_by in samples; 0 start_end, 1 start, 2 end, 3 remove
    double rate, bt;            // bt = bs / rate: seconds per block
    double min_silence, mvt;
    float thr;                  // (float)10^(dB / 20)
    int NB;                     // flags per row (stride)
};

// flag[b][k] = sqrtf(max x^2 over block k, fp32) < thr: one wave per block, the tail block ends at L_b
__global__ __launch_bounds__(256) void sil_block_flags_kernel(const float* __restrict__ x, int N, const int* __restrict__ lens,
                                                              RmsParams P, uint8_t* __restrict__ flag) {
    const int b = blockIdx.y, L = lens[b];
    const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long s0 = k * P.bs;
    if (s0 >= L) return;
    const int n = (int)std::min<long long>(P.bs, L - s0);
    const float* r = x + (long long)b * N + s0;
    float m = 0.f;
    for (int i = threadIdx.x & 63; i < n; i += 64) m = fmaxf(m, r[i] * r[i]);
    m = wave_reduce(m, OpMax());
    if ((threadIdx.x & 63) == 0) flag[(long long)b * P.NB + k] = sqrtf(m) < P.thr ? 1 : 0;
}

// The double-precision decisions of the rms method are the reference's Python doubles: every product is rounded before it is
// subtracted or compared.  Contracted into one fma the product is not, and a voice of exactly min_voice_time (20 blocks of
// 10 ms at the defaults: 30 * 0.01 - 10 * 0.01 = 0.19999999999999998 < 0.2, but fma(30, 0.01, -0.1) = 0.2) or a silence that
// ends one sample before the row does is judged the other way.  So they are compiled uncontracted, and the link of a pair
// (r - 1, r) is one function that both of its threads call: the two cannot disagree whatever the compiler makes of it.
__device__ __forceinline__ double sil_end_seconds(int j, double bt, double Lr) {
#pragma clang fp contract(off)
    const double t = (double)j * bt;
    return fmin(Lr, t);
}

// silence (i_next, .) starts less than min_voice_time after silence (., j_prev) ends
__device__ __forceinline__ bool sil_links(int j_prev, int i_next, double bt, double Lr, double mvt) {
#pragma clang fp contract(off)
    const double s = (double)i_next * bt;
    const double e = sil_end_seconds(j_prev, bt, Lr);
    const double gap = s - e;
    return gap < mvt;
}

// a silence that ends at e seconds ends within one sample of the row's end
__device__ __forceinline__ bool sil_ends_row(double e, double rate, int L) {
#pragma clang fp contract(off)
    const double t = e * rate;
    const double d = t - (double)L;
    return fabs(d) <= 1.0;
}

// One workgroup per row, three passes, each over chunks of blockDim entries with the scans carried from chunk to chunk:
//   1. over the block flags: a silent run [i, j) ends at k = j - 1; i = 1 + the last loud block before k (max scan); the runs
//      with (j - i) * bt >= min_silence are numbered (sum scan) and listed in (si, sj)
//   2. over that list: silence r links to r - 1 when s[r] - e[r - 1] < min_voice_time (sil_links); every chain of links is
//      one merged silence, numbered by its head (sum scan): d0 = (int)(s_head * rate), d1 = (int)(e_tail * rate), the tail
//      being the silence whose successor does not link to it
//   3. over the merged silences (mode remove): each becomes its dropped interval, in place; the slice modes need the first
//      and the last only
__global__ __launch_bounds__(1024) void sil_rms_runs_kernel(const uint8_t* __restrict__ flag, const int* __restrict__ lens,
                                                            RmsParams P, int* __restrict__ si, int* __restrict__ sj,
                                                            Intervals iv) {
#pragma clang fp contract(off)
    __shared__ int sh[16];
    __shared__ int s_cut, s_last_end;
    const int b = blockIdx.x, L = lens[b], tid = threadIdx.x;
    const int nb = (int)(((long long)L + P.bs - 1) / P.bs);
    const uint8_t* f = flag + (long long)b * P.NB;
    si += (long long)b * iv.cap;
    sj += (long long)b * iv.cap;
    int* d0 = iv.d0 + (long long)b * iv.cap;
    int* d1 = iv.d1 + (long long)b * iv.cap;
    const double Lr = (double)L / P.rate;
    if (tid == 0) {
        s_cut = L;
        s_last_end = 0;
    }

    int ns = 0, prev_loud = -1;
    for (int c0 = 0; c0 < nb; c0 += blockDim.x) {
        const int k = c0 + tid;
        const bool valid = k < nb;
        const bool silent = valid && f[k] != 0;
        const bool next_silent = k + 1 < nb && f[k + 1] != 0;
        int all_loud, all_q;
        const int loud = max(prev_loud, block_scan(valid && !silent ? k : -1, sh, all_loud, OpMax()));
        const int i = loud + 1, j = k + 1;
        const int q = silent && !next_silent && (double)(j - i) * P.bt >= P.min_silence ? 1 : 0;
        const int r = ns + block_scan(q, sh, all_q, OpAdd()) - q;
        if (q && r < iv.cap) {
            si[r] = i;
            sj[r] = j;
        }
        prev_loud = max(prev_loud, all_loud);
        ns += all_q;
    }
    ns = min(ns, iv.cap);
    __syncthreads();

    int nm = 0;
    for (int c0 = 0; c0 < ns; c0 += blockDim.x) {
        const int r = c0 + tid;
        const bool valid = r < ns;
        double s = 0.0, e = 0.0;
        bool link = false, link_next = false;
        if (valid) {
            s = (double)si[r] * P.bt;
            e = sil_end_seconds(sj[r], P.bt, Lr);
            if (P.mvt != 0.0) {
                if (r > 0) link = sil_links(sj[r - 1], si[r], P.bt, Lr, P.mvt);
                if (r + 1 < ns) link_next = sil_links(sj[r], si[r + 1], P.bt, Lr, P.mvt);
            }
        }
        const int head = valid && !link ? 1 : 0;
        int all;
        const int m = nm + block_scan(head, sh, all, OpAdd()) - 1;
        if (head) d0[m] = (int)(s * P.rate);
        if (valid && !link_next) d1[m] = (int)(e * P.rate);
        if (valid && r == ns - 1) s_last_end = sil_ends_row(e, P.rate, L) ? 1 : 0;
        nm += all;
    }
    __syncthreads();

    if (P.mode == 3) {
        const long long rb = P.rb, h = P.rb / 2;
        for (int c0 = 0; c0 < nm; c0 += blockDim.x) {
            const int m = c0 + tid;
            if (m >= nm) continue;
            const long long S = d0[m], E = d1[m];
            long long a = S, z = S;                         // empty
            if (S == 0) {
                a = 0;
                z = std::max<long long>(0, E - rb);
            } else if (llabs(E - (long long)L) <= 1) {
                atomicMin(&s_cut, (int)std::min<long long>(L, S + rb));
            } else if (S + h < E - h) {
                a = S + h;
                z = E - h;
            }
            d0[m] = (int)a;
            d1[m] = (int)z;
        }
        __syncthreads();
        if (tid == 0) {
            iv.n[b] = nm;
            iv.cut[b] = s_cut;
        }
    } else if (tid == 0) {
        int a = 0, cut = L;
        if (nm > 0) {
            if (P.mode != 1 && s_last_end) cut = (int)std::min<long long>(L, (long long)d0[nm - 1] + P.rb);
            if (P.mode != 2 && si[0] == 0) a = (int)std::max<long long>(0, (long long)d1[0] - P.rb);
        }
        d0[0] = 0;
        d1[0] = a;
        iv.n[b] = 1;
        iv.cut[b] = cut;
    }
}

// ---------------------------------------------------------------------------------------------- threshold method
// m = (float)mean(x); first / last t with fabsf(x[t] - m) > thr; keeps [first, last) (mode: which of the two ends are cut)
__global__ __launch_bounds__(1024) void sil_threshold_bounds_kernel(const float* __restrict__ x, int N,
                                                                    const int* __restrict__ lens, float thr, int mode,
                                                                    Intervals iv) {
    __shared__ double shd[16];
    __shared__ int shi[16];
    const int b = blockIdx.x, L = lens[b];
    const float* r = x + (long long)b * N;
    double s = 0.0, sum;
    for (int t = threadIdx.x; t < L; t += blockDim.x) s += (double)r[t];
    block_scan(s, shd, sum, OpAdd());
    const float mean = (float)(sum / (double)L);
    int last = -1, first_neg = -1;                      // first as max of -(t + 1) + ...: keep both as max reductions
    for (int t = threadIdx.x; t < L; t += blockDim.x)
        if (fabsf(r[t] - mean) > thr) {
            last = max(last, t);
            first_neg = max(first_neg, L - 1 - t);
        }
    const int last_all = block_reduce(last, shi, OpMax()), first_all = block_reduce(first_neg, shi, OpMax());
    if (threadIdx.x != 0) return;
    int a = 0, cut = L;
    if (last_all >= 0) {
        if (mode != 2) a = L - 1 - first_all;
        if (mode != 1) cut = last_all;
    }
    iv.d0[(long long)b * iv.cap] = 0;
    iv.d1[(long long)b * iv.cap] = a;
    iv.n[b] = 1;
    iv.cut[b] = cut;
}

// ---------------------------------------------------------------------------------------------- mean-window method
// tsum[b][tile] = sum of the tile's fp32 squares, in fp64
__global__ __launch_bounds__(256) void sil_square_sum_kernel(const float* __restrict__ x, int N, int NT,
                                                             const int* __restrict__ lens, double* __restrict__ tsum) {
    __shared__ double sh[16];
    const int b = blockIdx.y, L = lens[b], t0 = blockIdx.x * SIL_TILE + threadIdx.x * SIL_PER;
    if (blockIdx.x * SIL_TILE >= L) return;
    double c = 0.0;
#pragma unroll
    for (int u = 0; u < SIL_PER; ++u)
        if (t0 + u < L) {
            const float v = x[(long long)b * N + t0 + u];
            c += (double)(v * v);
        }
    double all;
    block_scan(c, sh, all, OpAdd());
    if (threadIdx.x == 0) tsum[b * NT + blockIdx.x] = all;
}

// P[b][t] = sum of x[0..t)^2 for t in [0, L_b] (row stride N + 1)
__global__ __launch_bounds__(256) void sil_square_prefix_kernel(const float* __restrict__ x, int N, int NT,
                                                                const int* __restrict__ lens, const double* __restrict__ toff,
                                                                double* __restrict__ P) {
    __shared__ double sh[16];
    const int b = blockIdx.y, L = lens[b], t0 = blockIdx.x * SIL_TILE + threadIdx.x * SIL_PER;
    if (blockIdx.x * SIL_TILE >= L) return;
    double q[SIL_PER], c = 0.0;
#pragma unroll
    for (int u = 0; u < SIL_PER; ++u) {
        float v = 0.f;
        if (t0 + u < L) v = x[(long long)b * N + t0 + u];
        q[u] = (double)(v * v);
        c += q[u];
    }
    double all;
    double run = toff[b * NT + blockIdx.x] + sil_scan_exclusive(c, sh, all);
    double* p = P + (long long)b * (N + 1);
#pragma unroll
    for (int u = 0; u < SIL_PER; ++u) {
        if (t0 + u < L) p[t0 + u] = run;
        run += q[u];
        if (t0 + u == L - 1) p[L] = run;
    }
}

// np.convolve(x^2, ones(w) / (w * threshold), 'same')[t]: the squares of samples [t + (w-1)/2 - (w-1), t + (w-1)/2], clipped
__device__ __forceinline__ double box_conv(const double* __restrict__ p, int L, int t, int w, double scale) {
    const int hi = min(L - 1, t + (w - 1) / 2), lo = max(0, t + (w - 1) / 2 - (w - 1));
    return (p[hi + 1] - p[lo]) * scale;
}

// csum[b][tile] = sum of the tile's conv values
__global__ __launch_bounds__(256) void sil_conv_sum_kernel(const double* __restrict__ P, int N, int NT,
                                                           const int* __restrict__ lens, int w, double scale,
                                                           double* __restrict__ csum) {
    __shared__ double sh[16];
    const int b = blockIdx.y, L = lens[b], t0 = blockIdx.x * SIL_TILE + threadIdx.x * SIL_PER;
    if (blockIdx.x * SIL_TILE >= L) return;
    const double* p = P + (long long)b * (N + 1);
    double c = 0.0;
#pragma unroll
    for (int u = 0; u < SIL_PER; ++u)
        if (t0 + u < L) c += box_conv(p, L, t0 + u, w, scale);
    double all;
    block_scan(c, sh, all, OpAdd());
    if (threadIdx.x == 0) csum[b * NT + blockIdx.x] = all;
}

// mask[b][t] = conv[t] > min(threshold, mean(conv) / 2)
__global__ void sil_conv_mask_kernel(const double* __restrict__ P, int N, const int* __restrict__ lens, int w, double scale,
                                     double threshold, const double* __restrict__ conv_total, uint8_t* __restrict__ mask) {
    const int b = blockIdx.y, L = lens[b], t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= L) return;
    const double th = fmin(threshold, conv_total[b] / (double)L / 2.0);
    mask[(long long)b * N + t] = box_conv(P + (long long)b * (N + 1), L, t, w, scale) > th ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- host side
// What tts_hip_remove_silence_probe asks of sil_run: stop behind stage `what` and copy its rows to `out` (host or device as
// `mem` says)
struct SilProbe {
    int what;
    void* out;
    int mem;
};

// `rows` rows of `bytes` bytes, `spitch` bytes apart, to rows `dpitch` bytes apart, on e->stream
int sil_copy_rows(tts_hip_engine* e, const SilProbe& p, size_t at, size_t dpitch, const void* src, size_t spitch, size_t bytes,
                  size_t rows) {
    const hipMemcpyKind kind = p.mem == TTS_HIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIPCHK(e, hipMemcpy2DAsync((char*)p.out + at, dpitch, src, spitch, bytes, rows, kind, e->stream));
    return TTS_HIP_OK;
}

// device pointers only; everything is enqueued on e->stream.  With `probe` the run ends behind that stage.
int sil_run(tts_hip_engine* e, const SilCall& c, const float* d_audio, float* d_out, int* d_out_len,
            const SilProbe* probe = nullptr) {
    const auto stop_at = [&](int stage) { return probe && probe->what == stage; };
    AudioProcDev& a = e->aproc;
    hipStream_t st = e->stream;
    const int B = c.B, N = c.N, NT = c.NT;
    HIPCHK(e, a.ws.ensure(c.total));
    char* base = (char*)a.ws.p;
    int* lens = (int*)(base + c.off_info);
    uint8_t* mask = (uint8_t*)(base + c.off_mask);
    int* cnt = (int*)(base + c.off_cnt);
    int* off = (int*)(base + c.off_off);
    const Intervals iv{(int*)(base + c.off_d0), (int*)(base + c.off_d1), (int*)(base + c.off_n), (int*)(base + c.off_cut), c.cap};
    e->audio_info_h.assign(c.lens.begin(), c.lens.end());
    if (int rc = stage_row_info(e, lens)) return rc;

    if (c.method == TTS_HIP_SILENCE_RMS) {
        RmsParams P{};
        P.bs = c.bs;
        P.rb = c.rb;
        P.mode = c.mode;
        P.rate = (double)c.rate;
        P.bt = (double)c.bs / (double)c.rate;
        P.min_silence = c.min_silence;
        P.mvt = c.mvt;
        P.thr = (float)std::pow(10.0, c.threshold / 20.0);
        P.NB = c.NB;
        uint8_t* flag = (uint8_t*)(base + c.off_flag);
        hipLaunchKernelGGL(sil_block_flags_kernel, dim3(blocks(c.NB, 4), B), dim3(256), 0, st, d_audio, N, lens, P, flag);
        HIPCHK(e, hipGetLastError());
        if (stop_at(SIL_FLAGS)) return sil_copy_rows(e, *probe, 0, (size_t)c.NB, flag, (size_t)c.NB, (size_t)c.NB, B);
        hipLaunchKernelGGL(sil_rms_runs_kernel, dim3(B), dim3(1024), 0, st, flag, lens, P, (int*)(base + c.off_si),
                           (int*)(base + c.off_sj), iv);
        HIPCHK(e, hipGetLastError());
    } else if (c.method == TTS_HIP_SILENCE_THRESHOLD) {
        hipLaunchKernelGGL(sil_threshold_bounds_kernel, dim3(B), dim3(1024), 0, st, d_audio, N, lens, (float)c.threshold, c.mode,
                           iv);
        HIPCHK(e, hipGetLastError());
    }
    if (stop_at(SIL_INTERVALS)) {               // n, cut, d0[cap], d1[cap] of every row
        const size_t cap4 = (size_t)c.cap * 4, pitch = 8 + 2 * cap4;
        if (int rc = sil_copy_rows(e, *probe, 0, pitch, iv.n, 4, 4, B)) return rc;
        if (int rc = sil_copy_rows(e, *probe, 4, pitch, iv.cut, 4, 4, B)) return rc;
        if (int rc = sil_copy_rows(e, *probe, 8, pitch, iv.d0, cap4, cap4, B)) return rc;
        return sil_copy_rows(e, *probe, 8 + cap4, pitch, iv.d1, cap4, cap4, B);
    }
    if (c.method == TTS_HIP_SILENCE_MEAN_WINDOW) {
        double* tsum = (double*)(base + c.off_tsum);
        double* toff = (double*)(base + c.off_toff);
        double* P = (double*)(base + c.off_P);
        double* tot = (double*)(base + c.off_tot);
        const double scale = 1.0 / ((double)c.w * c.threshold);
        hipLaunchKernelGGL(sil_square_sum_kernel, dim3(NT, B), dim3(256), 0, st, d_audio, N, NT, lens, tsum);
        HIPCHK(e, hipGetLastError());
        hipLaunchKernelGGL(sil_row_scan_kernel<double>, dim3(B), dim3(1024), 0, st, tsum, toff, NT, lens, (double*)nullptr);
        HIPCHK(e, hipGetLastError());
        hipLaunchKernelGGL(sil_square_prefix_kernel, dim3(NT, B), dim3(256), 0, st, d_audio, N, NT, lens, toff, P);
        HIPCHK(e, hipGetLastError());
        if (stop_at(SIL_PREFIX)) {
            const size_t row = ((size_t)N + 1) * 8;
            return sil_copy_rows(e, *probe, 0, row, P, row, row, B);
        }
        hipLaunchKernelGGL(sil_conv_sum_kernel, dim3(NT, B), dim3(256), 0, st, P, N, NT, lens, c.w, scale, tsum);
        HIPCHK(e, hipGetLastError());
        hipLaunchKernelGGL(sil_row_scan_kernel<double>, dim3(B), dim3(1024), 0, st, tsum, toff, NT, lens, tot);
        HIPCHK(e, hipGetLastError());
        hipLaunchKernelGGL(sil_conv_mask_kernel, dim3(blocks(N, 256), B), dim3(256), 0, st, P, N, lens, c.w, scale, c.threshold,
                           tot, mask);
        HIPCHK(e, hipGetLastError());
    } else {
        hipLaunchKernelGGL(sil_interval_mask_kernel, dim3(blocks(N, 256), B), dim3(256), 0, st, iv, N, lens, mask);
        HIPCHK(e, hipGetLastError());
    }
    if (stop_at(SIL_MASK)) return sil_copy_rows(e, *probe, 0, (size_t)N, mask, (size_t)N, (size_t)N, B);
    hipLaunchKernelGGL(sil_tile_count_kernel, dim3(NT, B), dim3(256), 0, st, mask, N, NT, lens, cnt);
    HIPCHK(e, hipGetLastError());
    hipLaunchKernelGGL(sil_row_scan_kernel<int>, dim3(B), dim3(1024), 0, st, cnt, off, NT, lens, d_out_len);
    HIPCHK(e, hipGetLastError());
    if (stop_at(SIL_TILE_OFFSETS)) return sil_copy_rows(e, *probe, 0, (size_t)NT * 4, off, (size_t)NT * 4, (size_t)NT * 4, B);
    hipLaunchKernelGGL(sil_scatter_kernel, dim3(NT, B), dim3(256), 0, st, d_audio, mask, N, NT, lens, off, d_out_len, d_out);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

}  // namespace

int tts_hip_remove_silence_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int method,
                                 int mode, int rate, double threshold, double min_silence, int block_size, int replace_by,
                                 double min_voice_time, float* out, int32_t* out_lengths, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    SilCall c;
    char why[256];
    if (int rc = sil_check("remove_silence_async", audio, B, N, lengths, method, mode, rate, threshold, min_silence, block_size,
                           replace_by, min_voice_time, out, out_lengths, TTS_HIP_MEM_DEVICE, c, why, sizeof why))
        return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    StreamScope scope(e, stream);
    return sil_run(e, c, audio, out, out_lengths);
}

int tts_hip_remove_silence(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int method, int mode,
                           int rate, double threshold, double min_silence, int block_size, int replace_by,
                           double min_voice_time, float* out, int32_t* out_lengths, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    SilCall c;
    char why[256];
    if (int rc = sil_check("remove_silence", audio, B, N, lengths, method, mode, rate, threshold, min_silence, block_size,
                           replace_by, min_voice_time, out, out_lengths, mem, c, why, sizeof why))
        return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4), res = io.out(out, (size_t)B * N * 4), len = io.out(out_lengths, (size_t)B * 4);
    if (int rc = io.begin()) return rc;
    if (int rc = sil_run(e, c, io.ptr<const float>(in), io.ptr<float>(res), io.ptr<int>(len))) return rc;
    return io.finish();
}

// Test hook: sil_run on the same rows up to stage `what`, then the rows that stage wrote.  *width (host memory) is set for
// every accepted call; out NULL asks for it alone.
int tts_hip_remove_silence_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int method, int mode,
                                 int rate, double threshold, double min_silence, int block_size, int replace_by,
                                 double min_voice_time, int what, void* out, int32_t* width, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    SilCall c;
    SilStage s{};
    char why[256];
    if (int rc = sil_probe_check("remove_silence_probe", audio, B, N, lengths, method, mode, rate, threshold, min_silence, block_size,
                                 replace_by, min_voice_time, what, out, width, mem, c, &s, why, sizeof why))
        return set_err(e, rc, "%s", why);
    *width = s.width;
    if (!out) return TTS_HIP_OK;
    HIPCHK(e, hipSetDevice(e->device));
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4), res = io.scratch((size_t)B * N * 4), len = io.scratch((size_t)B * 4);
    if (int rc = io.begin()) return rc;
    const SilProbe probe{what, out, mem};
    if (int rc = sil_run(e, c, io.ptr<const float>(in), io.ptr<float>(res), io.ptr<int>(len), &probe)) return rc;
    return io.finish();
}
