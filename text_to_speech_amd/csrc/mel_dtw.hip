// mel_dtw.hip -- mel-cepstral distortion of two ragged batches of log-mels along a dynamic-time-warping path, on gfx950.
//
// The math is pinned in include/tts_hip.h (tts_hip_mel_dtw) and restated in float64 by tests/mel_dtw_ref.py; the call's checks
// and its workspace are csrc/mel_dtw_call.h.  Four launches per aligned call:
//   dtw_cep_kernel    cepstra of both operands (DCT rows in LDS); frames at and behind a row's length are not computed.
//   dtw_dist_kernel   every d(i, j) of a pair, written in the skewed (diagonal-major) layout of MelDtwLayout.
//   dtw_sweep_kernel  one workgroup per pair sweeps the anti-diagonals k = i + j: columns j lie across the S threads, strips of
//                     S columns when lb exceeds them (the last column of a strip waits in LDS for the next one).  A cell is one
//                     float32 add; the three neighbours come from the thread's own register and from the left thread's last two
//                     values in LDS; one workgroup barrier per diagonal and nothing else -- no wait between workgroups, no flag in
//                     global memory.  The distances are prefetched P diagonals ahead, so a step waits for LDS and the barrier,
//                     not for HBM.  It writes one step code per cell (a byte, skewed as well) and the cost of the last cell.
//   dtw_path_kernel   one wave per pair: lane 0 walks the step codes back from (la - 1, lb - 1) writing the path from the
//                     buffer's end, the wave then moves it to the front, pads with -1 and writes the three statistics.
// Without TTS_HIP_DTW_ALIGN a single reduction kernel (dtw_diag_kernel) replaces the last three.  Nothing depends on the rows
// beside a pair or on the batch size: a row alone gives the bits it gives in any batch.
#include "audio_dev.h"
#include "engine.h"
#include "mel_dtw_call.h"

namespace {

constexpr int CF = 32, CR = 64;      // cepstra: frames per block, DCT rows per pass through LDS
constexpr int S = 256, P = 8;        // sweep: columns per strip (= threads), diagonals the distances are loaded ahead
constexpr double kMcdFactor = 6.141851463713754;      // 10 sqrt(2) / ln(10)
static_assert(S >= 3, "a strip's edge is rewritten S - 1 steps after its last read");

struct DtwArgs {
    const float *a, *b;              // [B][Ta][n_mel], [B][Tb][n_mel]
    const float* dct;                // [R][n_mel]
    const int* lens;                 // [2][B]
    float *cep_a, *cep_b;            // [B][Ta][R], [B][Tb][R]
    float* dist;                     // skewed [B][K][W]
    uint8_t* step;                   // skewed [B][K][W]
    float* cost;                     // skewed [B][K][W], or null
    float* final_cost;               // [B]
    float* stats;                    // [3][B]
    int32_t* path;                   // [B][K][2], or null
    int B, Ta, Tb, n_mel, R, W, K, skew_i;
};

__device__ __forceinline__ size_t skewed(const DtwArgs& g, int i, int j) { return (size_t)(i + j) * g.W + (g.skew_i ? i : j); }

__device__ __forceinline__ float dtw_dist(const float* ca, const float* cb, int R) {
    float acc = 0.f;
    for (int r = 0; r < R; ++r) {
        const float d = ca[r] - cb[r];
        acc = fmaf(d, d, acc);
    }
    return sqrtf(acc);
}

// blockIdx.x = (operand, row, chunk of CF frames)
__global__ __launch_bounds__(256) void dtw_cep_kernel(DtwArgs g, int chunks) {
    __shared__ float Dt[kDtwMaxMel * CR];        // [k][r] of the pass's rows
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % chunks, b = (blockIdx.x / chunks) % g.B, op = blockIdx.x / chunks / g.B;
    const int T = op ? g.Tb : g.Ta, len = g.lens[op * g.B + b], t0 = chunk * CF;
    if (t0 >= len) return;
    const int nf = min(CF, len - t0);
    const float* m = (op ? g.b : g.a) + ((size_t)b * T + t0) * g.n_mel;
    float* out = (op ? g.cep_b : g.cep_a) + ((size_t)b * T + t0) * g.R;
    for (int r0 = 0; r0 < g.R; r0 += CR) {
        const int nr = min(CR, g.R - r0);
        for (int idx = tid; idx < nr * g.n_mel; idx += 256) Dt[(idx % g.n_mel) * CR + idx / g.n_mel] = g.dct[(size_t)r0 * g.n_mel + idx];
        __syncthreads();
        for (int idx = tid; idx < nf * nr; idx += 256) {
            const int f = idx / nr, r = idx % nr;
            float acc = 0.f;
            for (int k = 0; k < g.n_mel; ++k) acc = fmaf(Dt[k * CR + r], m[(size_t)f * g.n_mel + k], acc);
            out[(size_t)f * g.R + r0 + r] = acc;
        }
        __syncthreads();
    }
}

// blockIdx.x = (row, diagonal, 256 entries of it)
__global__ __launch_bounds__(256) void dtw_dist_kernel(DtwArgs g, int xblocks) {
    const int xb = blockIdx.x % xblocks, k = (blockIdx.x / xblocks) % g.K, b = blockIdx.x / xblocks / g.K;
    const int x = xb * 256 + threadIdx.x, la = g.lens[b], lb = g.lens[g.B + b];
    const int i = g.skew_i ? x : k - x, j = k - i;
    if (x >= g.W || i < 0 || i >= la || j < 0 || j >= lb) return;
    g.dist[((size_t)b * g.K + k) * g.W + x] = dtw_dist(g.cep_a + ((size_t)b * g.Ta + i) * g.R, g.cep_b + ((size_t)b * g.Tb + j) * g.R, g.R);
}

// The sweep's barrier: the threads exchange through LDS only (what they write to global memory is read by later launches), so
// the step orders LDS and leaves the global loads and stores in flight -- __syncthreads drains them, and with them the
// look-ahead of the distances.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// blockIdx.x = row.  Thread tid owns column j = j0 + tid of the strip; at step t it is at cell (i = t - tid, j).
__global__ __launch_bounds__(S) void dtw_sweep_kernel(DtwArgs g) {
    __shared__ float edge[kDtwMaxFrames];        // C(i, j0 - 1): the last column of the strip before this one
    __shared__ float diag[3][S];                 // the strip's values of the last three steps
    const int b = blockIdx.x, tid = threadIdx.x;
    const int la = g.lens[b], lb = g.lens[g.B + b];
    const size_t base = (size_t)b * g.K * g.W;
    const float* dist = g.dist + base;
    uint8_t* step = g.step + base;
    float* cost = g.cost ? g.cost + base : nullptr;
    const float inf = __builtin_inff();
    for (int j0 = 0; j0 < lb; j0 += S) {
        const int j = j0 + tid, nsteps = la + min(S, lb - j0) - 1;
        const bool col = j < lb;
        float pre[P];
#pragma unroll
        for (int u = 0; u < P; ++u) {
            const int i = u - tid;
            pre[u] = dist[col && i >= 0 && i < la ? skewed(g, i, j) : 0];      // (entry 0 of the pair: loaded, never used)
        }
        float up = inf;                          // C(i - 1, j): this thread's value of the step before
        int w = 0;                               // t % 3: the buffer this step writes
        // whole rounds of P steps: behind step nsteps - 1 no cell exists (i >= la), so the up to P - 1 extra steps only meet
        // their barriers -- and the body has no branch that every thread takes, which keeps each look-ahead load in its own
        // register from issue to use
        for (int t0 = 0; t0 < nsteps; t0 += P) {
#pragma unroll
            for (int u = 0; u < P; ++u) {
                const int i = t0 + u - tid, ahead = i + P;
                const float d = pre[u];
                // an unconditional load (a cell that does not exist reads entry 0 of the pair and drops it)
                pre[u] = dist[col && ahead >= 0 && ahead < la ? skewed(g, ahead, j) : 0];
                const int w1 = w == 0 ? 2 : w - 1, w2 = w == 2 ? 0 : w + 1;      // the buffers of steps t - 1 and t - 2
                float c = inf;
                if (col && i >= 0 && i < la) {
                    float left = inf, dg = inf;                                  // C(i, j - 1), C(i - 1, j - 1)
                    if (tid > 0) {
                        left = diag[w1][tid - 1];
                        if (i > 0) dg = diag[w2][tid - 1];
                    } else if (j0 > 0) {
                        left = edge[i];
                        if (i > 0) dg = edge[i - 1];
                    }
                    float best = dg;
                    int code = 0;
                    if (up < best) best = up, code = 1;
                    if (left < best) best = left, code = 2;
                    c = i == 0 && j == 0 ? d : d + best;
                    const size_t at = skewed(g, i, j);
                    step[at] = (uint8_t)code;
                    if (cost) cost[at] = c;
                    if (i == la - 1 && j == lb - 1) g.final_cost[b] = c;
                    if (tid == S - 1) edge[i] = c;       // read again at steps i and i + 1 of the next strip only
                    up = c;
                }
                diag[w][tid] = c;
                lds_barrier();
                w = w2;
            }
        }
    }
}

// blockIdx.x = row, one wave.
__global__ __launch_bounds__(64) void dtw_path_kernel(DtwArgs g) {
    __shared__ int n_sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int la = g.lens[b], lb = g.lens[g.B + b];
    const uint8_t* step = g.step + (size_t)b * g.K * g.W;
    int32_t* path = g.path ? g.path + (size_t)b * g.K * 2 : nullptr;
    if (lane == 0) {
        int i = la - 1, j = lb - 1, n = 0;
        for (;;) {
            if (path) {
                path[2 * (size_t)(g.K - 1 - n)] = i;
                path[2 * (size_t)(g.K - 1 - n) + 1] = j;
            }
            ++n;
            if (i == 0 && j == 0) break;
            // on the first row and column only one step exists (what the sweep wrote there for finite costs)
            const int code = i == 0 ? 2 : j == 0 ? 1 : step[skewed(g, i, j)];
            if (code != 2) --i;
            if (code != 1) --j;
        }
        n_sh = n;
        const float cost = g.final_cost[b];
        g.stats[b] = cost;
        g.stats[g.B + b] = (float)n;
        g.stats[2 * (size_t)g.B + b] = (float)(kMcdFactor * (double)cost / (double)n);
    }
    __syncthreads();
    if (!path) return;
    const int n = n_sh, off = g.K - n;
    for (int t0 = 0; t0 < g.K; t0 += 64) {       // to the front, 64 pairs at a time: what a round reads no earlier round wrote
        const int t = t0 + lane;
        int pi = -1, pj = -1;
        if (t < n) pi = path[2 * (size_t)(off + t)], pj = path[2 * (size_t)(off + t) + 1];
        __syncthreads();
        if (t < g.K) path[2 * (size_t)t] = pi, path[2 * (size_t)t + 1] = pj;
        __syncthreads();
    }
}

// Without alignment: blockIdx.x = row; the diagonal's distances summed in float64 (thread t takes t, t + 256, ...).
__global__ __launch_bounds__(256) void dtw_diag_kernel(DtwArgs g) {
    __shared__ double sh[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(g.lens[b], g.lens[g.B + b]);
    double acc = 0.0;
    for (int t = tid; t < n; t += 256)
        acc += (double)dtw_dist(g.cep_a + ((size_t)b * g.Ta + t) * g.R, g.cep_b + ((size_t)b * g.Tb + t) * g.R, g.R);
    acc = block_reduce(acc, sh, OpAdd());
    if (g.path)
        for (int t = tid; t < g.K; t += 256) g.path[((size_t)b * g.K + t) * 2] = g.path[((size_t)b * g.K + t) * 2 + 1] = t < n ? t : -1;
    if (tid == 0) {
        const float cost = (float)acc;
        g.stats[b] = cost;
        g.stats[g.B + b] = (float)n;
        g.stats[2 * (size_t)g.B + b] = (float)(kMcdFactor * (double)cost / (double)n);
    }
}

// The probe's dense results, zeros at and behind the lengths
__global__ __launch_bounds__(256) void dtw_dense_cep_kernel(DtwArgs g, int op, float* out, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int T = op ? g.Tb : g.Ta;
    const int t = (int)(idx / g.R % T), b = (int)(idx / g.R / T);
    out[idx] = t < g.lens[op * g.B + b] ? (op ? g.cep_b : g.cep_a)[idx] : 0.f;
}
template <class T>
__global__ __launch_bounds__(256) void dtw_dense_kernel(DtwArgs g, const T* src, float* out, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % g.Tb), i = (int)(idx / g.Tb % g.Ta), b = (int)(idx / g.Tb / g.Ta);
    out[idx] = i < g.lens[b] && j < g.lens[g.B + b] ? (float)src[(size_t)b * g.K * g.W + skewed(g, i, j)] : 0.f;
}

// The handle's DCT table for these settings, built on first use
int dtw_table(tts_hip_engine* e, int n_mel, int n_cep, bool c0, const float** out) {
    auto& slot = e->dtw.dct[std::make_tuple(n_mel, n_cep, (int)c0)];
    if (!slot) {
        const std::vector<float> D = mel_dtw_dct(n_mel, n_cep, c0);
        float* p = nullptr;
        HIPCHK(e, hipMalloc(&p, D.size() * sizeof(float)));
        const hipError_t err = hipMemcpy(p, D.data(), D.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            (void)hipFree(p);
            return set_err(e, TTS_HIP_EHIP, "mel_dtw: DCT table upload -> %s", hipGetErrorString(err));
        }
        slot = p;
    }
    *out = slot;
    return TTS_HIP_OK;
}

// (The request already passed mel_dtw_check.)  Enqueued on e->stream, which is drained before returning.
int mel_dtw_impl(tts_hip_engine* e, const MelDtwCall& c) {
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const MelDtwLayout l = mel_dtw_layout(c);
    const float* dct = nullptr;
    if (const int rc = dtw_table(e, c.n_mel, c.n_cep, (c.flags & TTS_HIP_DTW_C0) != 0, &dct)) return rc;
    HIPCHK(e, e->dtw.ws.ensure(l.bytes));
    char* ws = (char*)e->dtw.ws.p;
    const bool host = c.mem == TTS_HIP_MEM_HOST, probing = dtw_probing(c);
    const size_t B = (size_t)c.B;

    std::vector<int32_t>& lens = e->dtw.lens_h;
    lens.resize(2 * B);
    for (int b = 0; b < c.B; ++b) lens[b] = c.len_a ? c.len_a[b] : c.Ta, lens[B + b] = c.len_b ? c.len_b[b] : c.Tb;
    HIPCHK(e, hipMemcpyAsync(ws + l.lens, lens.data(), 2 * B * sizeof(int32_t), hipMemcpyHostToDevice, st));

    DtwArgs g{};
    g.a = c.a, g.b = c.b;
    if (host) {
        HIPCHK(e, hipMemcpyAsync(ws + l.in_a, c.a, B * c.Ta * c.n_mel * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(ws + l.in_b, c.b, B * c.Tb * c.n_mel * sizeof(float), hipMemcpyHostToDevice, st));
        g.a = (const float*)(ws + l.in_a), g.b = (const float*)(ws + l.in_b);
    }
    g.dct = dct, g.lens = (const int*)(ws + l.lens);
    g.cep_a = (float*)(ws + l.cep_a), g.cep_b = (float*)(ws + l.cep_b);
    g.dist = (float*)(ws + l.dist), g.step = (uint8_t*)(ws + l.step);
    g.cost = probing && c.what == TTS_HIP_DTW_COST ? (float*)(ws + l.cost) : nullptr;
    g.final_cost = (float*)(ws + l.final_cost);
    g.stats = host ? (float*)(ws + l.stats) : c.stats;
    g.path = !c.path ? nullptr : host ? (int32_t*)(ws + l.path) : c.path;
    g.B = c.B, g.Ta = c.Ta, g.Tb = c.Tb, g.n_mel = c.n_mel, g.R = l.R, g.W = l.W, g.K = l.K, g.skew_i = l.skew_i;

    // grids: B * Ta * Tb <= 2^25 bounds every product below
    const int chunks = ((c.Ta > c.Tb ? c.Ta : c.Tb) + CF - 1) / CF, xblocks = (l.W + 255) / 256;
    timing_begin(e, 0);
    hipLaunchKernelGGL(dtw_cep_kernel, dim3((unsigned)(2 * B * chunks)), dim3(256), 0, st, g, chunks);
    timing_end(e);
    HIPCHK(e, hipGetLastError());
    if (l.aligned) {
        timing_begin(e, 1);
        hipLaunchKernelGGL(dtw_dist_kernel, dim3((unsigned)(B * l.K * xblocks)), dim3(256), 0, st, g, xblocks);
        timing_end(e);
        HIPCHK(e, hipGetLastError());
        if (!probing || c.what >= TTS_HIP_DTW_COST) {
            timing_begin(e, 2);
            hipLaunchKernelGGL(dtw_sweep_kernel, dim3((unsigned)B), dim3(S), 0, st, g);
            timing_end(e);
            HIPCHK(e, hipGetLastError());
        }
    }
    if (!probing) {
        timing_begin(e, 3);
        if (l.aligned) hipLaunchKernelGGL(dtw_path_kernel, dim3((unsigned)B), dim3(64), 0, st, g);
        else hipLaunchKernelGGL(dtw_diag_kernel, dim3((unsigned)B), dim3(256), 0, st, g);
        timing_end(e);
        HIPCHK(e, hipGetLastError());
        if (host) {
            HIPCHK(e, hipMemcpyAsync(c.stats, g.stats, 3 * B * sizeof(float), hipMemcpyDeviceToHost, st));
            if (c.path) HIPCHK(e, hipMemcpyAsync(c.path, g.path, B * l.K * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
    } else {
        float* out = host ? (float*)(ws + l.out) : c.out;
        const dim3 grid((unsigned)((l.out_elems + 255) / 256));
        if (c.what <= TTS_HIP_DTW_CEPSTRA_B) hipLaunchKernelGGL(dtw_dense_cep_kernel, grid, dim3(256), 0, st, g, c.what, out, l.out_elems);
        else if (c.what == TTS_HIP_DTW_STEP) hipLaunchKernelGGL(dtw_dense_kernel<uint8_t>, grid, dim3(256), 0, st, g, (const uint8_t*)g.step, out, l.out_elems);
        else hipLaunchKernelGGL(dtw_dense_kernel<float>, grid, dim3(256), 0, st, g, c.what == TTS_HIP_DTW_COST ? (const float*)g.cost : (const float*)g.dist, out, l.out_elems);
        HIPCHK(e, hipGetLastError());
        if (host) HIPCHK(e, hipMemcpyAsync(c.out, out, l.out_elems * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(e, hipStreamSynchronize(st));
    return TTS_HIP_OK;
}

int mel_dtw_entry(tts_hip_engine* e, const MelDtwCall& c) {
    if (!e) return TTS_HIP_EINVAL;
    char why[256] = "";
    if (const int rc = mel_dtw_check(c, why, sizeof why)) return set_err(e, rc, "%s", why);
    StreamScope scope(e, c.stream);
    return mel_dtw_impl(e, c);
}

}  // namespace

void mel_dtw_free(tts_hip_engine* e) {
    for (auto& kv : e->dtw.dct)
        if (kv.second) (void)hipFree(kv.second);
    e->dtw.dct.clear();
    e->dtw.ws.release();
}

extern "C" int tts_hip_mel_dtw(tts_hip_engine* e, const float* a, const float* b, int B, int Ta, int Tb, int n_mel,
                               const int32_t* len_a, const int32_t* len_b, int n_cep, int flags, float* stats, int32_t* path,
                               int mem, void* stream) {
    return mel_dtw_entry(e, MelDtwCall{"mel_dtw", a, b, B, Ta, Tb, n_mel, len_a, len_b, n_cep, flags, stats, path, false, -1, nullptr, mem, stream});
}

extern "C" int tts_hip_mel_dtw_probe(tts_hip_engine* e, const float* a, const float* b, int B, int Ta, int Tb, int n_mel,
                                     const int32_t* len_a, const int32_t* len_b, int n_cep, int flags, int what, float* out,
                                     int mem, void* stream) {
    return mel_dtw_entry(e, MelDtwCall{"mel_dtw_probe", a, b, B, Ta, Tb, n_mel, len_a, len_b, n_cep, flags, nullptr, nullptr, true, what,
                                       out, mem, stream});
}
