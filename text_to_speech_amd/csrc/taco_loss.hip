// taco_loss.hip -- the reference's TacotronLoss on gfx950: one reduction pass over the outputs of the teacher-forced pass.
//
// Replaces the reference's custom_train_objects/losses/tacotron_loss.py:62-167 (compute_mel_loss, call) for evaluation: the
// per-row values [loss | <kind>_mel_loss ... | <kind>_mel_postnet_loss ... | gate_loss] of a batch, no gradient.  The math is
// pinned in include/tts_hip.h (tts_hip_tacotron2_loss) and restated in float64 by tests/taco_loss_ref.py.
//
// The pass is HBM-bound: 3 x [B, T, 80] + 2 x [B, T] floats are read once (mel_target twice when a weighted kind needs the
// row's extrema first) and K x B floats are written.  A row is cut into chunks of kLossChunkFrames frames -- by T alone -- and
// one block of 320 threads sums a chunk: a chunk is 320 consecutive float4 of each array and thread i takes float4 i (frame =
// i / 20: the channel axis lies across the lanes), so every load is a 16-byte load of consecutive lanes and a thread's three
// loads are in flight together.
// An element's error is computed in float32, in the reference's order of operations; from the per-thread accumulator on
// every sum is float64: the block's accumulators through LDS and wave_reduce in a fixed order, one slot of partial sums per
// block in the workspace, and a second small launch that adds a row's chunks in index order and divides.  No atomics: a result is
// reproducible bit for bit, and a row's numbers do not depend on the rows beside it.  The gate term (B x T values, 1 / 240
// of the data) is float64 throughout, so neither the clip's log(1 - o) nor max(x, 0) - x g loses digits.
#include <cfloat>

#include "audio_dev.h"
#include "dev_util.h"
#include "engine.h"
#include "taco_loss_call.h"

using ttsgemm::f32x4;

namespace {

constexpr int CF = kLossChunkFrames, NMEL = kLossMel, Q = kLossMel / 4, THREADS = CF * Q, WAVES = THREADS / 64;
static_assert(THREADS % 64 == 0 && THREADS <= 1024 && kLossSums == 2 * WAVES, "one float4 of each array per thread, two sums per wave");

struct LossArgs {
    const float *mel_target, *gate_target, *decoder_output, *mel, *stop_tokens;
    float* extrema;                  // [B][chunks][2]
    double* sums;                    // [B][chunks][kLossSums]
    float* out;                      // [K][B]
    int B, T, chunks;
    int kinds[kLossMaxKinds], n_kinds;
    int masked, from_logits;
    double finish_weight, not_finish_weight;
};

// min(y) and min(-y) over one chunk of mel_target (OpMax starts from -1: it is for magnitudes, and a log-mel is negative)
__global__ __launch_bounds__(THREADS) void loss_extrema_kernel(LossArgs a) {
    __shared__ float sh[16];
    const int b = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
    const int t0 = chunk * CF, nf = min(CF, a.T - t0);
    const f32x4* y4 = reinterpret_cast<const f32x4*>(a.mel_target + ((size_t)b * a.T + t0) * NMEL);
    float lo = FLT_MAX, nhi = FLT_MAX;
    for (int i = threadIdx.x; i < nf * Q; i += THREADS) {
        const f32x4 y = y4[i];
        lo = fminf(fminf(lo, fminf(y.x, y.y)), fminf(y.z, y.w));
        nhi = fminf(fminf(nhi, fminf(-y.x, -y.y)), fminf(-y.z, -y.w));
    }
    lo = block_reduce(lo, sh, OpMin());
    nhi = block_reduce(nhi, sh, OpMin());
    if (threadIdx.x == 0) {
        a.extrema[(size_t)blockIdx.x * 2] = lo;
        a.extrema[(size_t)blockIdx.x * 2 + 1] = nhi;
    }
}

// The partial sums of one chunk (kLossSums doubles; without a weighted kind the weighted ones are 0)
template <bool kWeighted>
__global__ __launch_bounds__(THREADS) void loss_chunk_kernel(LossArgs a) {
    __shared__ float shf[16];
    __shared__ double shd[kLossSums][THREADS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
    const int t0 = chunk * CF, nf = min(CF, a.T - t0);
    const size_t row0 = (size_t)b * a.T + t0;

    // every global load of the block first, so that the row-extrema fold below (two barriers each) waits beside them
    const bool on = tid < nf * Q;                // THREADS = CF * Q: one float4 of each array per thread
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 y = on ? reinterpret_cast<const f32x4*>(a.mel_target + row0 * NMEL)[tid] : zero;
    const f32x4 d = on ? reinterpret_cast<const f32x4*>(a.decoder_output + row0 * NMEL)[tid] : zero;
    const f32x4 p = on ? reinterpret_cast<const f32x4*>(a.mel + row0 * NMEL)[tid] : zero;
    const double m = on && a.masked ? 1.0 - (double)a.gate_target[row0 + tid / Q] : 1.0;
    const float g32 = tid < nf ? a.gate_target[row0 + tid] : 0.f, x = tid < nf ? a.stop_tokens[row0 + tid] : 0.5f;

    float ymin = 0.f, wden = 1.f;                // w = (y - ymin + 1) / (ymax - ymin + 1), over the whole padded row
    if (kWeighted) {
        const float* ex = a.extrema + (size_t)b * a.chunks * 2;
        float lo = FLT_MAX, nhi = FLT_MAX;
        for (int i = tid; i < a.chunks; i += THREADS) {
            lo = fminf(lo, ex[2 * i]);
            nhi = fminf(nhi, ex[2 * i + 1]);
        }
        ymin = block_reduce(lo, shf, OpMin());
        wden = (-block_reduce(nhi, shf, OpMin()) - ymin) + 1.f;
    }

    double acc[kLossSums] = {};
    if (on) {
        double s[2 * kLossMaxKinds] = {};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ed = y[k] - d[k], ep = y[k] - p[k];
            const float sq_d = ed * ed, ab_d = fabsf(ed), sq_p = ep * ep, ab_p = fabsf(ep);
            s[TTS_HIP_LOSS_MSE] += (double)sq_d;
            s[TTS_HIP_LOSS_MAE] += (double)ab_d;
            s[kLossMaxKinds + TTS_HIP_LOSS_MSE] += (double)sq_p;
            s[kLossMaxKinds + TTS_HIP_LOSS_MAE] += (double)ab_p;
            if (kWeighted) {
                const float w = ((y[k] - ymin) + 1.f) / wden;
                s[TTS_HIP_LOSS_WEIGHTED_MSE] += (double)(sq_d * w);
                s[TTS_HIP_LOSS_WEIGHTED_MAE] += (double)(ab_d * w);
                s[kLossMaxKinds + TTS_HIP_LOSS_WEIGHTED_MSE] += (double)(sq_p * w);
                s[kLossMaxKinds + TTS_HIP_LOSS_WEIGHTED_MAE] += (double)(ab_p * w);
            }
        }
#pragma unroll
        for (int j = 0; j < 2 * kLossMaxKinds; ++j) acc[j] = s[j] * m;
    }
    if (tid < nf) {                              // the gate term and the mask of frame t0 + tid
        const double g = (double)g32;
        double bce;
        if (a.from_logits) {
            const double xd = (double)x;
            bce = fmax(xd, 0.0) - xd * g + log1p(exp(-fabs(xd)));
        } else {
            const double o = (double)fminf(fmaxf(x, (float)1e-7), (float)(1.0 - 1e-7));
            bce = -(g * log(o) + (1.0 - g) * log(1.0 - o));
        }
        acc[kLossSumGate] = bce * (g * a.finish_weight + (1.0 - g) * a.not_finish_weight);
        acc[kLossSumMask] = a.masked ? 1.0 - g : 1.0;
    }

    // the block's kLossSums sums: every thread's accumulators through LDS, wave w then owns sums w and w + WAVES -- lane l adds
    // the accumulators of threads l, l + 64, ... in that order, and wave_reduce folds the 64 lanes.  Two reductions per wave, side
    // by side, instead of ten one behind the other: the shuffles' latency is what a block of one float4 per thread waits for.
#pragma unroll
    for (int j = 0; j < kLossSums; ++j) shd[j][tid] = acc[j];
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    double r0 = 0.0, r1 = 0.0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        r0 += shd[w][lane + 64 * k];
        r1 += shd[w + WAVES][lane + 64 * k];
    }
    r0 = wave_reduce(r0, OpAdd());
    r1 = wave_reduce(r1, OpAdd());
    if (lane == 0) {
        a.sums[(size_t)blockIdx.x * kLossSums + w] = r0;
        a.sums[(size_t)blockIdx.x * kLossSums + w + WAVES] = r1;
    }
}

// Row b: its chunks' partial sums added in index order, the divisions, the K outputs.  The partials of FT chunks are one
// run of consecutive doubles: the block loads a run at once (every thread's loads in flight together), then thread j adds sum
// j of its chunks from LDS, so a row of many chunks waits for one load latency per run, not one per chunk.
constexpr int FT = 200;                          // chunks per run: 16 000 bytes of LDS
static_assert(FT * kLossSums <= 8 * 256, "a run is at most eight loads per thread");
__global__ __launch_bounds__(256) void loss_finish_kernel(LossArgs a) {
    __shared__ double tile[FT * kLossSums];
    __shared__ double sh[kLossSums];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* p = a.sums + (size_t)b * a.chunks * kLossSums;
    double v = 0.0;
    for (int c0 = 0; c0 < a.chunks; c0 += FT) {
        const int n = min(FT, a.chunks - c0) * kLossSums;
        double t[8];                             // the run's loads first, all in flight, then their LDS writes
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = tid + u * 256 < n ? p[(size_t)c0 * kLossSums + tid + u * 256] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (tid + u * 256 < n) tile[tid + u * 256] = t[u];
        __syncthreads();
        if (tid < kLossSums)                     // 16 LDS reads in flight, then their adds in index order (+ 0.0 past the run's end)
            for (int k0 = tid; k0 < n; k0 += 16 * kLossSums) {
                double t[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) t[u] = k0 + u * kLossSums < n ? tile[k0 + u * kLossSums] : 0.0;
#pragma unroll
                for (int u = 0; u < 16; ++u) v += t[u];
            }
        __syncthreads();
    }
    if (tid < kLossSums) sh[tid] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double den = sh[kLossSumMask] * NMEL;                 // unmasked: the mask is 1, so this is T * 80
    const double gate = sh[kLossSumGate] / a.T;                 // over the padded length
    double total = gate;
    for (int i = 0; i < a.n_kinds; ++i) {
        const double dec = den != 0.0 ? sh[a.kinds[i]] / den : 0.0;                       // divide_no_nan
        const double post = den != 0.0 ? sh[kLossMaxKinds + a.kinds[i]] / den : 0.0;
        a.out[(size_t)(1 + i) * a.B + b] = (float)dec;
        a.out[(size_t)(1 + a.n_kinds + i) * a.B + b] = (float)post;
        total += dec + post;
    }
    a.out[b] = (float)total;
    a.out[(size_t)(1 + 2 * a.n_kinds) * a.B + b] = (float)gate;
}

// (The request already passed taco_loss_check.)  Enqueued on e->stream, which is drained before returning.
int tacotron2_loss_impl(tts_hip_engine* e, const TacoLossCall& c) {
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const TacoLossLayout l = taco_loss_layout(c);
    HIPCHK(e, e->taco.loss_ws.ensure(l.bytes));
    char* ws = (char*)e->taco.loss_ws.p;
    const bool host = c.mem == TTS_HIP_MEM_HOST;

    const float* in[5] = {c.mel_target, c.gate_target, c.decoder_output, c.mel, c.stop_tokens};
    if (host) {
        const size_t frames = (size_t)c.B * c.T;
        for (int i = 0; i < 5; ++i) {
            const size_t bytes = frames * (i == 1 || i == 4 ? 1 : NMEL) * sizeof(float);
            HIPCHK(e, hipMemcpyAsync(ws + l.in[i], in[i], bytes, hipMemcpyHostToDevice, st));
            in[i] = (const float*)(ws + l.in[i]);
        }
    }
    LossArgs a{};
    a.mel_target = in[0], a.gate_target = in[1], a.decoder_output = in[2], a.mel = in[3], a.stop_tokens = in[4];
    a.extrema = (float*)(ws + l.extrema), a.sums = (double*)(ws + l.sums), a.out = host ? (float*)(ws + l.out) : c.out;
    a.B = c.B, a.T = c.T, a.chunks = l.chunks, a.n_kinds = c.n_kinds;
    for (int i = 0; i < c.n_kinds; ++i) a.kinds[i] = c.kinds[i];
    a.masked = c.mask_mel_padding, a.from_logits = c.from_logits;
    a.finish_weight = c.finish_weight, a.not_finish_weight = c.not_finish_weight;

    const dim3 grid((unsigned)(c.B * l.chunks));                 // at most 65536 / 16 + 65536 blocks
    if (l.weighted) {
        hipLaunchKernelGGL(loss_extrema_kernel, grid, dim3(THREADS), 0, st, a);
        HIPCHK(e, hipGetLastError());
        hipLaunchKernelGGL(loss_chunk_kernel<true>, grid, dim3(THREADS), 0, st, a);
    } else {
        hipLaunchKernelGGL(loss_chunk_kernel<false>, grid, dim3(THREADS), 0, st, a);
    }
    HIPCHK(e, hipGetLastError());
    hipLaunchKernelGGL(loss_finish_kernel, dim3((unsigned)c.B), dim3(256), 0, st, a);
    HIPCHK(e, hipGetLastError());
    if (host) HIPCHK(e, hipMemcpyAsync(c.out, a.out, (size_t)l.K * c.B * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return TTS_HIP_OK;
}

}  // namespace

extern "C" int tts_hip_tacotron2_loss(tts_hip_engine* e, const float* mel_target, const float* gate_target,
                                      const float* decoder_output, const float* mel, const float* stop_tokens, int B, int T,
                                      const int32_t* kinds, int n_kinds, int mask_mel_padding, int from_logits,
                                      double finish_weight, double not_finish_weight, float* out, int mem, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    const TacoLossCall c{"tacotron2_loss", mel_target, gate_target, decoder_output, mel, stop_tokens, B, T, kinds, n_kinds,
                         mask_mel_padding != 0, from_logits != 0, finish_weight, not_finish_weight, out, mem, stream};
    char why[256] = "";
    if (const int rc = taco_loss_check(c, why, sizeof why)) return set_err(e, rc, "%s", why);
    StreamScope scope(e, c.stream);
    return tacotron2_loss_impl(e, c);
}
