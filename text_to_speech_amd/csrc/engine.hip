// engine.hip -- C ABI entry points: handle lifetime, weight intake, host/device staging, timing hooks.
#include "engine.h"
#include "ttsw_host.h"

#include <cstdarg>
#include <cstring>
#include <exception>

int set_err(const tts_hip_engine* e, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    return code;
}

const HostTensor* find_tensor(const tts_hip_engine* e, const std::string& name) {
    auto it = e->host.find(name);
    return it == e->host.end() ? nullptr : &it->second;
}

int dev_alloc(tts_hip_engine* e, size_t n_floats, float** dst, std::vector<void*>& allocs, bool zero) {
    void* p = nullptr;
    if (hipError_t err = hipMalloc(&p, n_floats * sizeof(float)); err != hipSuccess) {
        if (err == hipErrorOutOfMemory) (void)hipGetLastError();
        return set_err(e, err == hipErrorOutOfMemory ? TTS_HIP_ENOMEM : TTS_HIP_EHIP, "hipMalloc(%zu bytes) -> %s",
                       n_floats * sizeof(float), hipGetErrorString(err));
    }
    allocs.push_back(p);
    if (zero) HIPCHK(e, hipMemsetAsync(p, 0, n_floats * sizeof(float), e->stream));
    *dst = (float*)p;
    return TTS_HIP_OK;
}

int upload(tts_hip_engine* e, const float* src, size_t n, float** dst, std::vector<void*>& allocs) {
    int rc = dev_alloc(e, n, dst, allocs, false);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return TTS_HIP_OK;
}

// ------------------------------------------------------------------------------------------- timing hooks
void timing_begin(tts_hip_engine* e, int kind) {
    if (!e->timing) return;
    TimedLaunch t;
    if (!e->ev_pool.empty()) {
        t = e->ev_pool.back();
        e->ev_pool.pop_back();
    } else {
        if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) return;
    }
    t.kind = kind;
    (void)hipEventRecord(t.a, e->stream);
    e->timed.push_back(t);
}
void timing_end(tts_hip_engine* e) {
    if (!e->timing || e->timed.empty()) return;
    (void)hipEventRecord(e->timed.back().b, e->stream);
}
void timing_collect(tts_hip_engine* e) {
    if (e->timed.empty()) return;
    (void)hipStreamSynchronize(e->stream);
    for (auto& t : e->timed) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess && t.kind >= 0 && t.kind < 5) {
            e->time_sum_us[t.kind] += 1e3 * ms;
            e->time_cnt[t.kind] += 1;
        }
        e->ev_pool.push_back(t);
    }
    e->timed.clear();
}

// ------------------------------------------------------------------------------------------- device-side sampling
// The reference draws WaveGlow's noise and the prenet dropout inside `infer`, on the device
// (/root/reference/architectures/waveglow_arch.py:272-274,299-302, tacotron2_arch.py:197-201).  Generator used here
// (documented so that a caller can reproduce a stream; restated in oracle/philox_ref.py):
//   Philox4x32-10 (Salmon et al., SC'11): key = (seed lo, seed hi), counter = (c lo, c hi, 0, 0) with c = offset + i / 4;
//   element i takes word i % 4 of block c.  A word x becomes u = ((x >> 8) + 0.5) * 2^-24 in (0, 1).
//   normals: words (0, 1) and (2, 3) of a block feed one Box-Muller pair each:
//     r = sqrt(-2 ln u_a), (z_a, z_b) = (r cos(2 pi u_b), r sin(2 pi u_b));
//   prenet masks (keep probability 0.5, scale 2, tacotron2_arch.py:188-203): 2.0 if the word's top bit is set else 0.0.
namespace {

struct Philox4 { uint32_t x[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(uint64_t ctr, uint64_t seed) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}
__device__ __forceinline__ float unit_open(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// The four outputs of one Philox block.  kind 0: standard normals, kind 1: prenet dropout masks.
__device__ __forceinline__ void philox_block_values(uint64_t ctr, uint64_t seed, int kind, float v[4]) {
    const Philox4 w = philox4x32_10(ctr, seed);
    if (kind == 0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float r = sqrtf(-2.0f * logf(unit_open(w.x[2 * p])));
            float sn, cs;
            sincosf(6.283185307179586f * unit_open(w.x[2 * p + 1]), &sn, &cs);
            v[2 * p] = r * cs;
            v[2 * p + 1] = r * sn;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (w.x[k] >> 31) ? 2.0f : 0.0f;
    }
}

// One thread per Philox block (4 outputs).
__global__ void philox_fill_kernel(float* __restrict__ out, long long n, uint64_t seed, uint64_t offset, int kind) {
    const long long blk = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk * 4 >= n) return;
    float v[4];
    philox_block_values(offset + (uint64_t)blk, seed, kind, v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (blk * 4 + k < n) out[blk * 4 + k] = v[k];
}

// Per-row streams: row b = blockIdx.y writes out[b * row_stride + i] = element i of stream (key[b], offset[b]) for
// i < count[b] -- the element rule of the flat kernel -- and touches nothing behind that.  The table travels by value in the
// kernel arguments (one launch per kPhiloxRows rows), so the caller's host arrays need not outlive the call.
constexpr int kPhiloxRows = 32;
struct PhiloxRows {
    uint64_t key[kPhiloxRows];
    uint64_t offset[kPhiloxRows];
    long long count[kPhiloxRows];
};
// vec4: every row base of the launch is 16-byte aligned (out is, and row_stride % 4 == 0)
__global__ void philox_fill_rows_kernel(float* __restrict__ out, long long row_stride, PhiloxRows rows, int kind, int vec4) {
    const int b = blockIdx.y;
    const long long n = rows.count[b];
    const long long blk = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk * 4 >= n) return;
    float v[4];
    philox_block_values(rows.offset[b] + (uint64_t)blk, rows.key[b], kind, v);
    float* dst = out + (long long)b * row_stride + blk * 4;
    if (vec4 && blk * 4 + 4 <= n) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (blk * 4 + k < n) dst[k] = v[k];
    }
}

}  // namespace

int philox_fill(tts_hip_engine* e, float* out, long long n, uint64_t seed, uint64_t offset, int kind, hipStream_t st) {
    if (n <= 0) return TTS_HIP_OK;
    const long long blocks = (n + 3) / 4;
    hipLaunchKernelGGL(philox_fill_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, out, n, seed, offset, kind);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}

int philox_fill_rows(tts_hip_engine* e, float* out, int B, long long row_stride, const uint64_t* keys, const uint64_t* offsets,
                     const long long* counts, int kind, hipStream_t st) {
    for (int b0 = 0; b0 < B; b0 += kPhiloxRows) {
        const int nb = B - b0 < kPhiloxRows ? B - b0 : kPhiloxRows;
        PhiloxRows rows{};
        long long most = 0;
        for (int r = 0; r < nb; ++r) {
            rows.key[r] = keys[b0 + r];
            rows.offset[r] = offsets[b0 + r];
            rows.count[r] = counts ? counts[b0 + r] : row_stride;
            if (rows.count[r] > most) most = rows.count[r];
        }
        if (most <= 0) continue;
        float* base = out + (long long)b0 * row_stride;
        const int vec4 = ((uintptr_t)base % 16 == 0 && row_stride % 4 == 0) ? 1 : 0;
        const long long blocks = (most + 3) / 4;
        hipLaunchKernelGGL(philox_fill_rows_kernel, dim3((unsigned)((blocks + 255) / 256), (unsigned)nb), dim3(256), 0, st, base,
                           row_stride, rows, kind, vec4);
        HIPCHK(e, hipGetLastError());
    }
    return TTS_HIP_OK;
}

// ------------------------------------------------------------------------------------------- audio calls: staging
int AudioStage::begin() {
    if (carve.o) HIPCHK(e, e->audio_io.ensure(carve.o));
    for (int i = 0; i < (int)slots.size(); ++i)
        if (slots[i].staged && slots[i].kind == IN)
            HIPCHK(e, hipMemcpyAsync(ptr<void>(i), slots[i].user, slots[i].bytes, hipMemcpyHostToDevice, e->stream));
    return TTS_HIP_OK;
}

int AudioStage::finish() {
    for (int i = 0; i < (int)slots.size(); ++i)
        if (slots[i].staged && slots[i].kind == OUT)
            HIPCHK(e, hipMemcpyAsync(slots[i].user, ptr<void>(i), slots[i].bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return TTS_HIP_OK;
}

int copy_stage_out(tts_hip_engine* e, const StageView& v, float* out, int mem) {
    const hipMemcpyKind kind = mem == TTS_HIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIPCHK(e, hipMemcpy2DAsync(out, v.width * 4, v.p, v.pitch * 4, v.width * 4, v.rows, kind, e->stream));
    return TTS_HIP_OK;
}

int stage_row_info(tts_hip_engine* e, int* d_info) {
    HIPCHK(e, hipMemcpyAsync(d_info, e->audio_info_h.data(), e->audio_info_h.size() * 4, hipMemcpyHostToDevice, e->stream));
    return TTS_HIP_OK;
}

// Box probe (bench.py): what the fp32 matrix pipe of THIS device sustains right now on a bare v_mfma_f32_32x32x2_f32 loop with
// the register traffic of the WN GEMMs (8 independent accumulators per wave, 2 waves per SIMD, every CU; scripts/micro/
// mfma_f32_rate.cpp is the stand-alone version: 155.3 TFLOP/s at 2.398 GHz on the round-3 boxes), and the shader clock it
// holds meanwhile.  Boxes of one pool differ by up to ~9 %: the probe puts a run's numbers in context.
typedef float probe_f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256, 2) void mfma_probe_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            unsigned long long* __restrict__ clk, int iters) {
    probe_f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = in[(threadIdx.x * 16 + i) & 4095];
        b[i] = in[(threadIdx.x * 16 + 8 + i + blockIdx.x) & 4095];
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(k + i) & 7], b[(k + 3 * i) & 7], acc[i], 0, 0, 0);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[i][r];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        clk[0] = t1 - t0;                                // shader clocks
        clk[1] = r1 - r0;                                // 100 MHz ticks
    }
}

// ------------------------------------------------------------------------------------------- C ABI
extern "C" {

int tts_hip_abi_version(void) { return 13; }

int tts_hip_create(int device, tts_hip_engine** out) {
    if (!out) return TTS_HIP_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TTS_HIP_EHIP;
    if (device < 0 || device >= n) return TTS_HIP_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return TTS_HIP_EHIP;
    tts_hip_engine* e = new (std::nothrow) tts_hip_engine();
    if (!e) return TTS_HIP_ENOMEM;
    e->device = device;
    (void)hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, device);
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
        delete e;
        return TTS_HIP_EHIP;
    }
    *out = e;
    return TTS_HIP_OK;
}

int tts_hip_destroy(tts_hip_engine* e) {
    if (!e) return TTS_HIP_EINVAL;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    timing_collect(e);
    for (auto& t : e->ev_pool) {
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    waveglow_free(e);
    tacotron2_free(e);
    melstft_free(e);
    audioproc_free(e);
    resample_free(e);
    mel_dtw_free(e);
    pitch_free(e);
    e->audio_io.release();
    (void)hipStreamDestroy(e->stream);
    delete e;
    return TTS_HIP_OK;
}

const char* tts_hip_last_error(const tts_hip_engine* e) { return e ? e->err.c_str() : "null engine"; }

int tts_hip_set_tensor(tts_hip_engine* e, const char* name, const float* data, const int64_t* dims, int ndim) {
    if (!e || !name || !data || !dims || ndim <= 0 || ndim > 8) return set_err(e, TTS_HIP_EINVAL, "set_tensor: bad argument");
    try {
        HostTensor t;
        t.dims.assign(dims, dims + ndim);
        const size_t n = checked_numel(t.dims);
        if (!n) return set_err(e, TTS_HIP_EINVAL, "set_tensor(%s): non-positive or oversized dim", name);
        t.data.assign(data, data + n);
        e->host[name] = std::move(t);
    } catch (const std::exception& ex) {                       // bad_alloc / length_error must not cross the C boundary
        return set_err(e, TTS_HIP_ENOMEM, "set_tensor(%s): %s", name, ex.what());
    }
    return TTS_HIP_OK;
}

int tts_hip_load_weights(tts_hip_engine* e, const char* path) {
    if (!e || !path) return TTS_HIP_EINVAL;
    std::string err;
    const int rc = parse_ttsw(path, &e->host, &err);
    if (rc) return set_err(e, rc, "%s", err.c_str());
    return TTS_HIP_OK;
}

int tts_hip_check_weights_file(const char* path, char* errbuf, int errbuf_len) {
    if (!path) return TTS_HIP_EINVAL;
    std::string err;
    const int rc = parse_ttsw(path, nullptr, &err);
    if (errbuf && errbuf_len > 0) snprintf(errbuf, (size_t)errbuf_len, "%s", err.c_str());
    return rc;
}

static int finalize_impl(tts_hip_engine* e);

int tts_hip_finalize(tts_hip_engine* e) {
    if (!e) return TTS_HIP_EINVAL;
    try {
        return finalize_impl(e);
    } catch (const std::exception& ex) {
        return set_err(e, TTS_HIP_ENOMEM, "finalize: %s", ex.what());
    }
}

static int finalize_impl(tts_hip_engine* e) {
    HIPCHK(e, hipSetDevice(e->device));
    int rc;
    bool has_wg = false, has_taco = false;
    for (auto& kv : e->host) {
        if (kv.first.rfind("waveglow/", 0) == 0) has_wg = true;
        if (kv.first.rfind("tacotron2/", 0) == 0) has_taco = true;
    }
    if (has_wg) {
        if ((rc = waveglow_finalize(e))) return rc;
        // the packed device copies are all that is needed from here on: drop 1 GB of host staging
        for (auto it = e->host.begin(); it != e->host.end();)
            it = (it->first.rfind("waveglow/", 0) == 0) ? e->host.erase(it) : std::next(it);
    }
    if (has_taco) {
        if ((rc = tacotron2_finalize(e))) return rc;
    }
    if (!e->stft.ready) {
        if ((rc = melstft_finalize(e))) return rc;
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return TTS_HIP_OK;
}

int tts_hip_has_model(const tts_hip_engine* e, const char* model) {
    if (!e || !model) return 0;
    if (!strcmp(model, "waveglow")) return e->wg.ready;
    if (!strcmp(model, "tacotron2")) return e->taco.ready;
    if (!strcmp(model, "mel_stft")) return e->stft.ready;
    return 0;
}

// Host callers: mel (and z, when given) go through the engine's staging buffers on the current stream.
static int wg_stage_in(tts_hip_engine* e, const float* mel, const float* z, int B, int T, const float** d_mel, const float** d_z) {
    const size_t n_mel = (size_t)B * T * 80, n_z = (size_t)B * T * 32 * 8;
    HIPCHK(e, e->wg.io_mel.ensure(n_mel * 4));
    HIPCHK(e, hipMemcpyAsync(e->wg.io_mel.p, mel, n_mel * 4, hipMemcpyHostToDevice, e->stream));
    *d_mel = e->wg.io_mel.f();
    if (z) {
        HIPCHK(e, e->wg.io_z.ensure(n_z * 4));
        HIPCHK(e, hipMemcpyAsync(e->wg.io_z.p, z, n_z * 4, hipMemcpyHostToDevice, e->stream));
        *d_z = e->wg.io_z.f();
    }
    return TTS_HIP_OK;
}

// runs of whole utterances, each within kMaxFramesPerRun frames; ragged: wg.call_table was built with the same chunkB
static int waveglow_run_chunks(tts_hip_engine* e, const float* d_mel, int B, int T, bool ragged, const float* d_z, float sigma,
                               float* d_out, int precision) {
    const int chunkB = kMaxFramesPerRun / T;
    const int* d_info = (const int*)e->wg.ragged_info.p;
    size_t tail_at = (size_t)B;
    for (int b0 = 0; b0 < B; b0 += chunkB) {
        const int nb = B - b0 < chunkB ? B - b0 : chunkB;
        const int n_tail = ragged ? e->wg.call_table.run_tails[b0 / chunkB] : 0;
        int rc = waveglow_run(e, d_mel + (size_t)b0 * T * 80, nb, T, d_z ? d_z + (size_t)b0 * T * 32 * 8 : nullptr, sigma,
                              d_out + (size_t)b0 * T * 256, precision, ragged ? d_info + b0 : nullptr,
                              ragged ? d_info + tail_at : nullptr, n_tail);
        if (rc) return rc;
        tail_at += (size_t)n_tail;
    }
    return TTS_HIP_OK;
}

// Every tts_hip_waveglow_infer* entry point: check, then table, staging, noise and the runs, in that order on one stream.
static int waveglow_call(tts_hip_engine* e, const WgCall& c) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->wg.ready) return set_err(e, TTS_HIP_ENOTREADY, "waveglow weights not finalized");
    char why[512];
    if (int rc = wg_call_check(c, why, sizeof why)) return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    StreamScope scope(e, c.async ? c.stream : nullptr);
    const int B = c.B, T = c.T;
    WgTable& tab = e->wg.call_table;
    if (c.lengths || c.noise == WG_NOISE_ROWS) wg_call_table(B, T, c.lengths, c.packed, c.packed ? B : kMaxFramesPerRun / T, &tab);
    if (c.lengths) {
        HIPCHK(e, e->wg.ragged_info.ensure(tab.info.size() * sizeof(int)));
        // (pageable source: the copy has left the table when the call returns, so the next call may rebuild it)
        HIPCHK(e, hipMemcpyAsync(e->wg.ragged_info.p, tab.info.data(), tab.info.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    const size_t n_z = (size_t)B * T * 32 * 8, n_out = (size_t)B * T * 256;
    const bool host = !c.async && c.mem == TTS_HIP_MEM_HOST;
    const float* d_mel = c.mel;
    const float* d_z = c.noise == WG_NOISE_Z ? c.z : nullptr;
    float* d_out = c.audio;
    if (host) {
        if (int rc = wg_stage_in(e, c.mel, d_z, B, T, &d_mel, &d_z)) return rc;
        HIPCHK(e, e->wg.io_out.ensure(n_out * 4));
        d_out = e->wg.io_out.f();
    }
    if (c.noise != WG_NOISE_Z) {                                 // a device buffer whatever `mem` says about mel / audio
        HIPCHK(e, e->wg.io_zgen.ensure(n_z * 4));
        d_z = e->wg.io_zgen.f();
        int rc = c.noise == WG_NOISE_SEED
                     ? philox_fill(e, e->wg.io_zgen.f(), (long long)n_z, c.seed, c.offset, TTS_HIP_RANDOM_NORMAL, e->stream)
                     : philox_fill_rows(e, e->wg.io_zgen.f(), B, (long long)T * 256, c.keys, c.offsets, tab.counts.data(),
                                        TTS_HIP_RANDOM_NORMAL, e->stream);
        if (rc) return rc;
    }
    int rc = c.packed ? waveglow_run_packed(e, d_mel, B, T, d_z, c.sigma, d_out, c.precision, (const int*)e->wg.ragged_info.p,
                                            tab.F, tab.n_gap)
                      : waveglow_run_chunks(e, d_mel, B, T, c.lengths != nullptr, d_z, c.sigma, d_out, c.precision);
    if (rc || c.async) return rc;
    if (host) HIPCHK(e, hipMemcpyAsync(c.audio, d_out, n_out * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return TTS_HIP_OK;
}

// The part of a WgCall that every entry point fills the same way; z / seed / keys and mem / stream are the entry point's own.
static WgCall wg_call(const char* who, const float* mel, int B, int T, const int32_t* lengths, bool packed, WgNoise noise,
                      float sigma, float* audio, int precision, bool async) {
    WgCall c{};
    c.who = who, c.mel = mel, c.B = B, c.T = T, c.lengths = lengths, c.packed = packed, c.noise = noise;
    c.sigma = sigma, c.audio = audio, c.precision = precision, c.async = async;
    return c;
}

// Both tts_hip_waveglow_encode entry points: check, then the lengths table, staging and the one run, on one stream.
// probe (tts_hip_waveglow_encode_probe): the same staging and the same run, stopped where the probe says; c.z and c.stats
// are NULL (the run's z goes to the handle's own buffer) and probe->out [n_probe floats] lives where c.mem says.
static int waveglow_encode_call(tts_hip_engine* e, const WgEncode& c, const WgEncodeProbe* probe = nullptr, size_t n_probe = 0) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->wg.ready) return set_err(e, TTS_HIP_ENOTREADY, "waveglow weights not finalized");
    char why[512];
    if (int rc = probe ? wg_encode_probe_check(c, *probe, why, sizeof why) : wg_encode_check(c, why, sizeof why))
        return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    StreamScope scope(e, c.async ? c.stream : nullptr);
    WaveGlowDev& wg = e->wg;
    const int B = c.B, T = c.T;
    WgTable& tab = wg.call_table;
    const int* d_lens = nullptr;
    if (c.lengths) {                                             // [lengths | tail frames] of the one run
        wg_call_table(B, T, c.lengths, false, B, &tab);
        HIPCHK(e, wg.ragged_info.ensure(tab.info.size() * sizeof(int)));
        HIPCHK(e, hipMemcpyAsync(wg.ragged_info.p, tab.info.data(), tab.info.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        d_lens = (const int*)wg.ragged_info.p;
    }
    const size_t n_audio = (size_t)B * T * 256, n_mel = (size_t)B * T * 80;
    const bool host = !c.async && c.mem == TTS_HIP_MEM_HOST;
    const float *d_audio = c.audio, *d_mel = c.mel;
    float *d_z = c.z, *d_stats = c.stats;
    if (host) {
        HIPCHK(e, wg.enc_audio.ensure(n_audio * 4));
        HIPCHK(e, wg.io_mel.ensure(n_mel * 4));
        HIPCHK(e, hipMemcpyAsync(wg.enc_audio.p, c.audio, n_audio * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(wg.io_mel.p, c.mel, n_mel * 4, hipMemcpyHostToDevice, e->stream));
        d_audio = wg.enc_audio.f(), d_mel = wg.io_mel.f();
        d_z = d_stats = nullptr;
    }
    if (!d_z || !d_stats) {                                      // the run writes both: [z | stats] it was not given a place for
        HIPCHK(e, wg.enc_z.ensure((n_audio + 3 * (size_t)B) * 4));
        if (!d_z) d_z = wg.enc_z.f();
        if (!d_stats) d_stats = wg.enc_z.f() + n_audio;
    }
    struct Scratch : DevBuf {                                    // (DevBuf has no destructor: the engine's buffers live with the handle)
        ~Scratch() { release(); }
    } tmp;
    WgEncodeProbe dev_probe{};
    if (probe) {
        dev_probe = *probe;
        if (host) {
            HIPCHK(e, tmp.ensure(n_probe * 4));
            dev_probe.out = tmp.f();
        }
    }
    int rc = waveglow_encode_run(e, d_audio, d_mel, B, T, d_lens, d_lens ? d_lens + B : nullptr, c.lengths ? tab.run_tails[0] : 0,
                                 d_z, d_stats, probe ? &dev_probe : nullptr);
    if (probe) {                                                 // always drained: the scratch buffer goes with this frame
        hipError_t herr = hipSuccess;
        if (!rc && host) herr = hipMemcpyAsync(probe->out, tmp.p, n_probe * 4, hipMemcpyDeviceToHost, e->stream);
        const hipError_t serr = hipStreamSynchronize(e->stream);
        if (rc) return rc;
        HIPCHK(e, herr);
        HIPCHK(e, serr);
        return TTS_HIP_OK;
    }
    if (rc || c.async) return rc;
    if (host && c.z) HIPCHK(e, hipMemcpyAsync(c.z, d_z, n_audio * 4, hipMemcpyDeviceToHost, e->stream));
    if (host && c.stats) HIPCHK(e, hipMemcpyAsync(c.stats, d_stats, 3 * (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return TTS_HIP_OK;
}

int tts_hip_waveglow_encode(tts_hip_engine* e, const float* audio, const float* mel, int B, int T, const int32_t* lengths, float* z,
                            float* stats, int mem) {
    const WgEncode c{"tts_hip_waveglow_encode", audio, mel, B, T, lengths, z, stats, false, mem, nullptr};
    return waveglow_encode_call(e, c);
}

int tts_hip_waveglow_encode_async(tts_hip_engine* e, const float* audio, const float* mel, int B, int T, const int32_t* lengths,
                                  float* z, float* stats, void* stream) {
    const WgEncode c{"tts_hip_waveglow_encode_async", audio, mel, B, T, lengths, z, stats, true, TTS_HIP_MEM_DEVICE, stream};
    return waveglow_encode_call(e, c);
}

// Test hook: the forward flow stopped after the init step or one flow; the stored flow state or the running sums of s.
int tts_hip_waveglow_encode_probe(tts_hip_engine* e, const float* audio, const float* mel, int B, int T, const int32_t* lengths,
                                  int flow, int what, float* out, int mem) {
    const WgEncode c{"tts_hip_waveglow_encode_probe", audio, mel, B, T, lengths, nullptr, nullptr, false, mem, nullptr};
    const WgEncodeProbe probe{flow, what, out};
    const int n = what == 1 ? 1 : flow <= 2 ? 8 : flow <= 6 ? 6 : 4;         // (after flow 11: z's channels 0 .. 3)
    return waveglow_encode_call(e, c, &probe, (size_t)(B > 0 && T > 0 ? (long long)B * T * 32 * n : 0));
}

int tts_hip_waveglow_infer(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                           float* audio, int mem) {
    WgCall c = wg_call("tts_hip_waveglow_infer", mel, B, T, nullptr, false, WG_NOISE_Z, sigma, audio, 0, false);
    c.z = z, c.mem = mem;
    return waveglow_call(e, c);
}

int tts_hip_waveglow_infer_f16(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                               float* audio, int mem) {
    WgCall c = wg_call("tts_hip_waveglow_infer_f16", mel, B, T, nullptr, false, WG_NOISE_Z, sigma, audio, 1, false);
    c.z = z, c.mem = mem;
    return waveglow_call(e, c);
}

int tts_hip_waveglow_infer_f16x3(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                                 float* audio, int mem) {
    WgCall c = wg_call("tts_hip_waveglow_infer_f16x3", mel, B, T, nullptr, false, WG_NOISE_Z, sigma, audio, 2, false);
    c.z = z, c.mem = mem;
    return waveglow_call(e, c);
}

// Test hook: the gated activations of one WN layer (before the res/skip and `end` convolutions), its conditioning plane or
// the flow state after one flow, natural position order, in any precision -- of a call without lengths, of the one run of a
// ragged call (the table and its staging are waveglow_call's) or of the packed row behind waveglow_run_packed's gather.
static int waveglow_probe_call(tts_hip_engine* e, const char* who, const float* mel, int B, int T, const int32_t* lengths,
                               bool packed, const float* z, float sigma, int precision, const WgProbe& p, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->wg.ready) return set_err(e, TTS_HIP_ENOTREADY, "waveglow weights not finalized");
    WgCall c = wg_call(who, mel, B, T, lengths, packed, WG_NOISE_Z, sigma, nullptr, precision, false);
    c.z = z, c.mem = mem;
    char why[512];
    if (int rc = wg_probe_check(c, p, why, sizeof why)) return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    WgTable& tab = e->wg.call_table;
    if (lengths) {                                               // one run: every row (ragged) or the one packed row
        wg_call_table(B, T, lengths, packed, B, &tab);
        HIPCHK(e, e->wg.ragged_info.ensure(tab.info.size() * sizeof(int)));
        HIPCHK(e, hipMemcpyAsync(e->wg.ragged_info.p, tab.info.data(), tab.info.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    // what 1: the flow's 2 * n_half channels, preceded by the early output that flows 8 and 4 append
    // what 2: the conditioning plane (bias included, gate-interleaved columns) that the Winograd form builds for the layer
    const int flow = p.flow, what = p.what;
    const int width = what == 0 ? e->wg.channels : what == 2 ? 2 * e->wg.channels : e->wg.flow[flow].n_rem + (flow % 4 == 0 && flow > 0 ? 2 : 0);
    const size_t frames = packed ? (size_t)tab.F : (size_t)B * T;
    const size_t n_out = frames * 32 * width;
    if (!n_out) return TTS_HIP_OK;                               // a packed row without a frame: `out` holds nothing
    const float* d_mel = mel;
    const float* d_z = z;
    struct Scratch : DevBuf {                                   // (DevBuf has no destructor: the engine's buffers live with the handle)
        ~Scratch() { release(); }
    } tmp;
    if (mem == TTS_HIP_MEM_HOST) {
        if (int rc = wg_stage_in(e, mel, z, B, T, &d_mel, &d_z)) return rc;
        HIPCHK(e, tmp.ensure(n_out * 4));
    }
    HIPCHK(e, e->wg.io_out.ensure((size_t)B * T * 256 * 4));      // the run's audio argument (flow 0's state)
    e->wg.probe_flow = flow;
    e->wg.probe_layer = p.layer;
    e->wg.probe_what = what;
    e->wg.probe_out = mem == TTS_HIP_MEM_HOST ? tmp.f() : p.out;
    const int* d_info = (const int*)e->wg.ragged_info.p;
    int rc = packed    ? waveglow_run_packed(e, d_mel, B, T, d_z, sigma, e->wg.io_out.f(), precision, d_info, tab.F, tab.n_gap)
             : lengths ? waveglow_run(e, d_mel, B, T, d_z, sigma, e->wg.io_out.f(), precision, d_info, d_info + B, tab.run_tails[0])
                       : waveglow_run(e, d_mel, B, T, d_z, sigma, e->wg.io_out.f(), precision);
    e->wg.probe_out = nullptr;
    e->wg.probe_flow = e->wg.probe_layer = -1;
    e->wg.probe_what = 0;
    hipError_t herr = hipSuccess;
    if (!rc && mem == TTS_HIP_MEM_HOST) herr = hipMemcpyAsync(p.out, tmp.p, n_out * 4, hipMemcpyDeviceToHost, e->stream);
    const hipError_t serr = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    HIPCHK(e, herr);
    HIPCHK(e, serr);
    return TTS_HIP_OK;
}

int tts_hip_waveglow_probe_rows(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths, int packed,
                                const float* z, float sigma, int precision, int flow, int what, int layer, float* out, int mem) {
    return waveglow_probe_call(e, "tts_hip_waveglow_probe_rows", mel, B, T, lengths, packed != 0, z, sigma, precision,
                               WgProbe{flow, what, layer, out}, mem);
}

int tts_hip_waveglow_probe(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma, int precision,
                           int flow, int what, int layer, float* out, int mem) {
    return waveglow_probe_call(e, "tts_hip_waveglow_probe", mel, B, T, nullptr, false, z, sigma, precision,
                               WgProbe{flow, what, layer, out}, mem);
}

int tts_hip_waveglow_probe_acts(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma, int flow,
                                int layer, float* acts, int mem) {
    return waveglow_probe_call(e, "tts_hip_waveglow_probe_acts", mel, B, T, nullptr, false, z, sigma, 0,
                               WgProbe{flow, 0, layer, acts}, mem);
}

int tts_hip_random_fill(tts_hip_engine* e, int kind, uint64_t seed, uint64_t offset, float* out, int64_t n, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    if (!out || n < 0 || (kind != TTS_HIP_RANDOM_NORMAL && kind != TTS_HIP_RANDOM_PRENET_MASK))
        return set_err(e, TTS_HIP_EINVAL, "random_fill: bad argument");
    HIPCHK(e, hipSetDevice(e->device));
    return philox_fill(e, out, (long long)n, seed, offset, kind, stream ? (hipStream_t)stream : e->stream);
}

// Per-row streams: row b of `out` (row_stride floats apart) = the first counts[b] elements of stream (keys[b], offsets[b]).
int tts_hip_random_fill_rows(tts_hip_engine* e, int kind, const uint64_t* keys, const uint64_t* offsets, int B,
                             int64_t row_stride, const int64_t* counts, float* out, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    if (kind != TTS_HIP_RANDOM_NORMAL && kind != TTS_HIP_RANDOM_PRENET_MASK)
        return set_err(e, TTS_HIP_EINVAL, "random_fill_rows: kind must be 0 (normal) or 1 (prenet mask), got %d", kind);
    if (!keys || !offsets) return set_err(e, TTS_HIP_EINVAL, "random_fill_rows: keys / offsets is NULL");
    if (B <= 0) return set_err(e, TTS_HIP_EINVAL, "random_fill_rows: B = %d must be positive", B);
    if (!out || row_stride < 0) return set_err(e, TTS_HIP_EINVAL, "random_fill_rows: bad argument");
    std::vector<long long> cnt((size_t)B, (long long)row_stride);
    if (counts)
        for (int b = 0; b < B; ++b) {
            if (counts[b] < 0 || counts[b] > row_stride)
                return set_err(e, TTS_HIP_EINVAL, "random_fill_rows: counts[%d] = %lld is outside [0, row_stride = %lld]", b,
                               (long long)counts[b], (long long)row_stride);
            cnt[b] = (long long)counts[b];
        }
    HIPCHK(e, hipSetDevice(e->device));
    return philox_fill_rows(e, out, B, (long long)row_stride, keys, offsets, cnt.data(), kind,
                            stream ? (hipStream_t)stream : e->stream);
}

// WaveGlow.infer with the noise drawn on the device (the reference's default: z = None, deterministic = False).
int tts_hip_waveglow_infer_seeded(tts_hip_engine* e, const float* mel, int B, int T, uint64_t seed, uint64_t offset,
                                  float sigma, float* audio, int precision, int mem) {
    WgCall c = wg_call("tts_hip_waveglow_infer_seeded", mel, B, T, nullptr, false, WG_NOISE_SEED, sigma, audio, precision, false);
    c.seed = seed, c.offset = offset, c.mem = mem;
    return waveglow_call(e, c);
}

// Device-pointer variants on a caller stream: enqueue and return (no synchronization).  Same arithmetic as the calls above.
int tts_hip_waveglow_infer_async(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                                 float* audio, int precision, void* stream) {
    WgCall c = wg_call("tts_hip_waveglow_infer_async", mel, B, T, nullptr, false, WG_NOISE_Z, sigma, audio, precision, true);
    c.z = z, c.stream = stream;
    return waveglow_call(e, c);
}

// WaveGlow.infer on a batch of unequal rows: lengths[b] frames of row b are real (NULL: the calls above, launch for launch).
int tts_hip_waveglow_infer_ragged(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths, const float* z,
                                  float sigma, float* audio, int precision, int mem) {
    WgCall c = wg_call("tts_hip_waveglow_infer_ragged", mel, B, T, lengths, false, WG_NOISE_Z, sigma, audio, precision, false);
    c.z = z, c.mem = mem;
    return waveglow_call(e, c);
}

int tts_hip_waveglow_infer_ragged_async(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                        const float* z, float sigma, float* audio, int precision, void* stream) {
    WgCall c = wg_call("tts_hip_waveglow_infer_ragged_async", mel, B, T, lengths, false, WG_NOISE_Z, sigma, audio, precision, true);
    c.z = z, c.stream = stream;
    return waveglow_call(e, c);
}

// WaveGlow.infer on a batch of unequal rows, computed as ONE packed row (the contract of the ragged calls above)
int tts_hip_waveglow_infer_packed(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths, const float* z,
                                  float sigma, float* audio, int precision, int mem) {
    WgCall c = wg_call("tts_hip_waveglow_infer_packed", mel, B, T, lengths, true, WG_NOISE_Z, sigma, audio, precision, false);
    c.z = z, c.mem = mem;
    return waveglow_call(e, c);
}

int tts_hip_waveglow_infer_packed_async(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                        const float* z, float sigma, float* audio, int precision, void* stream) {
    WgCall c = wg_call("tts_hip_waveglow_infer_packed_async", mel, B, T, lengths, true, WG_NOISE_Z, sigma, audio, precision, true);
    c.z = z, c.stream = stream;
    return waveglow_call(e, c);
}

// The ragged / packed calls with row b's noise z[b, p, c] = normal element p * 8 + c of stream (keys[b], offsets[b]), drawn
// into wg.io_zgen in the batch layout (a packed run reads it through its gather); only a row's real frames are drawn.
int tts_hip_waveglow_infer_rows_seeded(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                       const uint64_t* keys, const uint64_t* offsets, float sigma, float* audio, int precision,
                                       int packed, int mem) {
    WgCall c = wg_call("tts_hip_waveglow_infer_rows_seeded", mel, B, T, lengths, packed != 0, WG_NOISE_ROWS, sigma, audio,
                       precision, false);
    c.keys = keys, c.offsets = offsets, c.mem = mem;
    return waveglow_call(e, c);
}

int tts_hip_waveglow_infer_rows_seeded_async(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                             const uint64_t* keys, const uint64_t* offsets, float sigma, float* audio,
                                             int precision, int packed, void* stream) {
    WgCall c = wg_call("tts_hip_waveglow_infer_rows_seeded_async", mel, B, T, lengths, packed != 0, WG_NOISE_ROWS, sigma, audio,
                       precision, true);
    c.keys = keys, c.offsets = offsets, c.stream = stream;
    return waveglow_call(e, c);
}

int tts_hip_kernel_timing(tts_hip_engine* e, int enable) {
    if (!e) return TTS_HIP_EINVAL;
    timing_collect(e);
    e->timing = enable != 0;
    for (int i = 0; i < 5; ++i) {
        e->time_sum_us[i] = 0;
        e->time_cnt[i] = 0;
    }
    return TTS_HIP_OK;
}

int tts_hip_kernel_time_us(tts_hip_engine* e, int kind, double* avg_us, int64_t* launches) {
    if (!e || kind < 0 || kind >= 5) return TTS_HIP_EINVAL;
    timing_collect(e);
    if (avg_us) *avg_us = e->time_cnt[kind] ? e->time_sum_us[kind] / (double)e->time_cnt[kind] : 0.0;
    if (launches) *launches = e->time_cnt[kind];
    return TTS_HIP_OK;
}

int tts_hip_set_decoder_mode(tts_hip_engine* e, int mode) {
    if (!e || mode < 0 || mode > 3) return set_err(e, TTS_HIP_EINVAL, "set_decoder_mode: mode must be 0 (graph), 1 (persistent), 2 (fused) or 3 (auto)");
    e->taco.persist_mode = mode;
    return TTS_HIP_OK;
}

int tts_hip_last_decoder_mode(const tts_hip_engine* e) { return e ? e->taco.last_path : -1; }

int tts_hip_last_conv_paths(const tts_hip_engine* e) { return e ? e->taco.last_conv_paths : -1; }

int tts_hip_set_waveglow_form(tts_hip_engine* e, int form) {
    if (!e || form < 0 || form > 3)
        return set_err(e, TTS_HIP_EINVAL, "set_waveglow_form: form must be 0 (direct), 1 (Winograd when the call shape allows it) or a measurement form (2, 3)");
    e->wg.form_mode = form;
    return TTS_HIP_OK;
}

int tts_hip_last_waveglow_form(const tts_hip_engine* e) { return e ? e->wg.last_form : -1; }

int tts_hip_waveglow_channels(const tts_hip_engine* e) { return e && e->wg.ready ? e->wg.channels : 0; }

int tts_hip_last_waveglow_tiles(const tts_hip_engine* e) { return e ? e->wg.last_tiles : -1; }

int tts_hip_probe_mfma_f32(tts_hip_engine* e, double* tflops, double* shader_clock_ghz) {
    if (!e) return TTS_HIP_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    const int ncu = e->n_cu > 0 ? e->n_cu : 256, blocks = 2 * ncu, iters = 6000;
    DevBuf in, out, clk;
    struct Free {
        DevBuf &a, &b, &c;
        ~Free() { a.release(); b.release(); c.release(); }
    } guard{in, out, clk};
    HIPCHK(e, in.ensure(4096 * 4));
    HIPCHK(e, out.ensure((size_t)blocks * 256 * 4));
    HIPCHK(e, clk.ensure(16));
    std::vector<float> h(4096);
    uint32_t st = 12345u;
    for (auto& v : h) {                                  // N(0, 1)-like operands: the clock the part holds depends on the data
        float u = 0.f;
        for (int i = 0; i < 12; ++i) {
            st = st * 1664525u + 1013904223u;
            u += (float)(st >> 8) * (1.0f / 16777216.0f);
        }
        v = u - 6.f;
    }
    HIPCHK(e, hipMemcpyAsync(in.p, h.data(), 4096 * 4, hipMemcpyHostToDevice, e->stream));
    hipEvent_t e0, e1;
    HIPCHK(e, hipEventCreate(&e0));
    HIPCHK(e, hipEventCreate(&e1));
    double best = 0.0, ghz = 0.0;
    hipError_t err = hipSuccess;
    for (int rep = 0; rep < 3 && err == hipSuccess; ++rep) {
        (void)hipEventRecord(e0, e->stream);
        hipLaunchKernelGGL(mfma_probe_kernel, dim3(blocks), dim3(256), 0, e->stream, in.f(), out.f(), (unsigned long long*)clk.p, iters);
        (void)hipEventRecord(e1, e->stream);
        err = hipEventSynchronize(e1);
        float ms = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
        unsigned long long c[2] = {0, 1};
        if (err == hipSuccess) err = hipMemcpy(c, clk.p, 16, hipMemcpyDeviceToHost);
        const double flop = (double)blocks * 4 * iters * 64.0 * 4096.0;      // 4 waves x iters x 64 MFMAs x (32 x 32 x 2 x 2) FLOP
        if (err == hipSuccess && ms > 0.f && flop / ms / 1e9 > best) {
            best = flop / ms / 1e9;
            ghz = c[1] ? (double)c[0] / ((double)c[1] * 10.0) : 0.0;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIPCHK(e, err);
    if (tflops) *tflops = best;
    if (shader_clock_ghz) *shader_clock_ghz = ghz;
    return TTS_HIP_OK;
}

int tts_hip_synchronize(tts_hip_engine* e) {
    if (!e) return TTS_HIP_EINVAL;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return TTS_HIP_OK;
}

}  // extern "C"
