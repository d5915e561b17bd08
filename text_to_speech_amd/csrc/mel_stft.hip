// mel_stft.hip -- mel spectrograms of any TacotronSTFT configuration and of WhisperSTFT on gfx950.
//
// Replaces the reference's utils/audio/stft.py:101-124 (MelSTFT.__call__: short-audio zero pad, pre-emphasis), :242-274
// (STFT.transform: reflect pad, windowed-DFT conv1d, magnitude), :306-314 (TacotronSTFT.mel_spectrogram: mag @ mel_basis^T,
// log(max(., 1e-5)), normalize) and :350-364 (WhisperSTFT.mel_spectrogram).  The reference computes the DFT as a dense
// conv1d against a [filter_length, 1, 2 * bins] basis; so does this file: frames are overlapping rows (stride hop_length) of
// the padded signal, fed to the fp32 MFMA GEMM without materialising them where the hop keeps them 16-byte aligned, and
// gathered first where it does not.  A plan (tts_hip_mel_fn) holds the two tables of one configuration; the fixed entry
// points tts_hip_mel_stft[_async, _probe] are calls on the handle's default plan.  include/tts_hip.h has the contract,
// audio_call.h the checks and the geometry.
#include "engine.h"
#include "audio_dev.h"
#include "gemm_f32.h"

#include <cmath>
#include <new>

using namespace ttsgemm;

namespace {

struct OpMaxAny {                       // a maximum over values of either sign (OpMax starts from -1)
    template <class T> __device__ static T id() { return -std::numeric_limits<T>::infinity(); }
    template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// x - pre * prev as one fp32 product and one fp32 difference (the reference's two ops; no fma)
__device__ __forceinline__ float pre_emphasis(float x, float prev, float pre) {
#pragma clang fp contract(off)
    const float t = pre * prev;
    return x - t;
}

// Steps 1 - 3 of a row in one pass: y[b][p] = z[reflect(p - half)] for p < L' + 2 * half, z = the row's L = lens[b] (null:
// N) samples, zero-padded to L' = max(L, wl) and pre-emphasised (pre > 0).  Rows of y are NP floats apart; everything else
// of y's n floats -- a row's slack, the rows' tails, the floats behind the last row -- is written 0, never the caller's tail.
__global__ void mel_pad_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int B, int NP, long long n,
                               const int* __restrict__ lens, int wl, int half, float pre) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long b = idx / NP;
    const int p = (int)(idx % NP);
    float v = 0.f;
    if (b < B) {
        const int L = lens ? lens[b] : N, Lp = max(L, wl);
        if (p < Lp + 2 * half) {
            int s = p - half;
            if (s < 0) s = -s;                   // numpy/keras 'reflect' (edge sample not repeated)
            if (s >= Lp) s = 2 * (Lp - 1) - s;
            const float* row = x + b * N;
            v = s < L ? row[s] : 0.f;
            if (pre > 0.f && s > 0) v = pre_emphasis(v, s - 1 < L ? row[s - 1] : 0.f, pre);
        }
    }
    y[idx] = v;
}

// frames[(b * Fr + f)][k] = y[b][f * hop + k], k < fl; zero in the K padding (hop % 4 != 0: a strided row would not be
// 16-byte aligned)
__global__ void mel_gather_kernel(const float* __restrict__ y, float* __restrict__ frames, long long rows, int Fr, int NP,
                                  int hop, int fl, int Kpad) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * Kpad) return;
    const long long r = idx / Kpad;
    const int k = (int)(idx % Kpad);
    frames[idx] = k < fl ? y[(r / Fr) * NP + (r % Fr) * (long long)hop + k] : 0.f;
}

// mag[f][c] = sqrt(re^2 + im^2), c < cut; zero in the K padding
__global__ void magnitude_kernel(const float* __restrict__ ft, float* __restrict__ mag, long long rows, int NB, int MAGK, int cut) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * MAGK) return;
    const long long r = idx / MAGK;
    const int c = (int)(idx % MAGK);
    float v = 0.f;
    if (c < cut) {
        const float re = ft[r * NB + c], im = ft[r * NB + cut + c];
        v = sqrtf(re * re + im * im);
    }
    mag[idx] = v;
}

// out[b][f][j] = log (or log10) of max(in[b][f][j], clip) for f < fo[b] (null: Fout), else 0; in has Fr >= Fout frames per
// row and may be out itself when Fr == Fout.
// The logarithm is taken in double and rounded once.  logf is v_log_f32 (1 ulp of log2 x) scaled by ln 2, which is up to
// 2.1 ulps of log x where |log2 x| sits in a higher binade than |log x| (measured on 81 840 mel cells: 45 % of them more
// than 1.5 ulps off); B * F * 80 values are too few for the fp64 rate to show.
__global__ void mel_log_kernel(const float* in, float* out, long long n, int Fr, int Fout, int nmel, const int* __restrict__ fo,
                               float clip, int base10) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long cell = idx / nmel, b = cell / Fout;
    const int f = (int)(cell % Fout), j = (int)(idx % nmel);
    float v = 0.f;
    if (f < (fo ? fo[b] : Fout)) {
        const double x = (double)fmaxf(in[(b * Fr + f) * nmel + j], clip);
        v = (float)(base10 ? log10(x) : log(x));
    }
    out[idx] = v;
}

// (x - mean) / std in place over a row's own frames F = fo[b] (null: Fout), 0 where std is 0: per_feature one workgroup per
// (mel channel blockIdx.x, row blockIdx.y) over its F cells, else one per row (grid.x = 1) over its F * nmel cells.  Mean,
// then the centred sum of squares (population std), the subtraction and the division in double; rounded once.
__global__ __launch_bounds__(256) void mel_normalize_kernel(float* __restrict__ x, int Fout, int nmel, const int* __restrict__ fo,
                                                            int per_feature) {
    __shared__ double sh[16];
    const int b = blockIdx.y, F = fo ? fo[b] : Fout;
    float* base = x + (long long)b * Fout * nmel + (per_feature ? blockIdx.x : 0);
    const long long cnt = per_feature ? F : (long long)F * nmel;
    const int step = per_feature ? nmel : 1;
    double s = 0.0;
    for (long long i = threadIdx.x; i < cnt; i += blockDim.x) s += (double)base[i * step];
    const double mean = block_reduce(s, sh, OpAdd{}) / (double)cnt;
    double q = 0.0;
    for (long long i = threadIdx.x; i < cnt; i += blockDim.x) {
        const double d = (double)base[i * step] - mean;
        q += d * d;
    }
    const double sd = sqrt(block_reduce(q, sh, OpAdd{}) / (double)cnt);
    for (long long i = threadIdx.x; i < cnt; i += blockDim.x)
        base[i * step] = sd == 0.0 ? 0.f : (float)(((double)base[i * step] - mean) / sd);
}

// rowmax[b] = the fp32 maximum over row b's own fo[b] (null: Fout) * nmel cells; one workgroup per row
__global__ __launch_bounds__(1024) void mel_rowmax_kernel(const float* __restrict__ x, int Fout, int nmel, const int* __restrict__ fo,
                                                          float* __restrict__ rowmax) {
    __shared__ float sh[16];
    const int b = blockIdx.x;
    const long long cnt = (long long)(fo ? fo[b] : Fout) * nmel;
    const float* base = x + (long long)b * Fout * nmel;
    float m = OpMaxAny::id<float>();
    for (long long i = threadIdx.x; i < cnt; i += blockDim.x) m = fmaxf(m, base[i]);
    m = block_reduce(m, sh, OpMaxAny{});
    if (threadIdx.x == 0) rowmax[b] = m;
}

// Whisper: (max(x, rowmax - 8) + 4) / 4 on a row's own cells, in fp32; the frames beyond them stay 0
__global__ void mel_whisper_kernel(float* __restrict__ x, long long n, int Fout, int nmel, const int* __restrict__ fo,
                                   const float* __restrict__ rowmax) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long cell = idx / nmel, b = cell / Fout;
    if ((int)(cell % Fout) >= (fo ? fo[b] : Fout)) return;
    const float m = fmaxf(x[idx], rowmax[b] - 8.0f);
    x[idx] = (m + 4.0f) / 4.0f;
}

void plan_free(tts_hip_mel_fn* fn) {
    if (!fn) return;
    for (void* p : fn->allocs) (void)hipFree(p);
    delete fn;
}

// the two tables of a checked plan; window [wl] or null = periodic Hann
int plan_build(tts_hip_engine* e, const MelPlan& p, const double* window, tts_hip_mel_fn** out) {
    tts_hip_mel_fn* fn = new (std::nothrow) tts_hip_mel_fn();
    if (!fn) return set_err(e, TTS_HIP_ENOMEM, "mel_fn_create: out of memory");
    fn->p = p;
    const int FL = p.fl, CUT = p.cut;
    // the window centred in filter_length (librosa.util.pad_center)
    std::vector<double> win(FL, 0.0);
    for (int i = 0; i < p.wl; ++i) win[p.lpad + i] = window ? window[i] : 0.5 - 0.5 * std::cos(2.0 * M_PI * i / p.wl);
    fn->win = win;
    // windowed DFT rows (stft.py:211-236): rows 0 .. cut - 1 real, cut .. 2 cut - 1 imaginary
    std::vector<float> basis((size_t)p.NB * p.Kpad, 0.f);
    for (int r = 0; r < CUT; ++r)
        for (int n = 0; n < FL; ++n) {
            const int kn = (int)(((long long)r * n) % FL);          // exact phase reduction
            const double ang = 2.0 * M_PI * kn / FL;
            basis[(size_t)r * p.Kpad + n] = (float)((double)(float)std::cos(ang) * win[n]);
            basis[(size_t)(CUT + r) * p.Kpad + n] = (float)((double)(float)(-std::sin(ang)) * win[n]);
        }
    int rc = upload(e, basis.data(), basis.size(), &fn->basis_Bt, fn->allocs);
    if (rc) return plan_free(fn), rc;
    // Slaney mel filterbank (librosa.filters.mel defaults; stft.py:65-72)
    std::vector<double> W;
    mel_filterbank(p, W);
    std::vector<float> mb((size_t)p.nmel * p.MAGK, 0.f);
    for (int i = 0; i < p.nmel; ++i)
        for (int c = 0; c < CUT; ++c) mb[(size_t)i * p.MAGK + c] = (float)W[(size_t)i * CUT + c];
    rc = upload(e, mb.data(), mb.size(), &fn->mel_Bt, fn->allocs);
    if (rc) return plan_free(fn), rc;
    *out = fn;
    return TTS_HIP_OK;
}

}  // namespace

// ft[b][f][r] = sum_n padded[b][f * hop + n] * basis[r][n] for the Fr frames of each of B rows, NP floats apart (`gathered`
// [B * Fr][Kpad]: gather plans only)
int mel_dft_gemm(tts_hip_engine* e, const tts_hip_mel_fn& fn, const float* padded, float* gathered, float* ft, int B, int Fr, int NP) {
    const MelPlan& p = fn.p;
    hipStream_t st = e->stream;
    const long long rows = (long long)B * Fr;
    if (p.gather) {
        const long long n = rows * p.Kpad;
        hipLaunchKernelGGL(mel_gather_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, padded, gathered, rows, Fr, NP, p.hop, p.fl, p.Kpad);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, gemm_small(gemm_linear(gathered, p.Kpad, p.Kpad, fn.basis_Bt, p.Kpad, p.NB, (int)rows, ft), 1, st));
    } else {
        // one z slice per row of the batch.  A frame is read K4 floats wide (inside the row's NP); the tables' columns from
        // filter_length on are zero
        GemmArgs a = gemm_linear(padded, p.hop, p.Kpad, fn.basis_Bt, p.Kpad, p.NB, Fr, ft, NP, (long long)Fr * p.NB);
        a.seg[0].k = p.K4;
        HIPCHK(e, gemm_small(a, B, st));
    }
    return TTS_HIP_OK;
}

// device pointers only, the call already checked (g).  ragged: the rows' lengths and frame counts go to the device; else
// every row is N samples and the kernels need no table.  stop (the probes): one of MEL_* returns right after that stage with
// *stop_out describing what it wrote, each with its logical width beside the stored one; -1 runs everything.
int mel_fn_exec(tts_hip_engine* e, const tts_hip_mel_fn& fn, const MelGeom& g, const float* d_audio, int B, int N, bool ragged,
                float* d_mel, int stop, StageView* stop_out) {
    const MelPlan& p = fn.p;
    auto stop_at = [&](int stage, const float* ptr, size_t rows, size_t width, size_t pitch) {
        if (stop == stage && stop_out) *stop_out = StageView{ptr, rows, width, pitch};
        return stop == stage;
    };
    hipStream_t st = e->stream;
    HIPCHK(e, e->stft.ws.ensure(g.total));
    char* base = (char*)e->stft.ws.p;
    int* d_info = (int*)(base + g.off_info);
    float* rowmax = (float*)(base + g.off_rowmax);
    float* padded = (float*)(base + g.off_padded);
    float* gathered = (float*)(base + g.off_gathered);
    float* ft = (float*)(base + g.off_spectrum);
    float* mag = (float*)(base + g.off_magnitude);
    const bool whisper = p.kind == TTS_HIP_MEL_WHISPER;
    float* lin = whisper ? (float*)(base + g.off_linear) : d_mel;    // Tacotron: the frames of the result are the DFT's
    const int *d_lens = nullptr, *d_fo = nullptr;
    if (ragged) {
        e->audio_info_h.assign(g.lens.begin(), g.lens.end());
        e->audio_info_h.insert(e->audio_info_h.end(), g.fout.begin(), g.fout.end());
        if (int rc = stage_row_info(e, d_info)) return rc;
        d_lens = d_info, d_fo = d_info + B;
    }
    const int Fr = g.Fr, Fout = g.Fout, NP = g.NP;
    const long long rows = (long long)B * Fr;
    {
        const long long n = (long long)B * NP + 64;
        hipLaunchKernelGGL(mel_pad_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d_audio, padded, N, B, NP, n, d_lens, p.wl, p.half,
                           (float)p.pre);
        HIPCHK(e, hipGetLastError());
    }
    if (stop_at(MEL_PADDED, padded, B, g.PW, NP)) return TTS_HIP_OK;
    if (int rc = mel_dft_gemm(e, fn, padded, gathered, ft, B, Fr, NP)) return rc;
    if (stop_at(MEL_SPECTRUM, ft, (size_t)rows, 2 * p.cut, p.NB)) return TTS_HIP_OK;
    {
        const long long n = rows * p.MAGK;
        hipLaunchKernelGGL(magnitude_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, ft, mag, rows, p.NB, p.MAGK, p.cut);
        HIPCHK(e, hipGetLastError());
    }
    if (stop_at(MEL_MAGNITUDE, mag, (size_t)rows, p.cut, p.MAGK)) return TTS_HIP_OK;
    // lin[m][j] = sum_c mag[m][c] * mel_basis[j][c]
    HIPCHK(e, gemm_small(gemm_linear(mag, p.MAGK, p.MAGK, fn.mel_Bt, p.MAGK, p.nmel, (int)rows, lin), 1, st));
    if (stop_at(MEL_LINEAR, lin, (size_t)rows, p.nmel, p.nmel)) return TTS_HIP_OK;
    const long long n = (long long)B * Fout * p.nmel;
    hipLaunchKernelGGL(mel_log_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, lin, d_mel, n, Fr, Fout, p.nmel, d_fo,
                       whisper ? 1e-10f : 1e-5f, whisper ? 1 : 0);
    HIPCHK(e, hipGetLastError());
    if (stop_at(MEL_LOG, d_mel, (size_t)B * Fout, p.nmel, p.nmel)) return TTS_HIP_OK;
    if (whisper) {
        hipLaunchKernelGGL(mel_rowmax_kernel, dim3(B), dim3(1024), 0, st, d_mel, Fout, p.nmel, d_fo, rowmax);
        HIPCHK(e, hipGetLastError());
        hipLaunchKernelGGL(mel_whisper_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d_mel, n, Fout, p.nmel, d_fo, rowmax);
        HIPCHK(e, hipGetLastError());
    } else if (p.norm != TTS_HIP_MEL_NORM_NONE) {
        const int pf = p.norm == TTS_HIP_MEL_NORM_PER_FEATURE;
        hipLaunchKernelGGL(mel_normalize_kernel, dim3(pf ? p.nmel : 1, B), dim3(256), 0, st, d_mel, Fout, p.nmel, d_fo, pf);
        HIPCHK(e, hipGetLastError());
    }
    return TTS_HIP_OK;
}

// a plan that is NULL (mel_call_check refuses it) or alive on this handle
int mel_plan_check(tts_hip_engine* e, const char* name, const tts_hip_mel_fn* fn) {
    const auto& plans = e->stft.plans;
    if (!fn || fn == e->stft.def || std::find(plans.begin(), plans.end(), fn) != plans.end()) return TTS_HIP_OK;
    return set_err(e, TTS_HIP_EINVAL, "%s: not a plan of this handle", name);
}

namespace {

// tts_hip_mel_fn_run (what = -1), tts_hip_mel_fn_probe (what = a stage, `out` takes that stage) and the fixed entry points
// on the default plan are one call
int mel_fn_sync(tts_hip_engine* e, const char* name, const tts_hip_mel_fn* fn, const float* audio, int B, int N,
                const int32_t* lengths, int what, float* out, int mem) {
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    MelGeom g;
    char why[256];
    if (int rc = mel_call_check(name, fn ? &fn->p : nullptr, audio, B, N, lengths, out, mem, &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    if (what < -1 || what >= MEL_STAGES) return set_err(e, TTS_HIP_EINVAL, "%s: no stage %d (0 .. %d)", name, what, MEL_STAGES - 1);
    HIPCHK(e, hipSetDevice(e->device));
    const size_t n_mel = (size_t)B * g.Fout * fn->p.nmel * 4;
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4);
    // a probe never produces the ordinary result: `out` takes the stage straight from the workspace
    const int res = what >= 0 ? io.scratch(n_mel) : io.out(out, n_mel);
    if (int rc = io.begin()) return rc;
    StageView view{};
    if (int rc = mel_fn_exec(e, *fn, g, io.ptr<const float>(in), B, N, lengths != nullptr, io.ptr<float>(res), what, &view)) return rc;
    if (what >= 0)
        if (int rc = copy_stage_out(e, view, out, mem)) return rc;
    return io.finish();
}

int mel_fn_async(tts_hip_engine* e, const char* name, const tts_hip_mel_fn* fn, const float* audio, int B, int N,
                 const int32_t* lengths, float* mel, void* stream) {
    if (int rc = mel_plan_check(e, name, fn)) return rc;
    MelGeom g;
    char why[256];
    if (int rc = mel_call_check(name, fn ? &fn->p : nullptr, audio, B, N, lengths, mel, TTS_HIP_MEM_DEVICE, &g, why, sizeof why))
        return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    StreamScope scope(e, stream);
    return mel_fn_exec(e, *fn, g, audio, B, N, lengths != nullptr, mel);
}

}  // namespace

void melstft_free(tts_hip_engine* e) {
    plan_free(e->stft.def);
    e->stft.def = nullptr;
    for (tts_hip_mel_fn* fn : e->stft.plans) plan_free(fn);
    e->stft.plans.clear();
    e->stft.ws.release();
    e->stft.inv_ws.release();
    e->stft.ready = false;
}

// the default plan (the caller's own plans stay)
int melstft_finalize(tts_hip_engine* e) {
    plan_free(e->stft.def);
    e->stft.def = nullptr;
    e->stft.ready = false;
    const tts_hip_mel_config cfg{TTS_HIP_MEL_TACOTRON, 22050, 80, 1024, 256, 1024, TTS_HIP_MEL_NORM_NONE, 0.0, 8000.0, 0.0};
    MelPlan p;
    char why[256];
    if (int rc = mel_cfg_check("mel_stft", &cfg, nullptr, true, &p, why, sizeof why)) return set_err(e, rc, "%s", why);
    if (int rc = plan_build(e, p, nullptr, &e->stft.def)) return rc;
    e->stft.ready = true;
    return TTS_HIP_OK;
}

int tts_hip_mel_stft_async(tts_hip_engine* e, const float* audio, int B, int N, float* mel, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->stft.ready) return set_err(e, TTS_HIP_ENOTREADY, "mel_stft not finalized");
    if (!audio || !mel || B <= 0 || N < 1024) return set_err(e, TTS_HIP_EINVAL, "mel_stft_async: bad argument (N >= 1024)");
    return mel_fn_async(e, "mel_stft_async", e->stft.def, audio, B, N, nullptr, mel, stream);
}

int tts_hip_mel_stft(tts_hip_engine* e, const float* audio, int B, int N, float* mel, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->stft.ready) return set_err(e, TTS_HIP_ENOTREADY, "mel_stft not finalized");
    if (!audio || !mel || B <= 0 || N < 1024) return set_err(e, TTS_HIP_EINVAL, "mel_stft: bad argument (N >= 1024)");
    return mel_fn_sync(e, "mel_stft", e->stft.def, audio, B, N, nullptr, -1, mel, mem);
}

// Test hook: the default plan on `audio` up to stage `what`, then the stage's logical extent (row padding dropped) to `out`.
int tts_hip_mel_stft_probe(tts_hip_engine* e, const float* audio, int B, int N, int what, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->stft.ready) return set_err(e, TTS_HIP_ENOTREADY, "mel_stft not finalized");
    if (!audio || !out || B <= 0 || N < 1024 || what < 0 || what > 3)
        return set_err(e, TTS_HIP_EINVAL, "mel_stft_probe: bad argument (N >= 1024, what 0 .. 3)");
    return mel_fn_sync(e, "mel_stft_probe", e->stft.def, audio, B, N, nullptr, what, out, mem);
}

int tts_hip_mel_fn_create(tts_hip_engine* e, const tts_hip_mel_config* cfg, const double* window, tts_hip_mel_fn** out) {
    if (!e) return TTS_HIP_EINVAL;
    if (out) *out = nullptr;
    MelPlan p;
    char why[256];
    if (int rc = mel_cfg_check("mel_fn_create", cfg, window, out != nullptr, &p, why, sizeof why)) return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    tts_hip_mel_fn* fn = nullptr;
    if (int rc = plan_build(e, p, window, &fn)) return rc;
    e->stft.plans.push_back(fn);
    *out = fn;
    return TTS_HIP_OK;
}

int tts_hip_mel_fn_free(tts_hip_engine* e, tts_hip_mel_fn* fn) {
    if (!e) return TTS_HIP_EINVAL;
    auto& plans = e->stft.plans;
    auto it = std::find(plans.begin(), plans.end(), fn);
    if (!fn || it == plans.end()) return set_err(e, TTS_HIP_EINVAL, "mel_fn_free: not a plan of this handle");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    plans.erase(it);
    plan_free(fn);
    return TTS_HIP_OK;
}

int tts_hip_mel_fn_frames(const tts_hip_mel_fn* fn, int n_samples) { return fn ? mel_out_frames(fn->p, n_samples) : -1; }

int tts_hip_mel_fn_run(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                       float* mel, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    return mel_fn_sync(e, "mel_fn_run", fn, audio, B, N, lengths, -1, mel, mem);
}

int tts_hip_mel_fn_run_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths,
                             const tts_hip_mel_fn* fn, float* mel, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    return mel_fn_async(e, "mel_fn_run_async", fn, audio, B, N, lengths, mel, stream);
}

int tts_hip_mel_fn_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                         int what, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (what < 0) return set_err(e, TTS_HIP_EINVAL, "mel_fn_probe: no stage %d (0 .. %d)", what, MEL_STAGES - 1);
    return mel_fn_sync(e, "mel_fn_probe", fn, audio, B, N, lengths, what, out, mem);
}
