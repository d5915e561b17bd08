// mel_stft.hip -- TacotronSTFT mel spectrogram on gfx950.
//
// Replaces /root/reference/utils/audio/stft.py:242-274 (STFT.transform: reflect pad, windowed-DFT conv1d, magnitude)
// and :306-314 (TacotronSTFT.mel_spectrogram: mag @ mel_basis^T, log(max(., 1e-5))).  The reference computes the DFT
// as a dense conv1d against a [1024, 1, 1026] basis; so does this file: frames are overlapping rows (stride 256) of
// the reflect-padded signal, fed to the fp32 MFMA GEMM without materialising them.
#include "engine.h"
#include "gemm_f32.h"

#include <cmath>

using namespace ttsgemm;

namespace {

constexpr int FL = 1024, HOP = 256, CUT = 513, NMEL = 80;
constexpr int NB = 1056;      // 2 * 513 = 1026 basis rows padded to a multiple of 32
constexpr int MAGK = 544;     // 513 padded to a multiple of 32

// y[b][p] = x[b][reflect(p - 512)], rows of y are NPS floats apart (NPS = N + 1024 rounded up to 4 for 16-B rows)
__global__ void reflect_pad_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int B, int NPS) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * NPS) return;
    const int b = (int)(idx / NPS), p = (int)(idx % NPS);
    float v = 0.f;
    if (p < N + FL) {
        int s = p - FL / 2;
        if (s < 0) s = -s;                   // numpy/keras 'reflect' (edge sample not repeated)
        if (s >= N) s = 2 * (N - 1) - s;
        v = x[(long long)b * N + s];
    }
    y[idx] = v;
}

// mag[f][c] = sqrt(re^2 + im^2), c < 513; zero in the K padding
__global__ void magnitude_kernel(const float* __restrict__ ft, float* __restrict__ mag, long long rows) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * MAGK) return;
    const long long r = idx / MAGK;
    const int c = (int)(idx % MAGK);
    float v = 0.f;
    if (c < CUT) {
        const float re = ft[r * NB + c], im = ft[r * NB + CUT + c];
        v = sqrtf(re * re + im * im);
    }
    mag[idx] = v;
}

// The logarithm is taken in double and rounded once.  logf is v_log_f32 (1 ulp of log2 x) scaled by ln 2, which is up to
// 2.1 ulps of log x where |log2 x| sits in a higher binade than |log x| (measured on 81 840 mel cells: 45 % of them more
// than 1.5 ulps off); B * F * 80 values are too few for the fp64 rate to show.
__global__ void log_clamp_kernel(float* __restrict__ m, long long n, float clip) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) m[idx] = (float)log((double)fmaxf(m[idx], clip));
}

double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

}  // namespace

void melstft_free(tts_hip_engine* e) {
    for (void* p : e->stft.allocs) (void)hipFree(p);
    e->stft.allocs.clear();
    e->stft.frames.release();
    e->stft.mag.release();
    e->stft.ready = false;
}

int melstft_finalize(tts_hip_engine* e) {
    melstft_free(e);
    // windowed DFT rows (stft.py:211-236): periodic Hann, rows 0..512 real, 513..1025 imaginary
    std::vector<float> basis((size_t)NB * FL, 0.f);
    for (int r = 0; r < CUT; ++r)
        for (int n = 0; n < FL; ++n) {
            const double win = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / FL);
            const int kn = (int)(((long long)r * n) % FL);          // exact phase reduction
            const double ang = 2.0 * M_PI * kn / FL;
            basis[(size_t)r * FL + n] = (float)((double)(float)std::cos(ang) * win);
            basis[(size_t)(CUT + r) * FL + n] = (float)((double)(float)(-std::sin(ang)) * win);
        }
    int rc = upload(e, basis.data(), basis.size(), &e->stft.basis_Bt, e->stft.allocs);
    if (rc) return rc;
    // Slaney mel filterbank (librosa.filters.mel defaults; stft.py:65-72), sr 22050, fmin 0, fmax 8000
    const double sr = 22050.0, fmin = 0.0, fmax = 8000.0;
    std::vector<double> mel_f(NMEL + 2);
    const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
    for (int i = 0; i < NMEL + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (NMEL + 1));
    std::vector<float> mb((size_t)NMEL * MAGK, 0.f);
    for (int i = 0; i < NMEL; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int c = 0; c < CUT; ++c) {
            const double fr = (sr / 2.0) * c / (CUT - 1);
            const double lower = (fr - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - fr) / (mel_f[i + 2] - mel_f[i + 1]);
            const double w = std::fmax(0.0, std::fmin(lower, upper));
            mb[(size_t)i * MAGK + c] = (float)(w * enorm);
        }
    }
    rc = upload(e, mb.data(), mb.size(), &e->stft.mel_Bt, e->stft.allocs);
    if (rc) return rc;
    e->stft.ready = true;
    return TTS_HIP_OK;
}

// stop (tts_hip_mel_stft_probe): 0 .. 3 returns right after that stage with *stop_out describing what it wrote -- 0 the
// reflect-padded rows [B][NP], 1 the spectrum [B * F][NB], 2 the magnitudes [B * F][MAGK], 3 the linear mel [B * F][80]
// (d_mel itself, before the logarithm), each with its logical width beside the stored one; -1 runs everything.
int melstft_run(tts_hip_engine* e, const float* d_audio, int B, int N, float* d_mel, int stop, StageView* stop_out) {
    MelStftDev& s = e->stft;
    auto stop_at = [&](int stage, const float* p, size_t rows, size_t width, size_t pitch) {
        if (stop == stage && stop_out) *stop_out = StageView{p, rows, width, pitch};
        return stop == stage;
    };
    const int NP = (N + FL + 3) / 4 * 4;      // padded row stride (16-B aligned rows for the float4 operand loads)
    const int F = N / HOP + 1;
    hipStream_t st = e->stream;
    HIPCHK(e, s.frames.ensure(((size_t)B * NP + 64) * 4 + (size_t)B * F * NB * 4));
    HIPCHK(e, s.mag.ensure((size_t)B * F * MAGK * 4));
    float* padded = s.frames.f();
    float* ft = padded + (((size_t)B * NP + 63) / 64) * 64;
    {
        const long long n = (long long)B * NP;
        hipLaunchKernelGGL(reflect_pad_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d_audio, padded, N, B, NP);
        HIPCHK(e, hipGetLastError());
    }
    if (stop_at(0, padded, B, (size_t)N + FL, NP)) return TTS_HIP_OK;
    // ft[b][f][r] = sum_n padded[b][f*256 + n] * basis[r][n], one z slice per row of the batch
    HIPCHK(e, gemm_small(gemm_linear(padded, HOP, FL, s.basis_Bt, FL, NB, F, ft, NP, (long long)F * NB), B, st));
    if (stop_at(1, ft, (size_t)B * F, 2 * CUT, NB)) return TTS_HIP_OK;
    {
        const long long n = (long long)B * F * MAGK;
        hipLaunchKernelGGL(magnitude_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, ft, s.mag.f(), (long long)B * F);
        HIPCHK(e, hipGetLastError());
    }
    if (stop_at(2, s.mag.f(), (size_t)B * F, CUT, MAGK)) return TTS_HIP_OK;
    // mel[m][j] = sum_c mag[m][c] * mel_basis[j][c]
    HIPCHK(e, gemm_small(gemm_linear(s.mag.f(), MAGK, MAGK, s.mel_Bt, MAGK, NMEL, B * F, d_mel), 1, st));
    if (stop_at(3, d_mel, (size_t)B * F, NMEL, NMEL)) return TTS_HIP_OK;
    {
        const long long n = (long long)B * F * NMEL;
        hipLaunchKernelGGL(log_clamp_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d_mel, n, 1e-5f);
        HIPCHK(e, hipGetLastError());
    }
    return TTS_HIP_OK;
}

int tts_hip_mel_stft_async(tts_hip_engine* e, const float* audio, int B, int N, float* mel, void* stream) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->stft.ready) return set_err(e, TTS_HIP_ENOTREADY, "mel_stft not finalized");
    if (!audio || !mel || B <= 0 || N < 1024) return set_err(e, TTS_HIP_EINVAL, "mel_stft_async: bad argument (N >= 1024)");
    HIPCHK(e, hipSetDevice(e->device));
    StreamScope scope(e, stream);
    return melstft_run(e, audio, B, N, mel);
}

int tts_hip_mel_stft(tts_hip_engine* e, const float* audio, int B, int N, float* mel, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->stft.ready) return set_err(e, TTS_HIP_ENOTREADY, "mel_stft not finalized");
    if (!audio || !mel || B <= 0 || N < 1024) return set_err(e, TTS_HIP_EINVAL, "mel_stft: bad argument (N >= 1024)");
    char why[256];
    if (int rc = audio_mem_check("mel_stft", mem, why, sizeof why)) return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4), out = io.out(mel, (size_t)B * (N / 256 + 1) * 80 * 4);
    if (int rc = io.begin()) return rc;
    if (int rc = melstft_run(e, io.ptr<const float>(in), B, N, io.ptr<float>(out))) return rc;
    return io.finish();
}

// Test hook: melstft_run on `audio` up to stage `what`, then the stage's logical extent (row padding dropped) to `out`.
int tts_hip_mel_stft_probe(tts_hip_engine* e, const float* audio, int B, int N, int what, float* out, int mem) {
    if (!e) return TTS_HIP_EINVAL;
    if (!e->stft.ready) return set_err(e, TTS_HIP_ENOTREADY, "mel_stft not finalized");
    if (!audio || !out || B <= 0 || N < 1024 || what < 0 || what > 3)
        return set_err(e, TTS_HIP_EINVAL, "mel_stft_probe: bad argument (N >= 1024, what 0 .. 3)");
    char why[256];
    if (int rc = audio_mem_check("mel_stft_probe", mem, why, sizeof why)) return set_err(e, rc, "%s", why);
    HIPCHK(e, hipSetDevice(e->device));
    AudioStage io(e, mem);
    const int in = io.in(audio, (size_t)B * N * 4);
    const int mel = io.scratch((size_t)B * (N / 256 + 1) * 80 * 4);      // the linear mel lands here (stage 3 only)
    if (int rc = io.begin()) return rc;
    StageView view{};
    if (int rc = melstft_run(e, io.ptr<const float>(in), B, N, io.ptr<float>(mel), what, &view)) return rc;
    if (int rc = copy_stage_out(e, view, out, mem)) return rc;
    return io.finish();
}
