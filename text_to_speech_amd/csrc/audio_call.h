// audio_call.h -- what the audio front-end calls (mel-STFT, STFT inverse / Griffin-Lim, denoise, time_stretch, formant_match, reduce_noise / trim_silence, resample, remove_silence) may be
// refused for, and the geometry those refusals rest on: pure host code on the caller's arguments (no HIP include; also built
// with plain g++ under ASan / UBSan by csrc/host_check.cpp, --audio-call, and compared there with a Python restatement,
// tests/test_audio_call.py).  The .hip files forward the message to set_err; nothing is copied or launched before a check
// has passed.  Every check is "first match wins" in the order it is written in.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../include/tts_hip.h"

inline int audio_refuse(char* msg, size_t n, const char* who, const char* fmt, ...) {
    const int at = snprintf(msg, n, "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (at >= 0 && (size_t)at < n) vsnprintf(msg + at, n - (size_t)at, fmt, ap);
    va_end(ap);
    return TTS_HIP_EINVAL;
}

// one row's length: lengths[b] in [1, N]
inline int audio_row_check(const char* who, int b, int len, int N, char* msg, size_t n) {
    if (len < 1 || len > N) return audio_refuse(msg, n, who, "lengths[%d] = %d outside [1, N = %d]", b, len, N);
    return TTS_HIP_OK;
}

// lens[b] = lengths[b] (NULL: N) for a batch of B rows of N samples, every one in [1, N]; *min_len = the shortest
inline int audio_rows_check(const char* who, int B, int N, const int32_t* lengths, std::vector<int>& lens, int* min_len, char* msg,
                            size_t n) {
    lens.assign(B, N);
    *min_len = N;
    if (lengths)
        for (int b = 0; b < B; ++b) {
            if (int rc = audio_row_check(who, b, lengths[b], N, msg, n)) return rc;
            lens[b] = lengths[b];
            *min_len = std::min(*min_len, lengths[b]);
        }
    return TTS_HIP_OK;
}

// `mem` of a synchronous entry point (an _async one has none: its callers pass TTS_HIP_MEM_DEVICE)
inline int audio_mem_check(const char* who, int mem, char* msg, size_t n) {
    if (mem != TTS_HIP_MEM_HOST && mem != TTS_HIP_MEM_DEVICE) return audio_refuse(msg, n, who, "bad mem kind %d", mem);
    return TTS_HIP_OK;
}

inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }
inline unsigned blocks(long long n, int t) { return (unsigned)((n + t - 1) / t); }

// A buffer cut into slices that each start on a 256-byte boundary: take() returns the slice's offset, `o` is the extent
struct Carve {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o += al256(bytes);
        return at;
    }
};

constexpr long long kAudioLim = (1ll << 31) - 65536;    // byte extent of any buffer a kernel or GEMM descriptor addresses
constexpr long long kAudioLim31 = 1ll << 31;            // the same for the kernels that index without a descriptor's slack

// ---------------------------------------------------------------------------------------------- reduce_noise (audio_proc.hip)
namespace rn {
constexpr int NFFT = 2048, HOP = 512, HALF = NFFT / 2, NBIN = NFFT / 2 + 1;
constexpr int NK = 2080;                     // 2 * 1025 DFT rows (real, imaginary) padded to a multiple of 32
}  // namespace rn

struct RnGeom {
    int Fr, NP, Frn, NQ;
    size_t off_info, off_pmax, off_thr, off_P, off_Q, off_S, off_Sn, off_T, off_mask, total;
};

inline RnGeom rn_geom(int B, int N, int noise_len) {
    using namespace rn;
    RnGeom g{};
    g.Fr = (N + 2560 + HOP - 1) / HOP;          // >= F_b = 1 + (L_b + 512) // 512 for every row; NP = Fr * 512 >= N + 2560
    g.NP = g.Fr * HOP;
    g.Frn = (noise_len + NFFT + HOP - 1) / HOP; // >= 1 + noise_len // 512
    g.NQ = g.Frn * HOP;
    Carve c;
    g.off_info = c.take((size_t)4 * B * 4);
    g.off_pmax = c.take((size_t)2 * B * 4);
    g.off_thr = c.take((size_t)B * NBIN * 4);
    g.off_P = c.take(((size_t)B * g.NP + NFFT) * 4);
    g.off_Q = c.take(((size_t)B * g.NQ + NFFT) * 4);
    g.off_S = c.take((size_t)B * g.Fr * NK * 4);
    g.off_Sn = c.take((size_t)B * g.Frn * NK * 4);
    g.off_T = c.take((size_t)B * g.Fr * NFFT * 4);
    g.off_mask = c.take((size_t)B * g.Fr * NBIN);
    g.total = c.o;
    return g;
}

// order: pointers / B / N, noise_len, lengths[b], the 31-bit limits, mem kind; fills `lens`
inline int rn_check(const char* who, const float* audio, int B, int N, const int32_t* lengths, int noise_len, const float* out,
                    int mem, std::vector<int>& lens, char* msg, size_t n) {
    using namespace rn;
    if (!audio || !out || B <= 0 || N <= 0) return audio_refuse(msg, n, who, "bad argument");
    if (noise_len < 1) return audio_refuse(msg, n, who, "noise_len = %d < 1", noise_len);
    int min_len;
    if (int rc = audio_rows_check(who, B, N, lengths, lens, &min_len, msg, n)) return rc;
    const RnGeom g = rn_geom(B, N, noise_len);
    const long long biggest = std::max({(long long)B * g.Fr * NK * 4, (long long)B * g.NP * 4 + NFFT * 4,
                                        (long long)B * g.Frn * NK * 4, (long long)B * g.NQ * 4 + NFFT * 4,
                                        (long long)B * N * 4, (long long)B * noise_len * 4});
    if (biggest >= kAudioLim || g.Fr > 65535)
        return audio_refuse(msg, n, who, "B = %d x N = %d (noise_len %d) too large for 31-bit offsets", B, N, noise_len);
    return audio_mem_check(who, mem, msg, n);
}

// ---------------------------------------------------------------------------------------------- trim_silence (audio_proc.hip)
struct TrimGeom {
    int W, Wp;          // window taps 2 * (window_length // 2), and rounded up to 4
    int Cst;            // doubles between two rows of the convolution: max(N, W) + 1
    int min_len;
};

// order: pointers / B / N, window_length, mode, threshold / margins, mem kind, lengths[b], the 31-bit limits; fills `lens`.
// have_out: the entry point's own outputs are there (start and end, or the probe's conv)
inline int trim_check(const char* who, const float* audio, bool have_out, int B, int N, const int32_t* lengths, int window_length,
                      double threshold, double add_start, double add_end, int mode, int mem, std::vector<int>& lens, TrimGeom* g,
                      char* msg, size_t n) {
    if (!audio || !have_out || B <= 0 || N <= 0) return audio_refuse(msg, n, who, "bad argument");
    if (window_length < 2) return audio_refuse(msg, n, who, "window_length = %d < 2", window_length);
    if (mode < 0 || mode > 2) return audio_refuse(msg, n, who, "mode %d not 0 (start_end), 1 (start) or 2 (end)", mode);
    if (!std::isfinite(threshold) || !std::isfinite(add_start) || !std::isfinite(add_end) ||
        add_start < 0 || add_end < 0 || (double)window_length * add_start > 1e9 || (double)window_length * add_end > 1e9)
        return audio_refuse(msg, n, who, "threshold / margins must be finite, margins >= 0 and not oversized");
    if (int rc = audio_mem_check(who, mem, msg, n)) return rc;
    const int h = window_length / 2;
    g->W = 2 * h;
    g->Wp = (g->W + 3) / 4 * 4;
    if (int rc = audio_rows_check(who, B, N, lengths, lens, &g->min_len, msg, n)) return rc;
    g->Cst = std::max(N, g->W) + 1;
    if ((long long)B * g->Cst * 8 >= kAudioLim || (long long)B * N * 4 >= kAudioLim)
        return audio_refuse(msg, n, who, "B = %d x N = %d too large for 31-bit offsets", B, N);
    return TTS_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- resample (resample.hip)
constexpr int RS_MAX_LEN = 1 << 24;                // samples per row, in and out

inline int ilog2(long long v) {
    int l = 0;
    while ((1ll << l) < v) ++l;
    return l;
}

struct RsLens {
    int logf, logi;             // log2 of the forward / inverse Bluestein lengths
};

// L_fwd >= N + N//2, L_inv >= 2M - 1, both at least 64
inline RsLens rs_lens(int n, int m) { return {std::max(6, ilog2((long long)n + n / 2)), std::max(6, ilog2(2ll * m - 1))}; }

inline int rs_out_len(int n, int rate, int target_rate) { return (int)((double)n / rate * target_rate); }

// order: pointers / B / N, rates, N and M against 2^24, M < 1, M against int(N / rate * target_rate), the 31-bit limits,
// lengths[b] (and what it resamples to), mem kind; fills the row lengths in and out
inline int rs_check(const char* who, const float* audio, int B, int N, const int32_t* lengths, int rate, int target_rate,
                    const float* out, int M, int mem, std::vector<int>& lens, std::vector<int>& mlens, char* msg, size_t n) {
    if (!audio || !out || B <= 0 || N <= 0) return audio_refuse(msg, n, who, "bad argument");
    if (rate <= 0 || target_rate <= 0)
        return audio_refuse(msg, n, who, "rates must be > 0 (rate %d, target_rate %d)", rate, target_rate);
    if (N > RS_MAX_LEN) return audio_refuse(msg, n, who, "N = %d > 2^24 samples per row", N);
    const double md = (double)N / rate * target_rate;
    if (!(md < (double)RS_MAX_LEN + 1))
        return audio_refuse(msg, n, who, "%d samples at %d -> %d Hz give more than 2^24 samples per row", N, rate, target_rate);
    const int want = rs_out_len(N, rate, target_rate);
    if (want < 1) return audio_refuse(msg, n, who, "%d samples at %d -> %d Hz give M = %d < 1", N, rate, target_rate, want);
    if (M != want) return audio_refuse(msg, n, who, "M = %d, but int(%d / %d * %d) = %d", M, N, rate, target_rate, want);
    if ((long long)B * M * 4 >= kAudioLim31 || (long long)B * N * 4 >= kAudioLim31)
        return audio_refuse(msg, n, who, "B = %d x N = %d (M %d) too large for 31-bit offsets", B, N, M);
    lens.assign(B, N);
    mlens.assign(B, M);
    if (lengths)                                            // row by row: a row's own two refusals before the next row's
        for (int b = 0; b < B; ++b) {
            if (int rc = audio_row_check(who, b, lengths[b], N, msg, n)) return rc;
            lens[b] = lengths[b];
            mlens[b] = rs_out_len(lens[b], rate, target_rate);
            if (mlens[b] < 1)
                return audio_refuse(msg, n, who, "lengths[%d] = %d resamples to %d < 1 samples", b, lens[b], mlens[b]);
        }
    return audio_mem_check(who, mem, msg, n);
}

constexpr int RS_FFT_MIN_LOG = 6, RS_FFT_MAX_LOG = 25;     // transform lengths rs_lens can ask for (N, M <= 2^24)

// tts_hip_resample_fft_probe -- order: pointers, logL, lines, the 31-bit limit of the staged lines
inline int rs_fft_probe_check(const char* who, const float* in, int lines, int logL, const float* out, char* msg, size_t n) {
    if (!in || !out) return audio_refuse(msg, n, who, "bad argument");
    if (logL < RS_FFT_MIN_LOG || logL > RS_FFT_MAX_LOG)
        return audio_refuse(msg, n, who, "logL = %d outside [%d, %d]", logL, RS_FFT_MIN_LOG, RS_FFT_MAX_LOG);
    if (lines < 1) return audio_refuse(msg, n, who, "lines = %d < 1", lines);
    if (((long long)lines << logL) * 8 >= kAudioLim31)
        return audio_refuse(msg, n, who, "lines = %d x 2^%d points too large for 31-bit offsets", lines, logL);
    return TTS_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- remove_silence (silence.hip)
constexpr int SIL_TILE = 2048;               // samples per workgroup of the tile kernels (256 threads x 8 consecutive)

struct SilCall {
    int B, N, method, mode, rate, bs, rb;
    double threshold, min_silence, mvt;
    std::vector<int> lens;
    int w = 0;                  // mean-window taps
    int NT = 0, NB = 0, cap = 1;
    size_t off_info, off_mask, off_cnt, off_off, off_n, off_cut, off_d0, off_d1, off_flag, off_si, off_sj, off_tsum, off_toff,
        off_P, off_tot, total;
};

// order: pointers / B / N, method, mode, mode 3 without rms, rate, the size limits, lengths[b], threshold, the rms settings,
// min_silence, the mean-window settings (a row shorter than the window among them), out overlapping audio, mem kind
inline int sil_check(const char* who, const float* audio, int B, int N, const int32_t* lengths, int method, int mode, int rate,
                     double threshold, double min_silence, int block_size, int replace_by, double min_voice_time, const float* out,
                     const int32_t* out_lengths, int mem, SilCall& c, char* msg, size_t n) {
    if (!audio || !out || !out_lengths || B <= 0 || N <= 0) return audio_refuse(msg, n, who, "bad argument");
    if (method < TTS_HIP_SILENCE_RMS || method > TTS_HIP_SILENCE_MEAN_WINDOW)
        return audio_refuse(msg, n, who, "method %d not 0 (rms), 1 (threshold) or 2 (mean-window)", method);
    if (mode < 0 || mode > 3)
        return audio_refuse(msg, n, who, "mode %d not 0 (start_end), 1 (start), 2 (end) or 3 (remove)", mode);
    if (mode == 3 && method != TTS_HIP_SILENCE_RMS)
        return audio_refuse(msg, n, who, "mode 3 (remove) belongs to the rms method (got method %d)", method);
    if (rate <= 0) return audio_refuse(msg, n, who, "rate = %d <= 0", rate);
    if (B > 65535 || N > (1 << 24) || (long long)B * N * 4 >= kAudioLim31)   // B is a grid dimension of every kernel
        return audio_refuse(msg, n, who, "B = %d x N = %d too large (B <= 65535, N <= 2^24, B * N * 4 < 2^31)", B, N);
    int min_len;
    if (int rc = audio_rows_check(who, B, N, lengths, c.lens, &min_len, msg, n)) return rc;
    const bool rms = method == TTS_HIP_SILENCE_RMS, mw = method == TTS_HIP_SILENCE_MEAN_WINDOW;
    if (!std::isfinite(threshold) || (!rms && threshold < 0))
        return audio_refuse(msg, n, who, "threshold = %g must be finite%s", threshold, rms ? "" : " and >= 0");
    if (rms) {
        if (block_size < 1) return audio_refuse(msg, n, who, "block_size = %d < 1", block_size);
        if (replace_by < 0) return audio_refuse(msg, n, who, "replace_by = %d < 0", replace_by);
        if (!std::isfinite(min_voice_time) || min_voice_time < 0)
            return audio_refuse(msg, n, who, "min_voice_time = %g must be finite and >= 0", min_voice_time);
    }
    if ((rms || mw) && (!std::isfinite(min_silence) || min_silence < 0))
        return audio_refuse(msg, n, who, "min_silence = %g must be finite and >= 0", min_silence);
    if (mw) {
        if (threshold <= 0) return audio_refuse(msg, n, who, "threshold = %g <= 0 (mean-window)", threshold);
        const double wd = min_silence * (double)rate;
        if (wd < 1.0) return audio_refuse(msg, n, who, "window w = (int)(min_silence * rate) = %d < 1", (int)wd);
        if (std::floor(wd) > (double)min_len)           // also keeps (int)wd in range
            return audio_refuse(msg, n, who, "a row of L = %d samples is shorter than the window w = %.0f", min_len, std::floor(wd));
        c.w = (int)wd;
        if (min_len < c.w)
            return audio_refuse(msg, n, who, "a row of L = %d samples is shorter than the window w = %d", min_len, c.w);
    }
    const char *a0 = (const char*)audio, *o0 = (const char*)out;
    const size_t bytes = (size_t)B * N * 4;
    if (a0 < o0 + bytes && o0 < a0 + bytes) return audio_refuse(msg, n, who, "out overlaps audio");
    if (int rc = audio_mem_check(who, mem, msg, n)) return rc;

    c.B = B;
    c.N = N;
    c.method = method;
    c.mode = mode;
    c.rate = rate;
    c.bs = block_size;
    c.rb = replace_by;
    c.threshold = threshold;
    c.min_silence = min_silence;
    c.mvt = min_voice_time;
    c.NT = (N + SIL_TILE - 1) / SIL_TILE;
    if (rms) {
        // silences per row: each holds >= q blocks (q * bt >= min_silence, taken one short against rounding) and a loud
        // block parts it from the next
        c.NB = (int)(((long long)N + c.bs - 1) / c.bs);
        const double per = min_silence / ((double)c.bs / (double)rate);
        const long long q = std::max<long long>(1, (per < 1e9 ? (long long)per : 1000000000ll) - 1);
        c.cap = (int)(c.NB / (q + 1) + 1);
    }
    Carve ws;
    c.off_info = ws.take((size_t)B * 4);
    c.off_mask = ws.take((size_t)B * N);
    c.off_cnt = ws.take((size_t)B * c.NT * 4);
    c.off_off = ws.take((size_t)B * c.NT * 4);
    c.off_n = ws.take((size_t)B * 4);
    c.off_cut = ws.take((size_t)B * 4);
    c.off_d0 = ws.take((size_t)B * c.cap * 4);
    c.off_d1 = ws.take((size_t)B * c.cap * 4);
    c.off_flag = ws.take(rms ? (size_t)B * c.NB : 0);
    c.off_si = ws.take(rms ? (size_t)B * c.cap * 4 : 0);
    c.off_sj = ws.take(rms ? (size_t)B * c.cap * 4 : 0);
    c.off_tsum = ws.take(mw ? (size_t)B * c.NT * 8 : 0);
    c.off_toff = ws.take(mw ? (size_t)B * c.NT * 8 : 0);
    c.off_P = ws.take(mw ? (size_t)B * ((size_t)N + 1) * 8 : 0);
    c.off_tot = ws.take(mw ? (size_t)B * 8 : 0);
    c.total = ws.o;
    return TTS_HIP_OK;
}

// The stages sil_run can stop at (tts_hip_remove_silence_probe): a row of the stage holds `width` elements of `elem` bytes
enum { SIL_FLAGS = 0, SIL_INTERVALS, SIL_MASK, SIL_TILE_OFFSETS, SIL_PREFIX, SIL_STAGES };

struct SilStage {
    int width, elem;
};

// order: width, sil_check's own but for the overlap (`out` NULL asks for the width alone and is no refusal), `what` out of
// range, a stage the method does not have, out overlapping audio; fills `c` and `s`
inline int sil_probe_check(const char* who, const float* audio, int B, int N, const int32_t* lengths, int method, int mode, int rate,
                           double threshold, double min_silence, int block_size, int replace_by, double min_voice_time, int what,
                           const void* out, const int32_t* width, int mem, SilCall& c, SilStage* s, char* msg, size_t n) {
    if (!width) return audio_refuse(msg, n, who, "bad argument");
    // the probe's out has its stage's extent, not the call's B * N floats: sil_check gets the address behind audio in its
    // place (compared with audio, never read), and the probe's own out is compared below
    const float* behind = audio && B > 0 && N > 0 ? audio + (size_t)B * N : audio;
    if (int rc = sil_check(who, audio, B, N, lengths, method, mode, rate, threshold, min_silence, block_size, replace_by,
                           min_voice_time, behind, width, mem, c, msg, n))
        return rc;
    if (what < 0 || what >= SIL_STAGES) return audio_refuse(msg, n, who, "no stage %d (0 .. %d)", what, SIL_STAGES - 1);
    const bool rms = method == TTS_HIP_SILENCE_RMS, mw = method == TTS_HIP_SILENCE_MEAN_WINDOW;
    if ((what == SIL_FLAGS && !rms) || (what == SIL_INTERVALS && mw) || (what == SIL_PREFIX && !mw))
        return audio_refuse(msg, n, who, "method %d has no stage %d", method, what);
    switch (what) {
        case SIL_FLAGS: *s = {c.NB, 1}; break;
        case SIL_INTERVALS: *s = {2 + 2 * c.cap, 4}; break;
        case SIL_MASK: *s = {N, 1}; break;
        case SIL_TILE_OFFSETS: *s = {c.NT, 4}; break;
        default: *s = {N + 1, 8}; break;
    }
    const char *a0 = (const char*)audio, *o0 = (const char*)out;
    const size_t a_bytes = (size_t)B * N * 4, o_bytes = (size_t)B * s->width * s->elem;
    if (out && a0 < o0 + o_bytes && o0 < a0 + a_bytes) return audio_refuse(msg, n, who, "out overlaps audio");
    return TTS_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- mel plans (mel_stft.hip)
// A plan (tts_hip_mel_fn) is a checked tts_hip_mel_config plus the operand widths its tables are padded to; a call derives
// its frame counts and its one workspace from the plan, B, N and lengths.
struct MelPlan {
    int kind, norm, sr, nmel, fl, hop, wl;
    double fmin, fmax, pre;
    int half, cut, lpad;        // filter_length // 2, the bins filter_length // 2 + 1, (filter_length - win_length) // 2
    int K4, Kpad;               // filter_length rounded up to 4 (what a strided frame reads) and to 32 (the K of the tables)
    int NB, MAGK;               // 2 * cut and cut rounded up to 32: DFT rows / magnitude columns
    bool gather;                // hop % 4 != 0: frames are materialised [B * Fr][Kpad] instead of read as strided rows
};

inline int up_to(int v, int m) { return (v + m - 1) / m * m; }

// create -- order: pointers, kind / normalize_mode, sampling_rate, filter_length, win_length, hop_length, n_mel_channels,
// mel_fmin / mel_fmax, pre_emph, window values; fills `p`
inline int mel_cfg_check(const char* who, const tts_hip_mel_config* c, const double* window, bool have_out, MelPlan* p, char* msg,
                         size_t n) {
    if (!c || !have_out) return audio_refuse(msg, n, who, "bad argument");
    if (c->kind != TTS_HIP_MEL_TACOTRON && c->kind != TTS_HIP_MEL_WHISPER)
        return audio_refuse(msg, n, who, "kind %d not 0 (tacotron) or 1 (whisper)", c->kind);
    if (c->normalize_mode < TTS_HIP_MEL_NORM_NONE || c->normalize_mode > TTS_HIP_MEL_NORM_ALL_FEATURE)
        return audio_refuse(msg, n, who, "normalize_mode %d not 0 (none), 1 (per_feature) or 2 (all_feature)", c->normalize_mode);
    if (c->sampling_rate < 1) return audio_refuse(msg, n, who, "sampling_rate = %d < 1", c->sampling_rate);
    if (c->filter_length < 2 || c->filter_length > 4096)
        return audio_refuse(msg, n, who, "filter_length = %d outside [2, 4096]", c->filter_length);
    if (c->win_length < 1 || c->win_length > c->filter_length)
        return audio_refuse(msg, n, who, "win_length = %d outside [1, filter_length = %d]", c->win_length, c->filter_length);
    if (c->hop_length < 1) return audio_refuse(msg, n, who, "hop_length = %d < 1", c->hop_length);
    if (c->n_mel_channels < 1 || c->n_mel_channels > 1024)
        return audio_refuse(msg, n, who, "n_mel_channels = %d outside [1, 1024]", c->n_mel_channels);
    if (!(c->mel_fmin >= 0 && c->mel_fmin < c->mel_fmax && c->mel_fmax <= c->sampling_rate / 2.0))
        return audio_refuse(msg, n, who, "need 0 <= mel_fmin = %g < mel_fmax = %g <= sampling_rate / 2 = %g", c->mel_fmin,
                            c->mel_fmax, c->sampling_rate / 2.0);
    if (!std::isfinite(c->pre_emph) || c->pre_emph < 0)
        return audio_refuse(msg, n, who, "pre_emph = %g must be finite and >= 0", c->pre_emph);
    if (window)
        for (int i = 0; i < c->win_length; ++i)
            if (!std::isfinite(window[i])) return audio_refuse(msg, n, who, "window[%d] is not finite", i);
    p->kind = c->kind, p->norm = c->normalize_mode, p->sr = c->sampling_rate, p->nmel = c->n_mel_channels;
    p->fl = c->filter_length, p->hop = c->hop_length, p->wl = c->win_length;
    p->fmin = c->mel_fmin, p->fmax = c->mel_fmax, p->pre = c->pre_emph;
    p->half = p->fl / 2, p->cut = p->fl / 2 + 1, p->lpad = (p->fl - p->wl) / 2;
    p->K4 = up_to(p->fl, 4), p->Kpad = up_to(p->fl, 32);
    p->NB = up_to(2 * p->cut, 32), p->MAGK = up_to(p->cut, 32);
    p->gather = p->hop % 4 != 0;
    return TTS_HIP_OK;
}

// frames the DFT gives a row of n samples (before Whisper drops the last): L' = max(n, win_length) zero-padded samples,
// reflect-padded by filter_length // 2 on each side.  0 when reflect cannot pad the row (L' <= filter_length // 2) or n < 1
inline int mel_dft_frames(const MelPlan& p, int n) {
    if (n < 1) return 0;
    const long long lp = std::max(n, p.wl);
    if (lp <= p.half) return 0;
    return (int)((lp + 2 * p.half - p.fl) / p.hop + 1);
}

// frames of the result; < 0 if the row is refused
inline int mel_out_frames(const MelPlan& p, int n) {
    const int f = mel_dft_frames(p, n);
    if (f < 1) return -1;
    if (p.kind == TTS_HIP_MEL_WHISPER) return f < 2 ? -1 : f - 1;
    return f;
}

// One workspace per call.  Named buffers (each below kAudioLim bytes): `padded` [B][NP] the zero-padded, pre-emphasised,
// reflect-padded rows, PW = max(N, win_length) + 2 * (filter_length // 2) of them logical and NP = PW + K4 - filter_length
// rounded up to 4 stored; `gathered` [B * Fr][Kpad] (gather plans only); `spectrum` [B * Fr][NB]; `magnitude`
// [B * Fr][MAGK]; `linear` [B * Fr][n_mel] (Whisper only: the result has one frame less per row); and the caller's audio
// [B][N] and mel [B][Fout][n_mel]
struct MelGeom {
    int Fr, Fout, PW, NP;
    std::vector<int> lens, fout;            // per row: samples, frames of the result
    size_t off_info, off_rowmax, off_padded, off_gathered, off_spectrum, off_magnitude, off_linear, total;
};

// The frame slots, the padded rows and the one workspace of a call on B rows of N samples -> the bytes of its largest buffer;
// the widths and offsets of `g` are filled where that lies below kAudioLim
inline long long mel_geom_layout(const MelPlan& p, int B, int N, MelGeom* g) {
    g->Fr = mel_dft_frames(p, N);
    g->Fout = mel_out_frames(p, N);
    const long long PW = (long long)std::max(N, p.wl) + 2 * p.half, NP = (PW + p.K4 - p.fl + 3) / 4 * 4;
    const long long rows = (long long)B * g->Fr;
    const long long biggest = std::max({(long long)B * NP * 4 + 256, p.gather ? rows * p.Kpad * 4 : 0, rows * p.NB * 4,
                                        rows * p.MAGK * 4, rows * p.nmel * 4, (long long)B * N * 4});
    if (biggest >= kAudioLim) return biggest;
    g->PW = (int)PW, g->NP = (int)NP;
    Carve c;
    g->off_info = c.take((size_t)2 * B * 4);
    g->off_rowmax = c.take((size_t)B * 4);
    g->off_padded = c.take((size_t)B * NP * 4 + 256);
    g->off_gathered = c.take(p.gather ? (size_t)rows * p.Kpad * 4 : 0);
    g->off_spectrum = c.take((size_t)rows * p.NB * 4);
    g->off_magnitude = c.take((size_t)rows * p.MAGK * 4);
    g->off_linear = c.take(p.kind == TTS_HIP_MEL_WHISPER ? (size_t)rows * p.nmel * 4 : 0);
    g->total = c.o;
    return biggest;
}

// run -- order: pointers / B / N, lengths[b], a row reflect cannot pad, a Whisper row of one frame, the 31-bit limits, mem
// kind; fills `g`
inline int mel_call_check(const char* who, const MelPlan* p, const float* audio, int B, int N, const int32_t* lengths,
                          const float* out, int mem, MelGeom* g, char* msg, size_t n) {
    if (!p || !audio || !out || B < 1 || N < 1) return audio_refuse(msg, n, who, "bad argument");
    int min_len;
    if (int rc = audio_rows_check(who, B, N, lengths, g->lens, &min_len, msg, n)) return rc;
    g->fout.assign(B, 0);
    for (int b = 0; b < B; ++b)
        if (mel_dft_frames(*p, g->lens[b]) < 1)
            return audio_refuse(msg, n, who, "row %d: max(L = %d, win_length = %d) samples are not more than filter_length // 2 = %d",
                                b, g->lens[b], p->wl, p->half);
    for (int b = 0; b < B; ++b) {
        g->fout[b] = mel_out_frames(*p, g->lens[b]);
        if (g->fout[b] < 1) return audio_refuse(msg, n, who, "row %d: L = %d samples give one frame, Whisper drops the last", b, g->lens[b]);
    }
    if (mel_geom_layout(*p, B, N, g) >= kAudioLim || B > 65535)
        return audio_refuse(msg, n, who, "B = %d x N = %d too large for 31-bit offsets (B <= 65535)", B, N);
    return audio_mem_check(who, mem, msg, n);
}

// ---------------------------------------------------------------------------------------------- STFT inverse, Griffin-Lim (stft_inv.hip)
// The Slaney filterbank of a plan in double, [n_mel][cut] (librosa.filters.mel defaults; stft.py:65-72): what plan_build
// rounds to the fp32 table, and what the mel inversion below starts from.
inline double mel_hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
inline double mel_mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}
inline void mel_filterbank(const MelPlan& p, std::vector<double>& W) {
    const double sr = p.sr;
    std::vector<double> mel_f(p.nmel + 2);
    const double m0 = mel_hz_to_mel(p.fmin), m1 = mel_hz_to_mel(p.fmax);
    for (int i = 0; i < p.nmel + 2; ++i) mel_f[i] = mel_mel_to_hz(m0 + (m1 - m0) * i / (p.nmel + 1));
    W.assign((size_t)p.nmel * p.cut, 0.0);
    for (int i = 0; i < p.nmel; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int c = 0; c < p.cut; ++c) {
            const double fr = (sr / 2.0) * c / (p.cut - 1);
            const double lower = (fr - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - fr) / (mel_f[i + 2] - mel_f[i + 1]);
            W[(size_t)i * p.cut + c] = std::fmax(0.0, std::fmin(lower, upper)) * enorm;
        }
    }
}

// Minv [n_mel][cut] = (W W^T)^-1 W, the transpose of the minimum-norm inverse W^T (W W^T)^-1 of the plan's filterbank:
// spectrum = mel . Minv.  W W^T is factored by Cholesky in double; false when it is not positive definite (a channel
// without a bin makes a zero row).
inline bool mel_min_norm_inverse(const MelPlan& p, std::vector<double>& Minv) {
    std::vector<double> W;
    mel_filterbank(p, W);
    const int n = p.nmel, c = p.cut;
    std::vector<double> G((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = 0; k < c; ++k) s += W[(size_t)i * c + k] * W[(size_t)j * c + k];
            G[(size_t)i * n + j] = s;
        }
    double scale = 0.0;
    for (int i = 0; i < n; ++i) scale = std::max(scale, G[(size_t)i * n + i]);
    for (int j = 0; j < n; ++j) {                               // G = L L^T in place (lower triangle)
        double d = G[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= G[(size_t)j * n + k] * G[(size_t)j * n + k];
        if (!(d > 1e-13 * scale)) return false;
        const double l = std::sqrt(d);
        G[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double s = G[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= G[(size_t)i * n + k] * G[(size_t)j * n + k];
            G[(size_t)i * n + j] = s / l;
        }
    }
    Minv = W;                                                   // solve L L^T X = W column by column of W
    for (int k = 0; k < c; ++k) {
        for (int i = 0; i < n; ++i) {
            double s = Minv[(size_t)i * c + k];
            for (int j = 0; j < i; ++j) s -= G[(size_t)i * n + j] * Minv[(size_t)j * c + k];
            Minv[(size_t)i * c + k] = s / G[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double s = Minv[(size_t)i * c + k];
            for (int j = i + 1; j < n; ++j) s -= G[(size_t)j * n + i] * Minv[(size_t)j * c + k];
            Minv[(size_t)i * c + k] = s / G[(size_t)i * n + i];
        }
    }
    return true;
}

// samples `frames` frames overlap-add to, the filter_length // 2 at each end dropped; < 0 for frames < 1
inline long long stft_samples(const MelPlan& p, int frames) {
    return frames < 1 ? -1 : (long long)p.hop * (frames - 1) + p.fl - 2 * p.half;
}

enum { GL_TARGET = 0, GL_OPERAND, GL_FRAMES, GL_SIGNAL, GL_SPECTRUM, GL_PHASOR, GL_STAGES };

// One workspace per call.  `operand` [B * F][NB] the GEMM's A (real parts at columns 0 .. cut - 1, imaginary parts at
// cut .. 2 cut - 1, zero beyond and in the frames behind a row's own); `tprev` and `phasor` the same shape; `target`
// [B * F][cut]; `tframes` [B * F][filter_length]; `padded` [B][NP] the reflect-padded rows, PW = hop (F - 1) + filter_length
// of them logical; `gathered` (gather plans) and `spectrum` as MelGeom's; `expmel` [B * F][EK] and `minv` [cut][EK] (log-mel input).
struct GlGeom {
    int B, F, PW, NP, EK;
    long long Sout;                         // output stride F * hop
    std::vector<int> frames;                // per row
    size_t off_info, off_target, off_operand, off_tprev, off_phasor, off_tframes, off_padded, off_gathered, off_spectrum,
        off_expmel, off_minv, total;
};

// The one workspace of a call on B rows of F frame slots (kind < 0: the inverse alone; what: the probed stage or -1) -> the
// bytes of its largest buffer, the caller's planes [B * F][C] and audio [B][F * hop] among them; the widths and offsets of
// `g` are filled where that lies below kAudioLim
inline long long gl_geom_layout(const MelPlan& p, int B, int F, int C, int kind, int what, GlGeom* g) {
    const bool gl = kind >= 0;
    const long long PW = (long long)p.hop * (F - 1) + p.fl, NP = (PW + p.K4 - p.fl + 3) / 4 * 4;
    const long long rows = (long long)B * F, EK = up_to(p.nmel, 32);
    const long long biggest = std::max({(long long)B * NP * 4 + 256, rows * p.Kpad * 4, rows * p.NB * 4, rows * p.fl * 4,
                                        rows * p.hop * 4, rows * C * 4, kind == 1 ? rows * EK * 4 : 0});
    if (biggest >= kAudioLim) return biggest;
    g->B = B, g->F = F, g->PW = (int)PW, g->NP = (int)NP, g->EK = (int)EK, g->Sout = (long long)F * p.hop;
    Carve c;
    g->off_info = c.take((size_t)B * 4);
    g->off_target = c.take(gl ? (size_t)rows * p.cut * 4 : 0);
    g->off_operand = c.take((size_t)rows * p.NB * 4);
    g->off_tprev = c.take(gl ? (size_t)rows * p.NB * 4 : 0);
    g->off_phasor = c.take(what == GL_PHASOR ? (size_t)rows * p.NB * 4 : 0);
    g->off_tframes = c.take((size_t)rows * p.fl * 4);
    g->off_padded = c.take(gl ? (size_t)B * NP * 4 + 256 : 0);
    g->off_gathered = c.take(gl && p.gather ? (size_t)rows * p.Kpad * 4 : 0);
    g->off_spectrum = c.take(gl ? (size_t)rows * p.NB * 4 : 0);
    g->off_expmel = c.take(kind == 1 ? (size_t)rows * EK * 4 : 0);
    g->off_minv = c.take(kind == 1 ? (size_t)p.cut * EK * 4 : 0);       // the caller's own Minv, transposed and padded
    g->total = c.o;
    return biggest;
}

// What tts_hip_stft_inverse (kind < 0: two planes of C = cut) and tts_hip_griffin_lim[_probe] (kind 0 / 1) may be refused
// for -- order: pointers, B / F, frames[b], C, n_iters, momentum, a Whisper plan, pre_emph, normalisation (kind 1), a row
// the reflect cannot pad, the 31-bit limits, mem kind, what / k (probe: what >= 0); fills `g`
inline int stft_inv_check(const char* who, const MelPlan* p, const void* in0, const void* in1, const void* out, int B, int F, int C,
                          const int32_t* frames, int kind, int n_iters, double momentum, int mem, int what, int k, GlGeom* g,
                          char* msg, size_t n) {
    const bool gl = kind >= 0;
    if (!p || !in0 || !in1 || !out) return audio_refuse(msg, n, who, "bad argument (NULL pointer)");
    if (B < 1 || F < 1) return audio_refuse(msg, n, who, "B = %d, F = %d: both must be >= 1", B, F);
    g->frames.assign(B, F);
    if (frames)
        for (int b = 0; b < B; ++b) {
            if (frames[b] < 1 || frames[b] > F) return audio_refuse(msg, n, who, "frames[%d] = %d outside [1, F = %d]", b, frames[b], F);
            g->frames[b] = frames[b];
        }
    if (kind > 1) return audio_refuse(msg, n, who, "input_kind %d not 0 (magnitude) or 1 (log-mel)", kind);
    const int want = kind == 1 ? p->nmel : p->cut;
    if (C != want) return audio_refuse(msg, n, who, "C = %d, but the plan's %s is %d", C, kind == 1 ? "n_mel_channels" : "bins", want);
    if (gl && n_iters < 0) return audio_refuse(msg, n, who, "n_iters = %d < 0", n_iters);
    if (gl && !(std::isfinite(momentum) && momentum >= 0 && momentum < 1))
        return audio_refuse(msg, n, who, "momentum = %g outside [0, 1)", momentum);
    if (p->kind != TTS_HIP_MEL_TACOTRON) return audio_refuse(msg, n, who, "a Whisper plan has no inverse");
    if (gl && p->pre > 0) return audio_refuse(msg, n, who, "pre_emph = %g > 0 cannot be inverted", p->pre);
    if (kind == 1 && p->norm != TTS_HIP_MEL_NORM_NONE)
        return audio_refuse(msg, n, who, "normalize_mode %d is not invertible (log-mel input)", p->norm);
    if (gl)
        for (int b = 0; b < B; ++b)
            if (stft_samples(*p, g->frames[b]) <= p->half)
                return audio_refuse(msg, n, who, "row %d: %d frames give %lld samples, not more than filter_length // 2 = %d", b,
                                    g->frames[b], stft_samples(*p, g->frames[b]), p->half);
    if (gl_geom_layout(*p, B, F, C, kind, what, g) >= kAudioLim || B > 65535)
        return audio_refuse(msg, n, who, "B = %d x F = %d too large for 31-bit offsets (B <= 65535)", B, F);
    if (int rc = audio_mem_check(who, mem, msg, n)) return rc;
    if (what >= 0) {
        if (what >= GL_STAGES) return audio_refuse(msg, n, who, "no stage %d (0 .. %d)", what, GL_STAGES - 1);
        if (k < 0 || k > n_iters) return audio_refuse(msg, n, who, "k = %d outside [0, n_iters = %d]", k, n_iters);
        if (what >= GL_SPECTRUM && k == n_iters)
            return audio_refuse(msg, n, who, "iteration k = n_iters = %d ends at its signal: no stage %d there", k, what);
    }
    return TTS_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- denoiser (stft_inv.hip)
enum { DN_SPECTRUM = 0, DN_OPERAND, DN_FRAMES, DN_STAGES };

// A denoise call is a transform and an inverse on the same frame slots: `fwd` is the transform's geometry (lens, fout = the
// frames the plan gives each row, its workspace in e->stft.ws), `inv` the inverse's on F = fwd.Fr frame slots (frames = fout,
// its workspace in e->stft.inv_ws); row b of the result holds keep[b] = min(lens[b], stft_samples(frames[b])) samples
struct DnGeom {
    MelGeom fwd;
    GlGeom inv;
    std::vector<int> keep;
};

// What tts_hip_denoise[_async, _probe] may be refused for -- order: pointers / B / N, lengths[b], a row reflect cannot pad,
// a Whisper plan, bias NULL, strength not finite or negative, the 31-bit limits (of either workspace and of audio [B][N]),
// mem kind, what (probe: what >= 0; the call itself: -1); fills `g`
inline int denoise_check(const char* who, const MelPlan* p, const float* audio, int B, int N, const int32_t* lengths, const float* bias,
                         double strength, const float* out, int mem, int what, DnGeom* g, char* msg, size_t n) {
    if (!p || !audio || !out || B < 1 || N < 1) return audio_refuse(msg, n, who, "bad argument");
    int min_len;
    if (int rc = audio_rows_check(who, B, N, lengths, g->fwd.lens, &min_len, msg, n)) return rc;
    for (int b = 0; b < B; ++b)
        if (mel_dft_frames(*p, g->fwd.lens[b]) < 1)
            return audio_refuse(msg, n, who, "row %d: max(L = %d, win_length = %d) samples are not more than filter_length // 2 = %d",
                                b, g->fwd.lens[b], p->wl, p->half);
    if (p->kind != TTS_HIP_MEL_TACOTRON) return audio_refuse(msg, n, who, "refused for a Whisper plan");
    if (!bias) return audio_refuse(msg, n, who, "bias is NULL");
    if (!(std::isfinite(strength) && strength >= 0)) return audio_refuse(msg, n, who, "strength = %g must be finite and >= 0", strength);
    if (B > 65535 || mel_geom_layout(*p, B, N, &g->fwd) >= kAudioLim ||
        gl_geom_layout(*p, B, g->fwd.Fr, p->cut, -1, -1, &g->inv) >= kAudioLim)
        return audio_refuse(msg, n, who, "B = %d x N = %d too large for 31-bit offsets (B <= 65535)", B, N);
    if (int rc = audio_mem_check(who, mem, msg, n)) return rc;
    if (what >= DN_STAGES) return audio_refuse(msg, n, who, "no stage %d (0 .. %d)", what, DN_STAGES - 1);
    g->fwd.fout.resize(B);
    g->keep.resize(B);
    for (int b = 0; b < B; ++b) {
        g->fwd.fout[b] = mel_dft_frames(*p, g->fwd.lens[b]);
        g->keep[b] = (int)std::min<long long>(g->fwd.lens[b], stft_samples(*p, g->fwd.fout[b]));
    }
    g->inv.frames = g->fwd.fout;
    return TTS_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- time stretch (stft_inv.hip)
enum { TS_SPECTRUM = 0, TS_MAGNITUDE, TS_OWNER, TS_OPERAND, TS_FRAMES, TS_STAGES };
constexpr double kTsRateMin = 0.25, kTsRateMax = 4.0;

inline bool ts_rate_ok(double r) { return std::isfinite(r) && r >= kTsRateMin && r <= kTsRateMax; }

// output frames of F analysis frames at rate r: the smallest T with (double)T * r >= F (the quotient may round either way)
inline int ts_out_frames(int F, double r) {
    long long T = (long long)std::ceil((double)F / r);
    while (T > 1 && (double)(T - 1) * r >= (double)F) --T;
    while ((double)T * r < (double)F) ++T;
    return (int)T;
}

// output samples of a row of n samples at rate r: llrint(n / r), ties to even
inline long long ts_out_samples(int n, double r) { return std::llrint((double)n / r); }

// frames / samples of a row under a plan; < 0 where time_stretch_check refuses the row or the plan
inline int ts_row_frames(const MelPlan& p, int n, double r) {
    if (p.kind != TTS_HIP_MEL_TACOTRON || p.pre > 0 || !ts_rate_ok(r) || mel_dft_frames(p, n) < 1) return -1;
    return ts_out_frames(mel_dft_frames(p, n), r);
}
inline long long ts_row_samples(const MelPlan& p, int n, double r) { return ts_row_frames(p, n, r) < 0 ? -1 : ts_out_samples(n, r); }

// A time-stretch call is a transform on the rows' own frames (`fwd`: lens, fout = F_b, its workspace in e->stft.ws), the
// vocoder between them, and an inverse on T = max_b T_b frame slots (`inv`: frames = T_b, its workspace in e->stft.inv_ws).
// Behind the inverse's own buffers that workspace holds the vocoder's: `rowinfo` [B] doubles rates, then [B] int32 S_b;
// `mag` m [B * T][cut] fp32; `owner` own [B * T][cut] int32 (-1: the frame has no peak); `adv` A[t-1][own[t][k]] and
// `rel` R[t][k], both [B * T][cut][2] fp32 (re, im).  inv.total covers them.  Row b of the result holds
// keep[b] = min(S_b, stft_samples(T_b)) samples of the inverse, zeros up to M = max_b S_b.
struct TsGeom {
    MelGeom fwd;
    GlGeom inv;
    std::vector<double> rates;
    std::vector<int> S, keep;
    int M;
    size_t off_rowinfo, off_mag, off_owner, off_adv, off_rel;
};

// What tts_hip_time_stretch[_async, _probe] may be refused for -- order: pointers (plan, audio, out, rates) / B / N,
// lengths[b], a row reflect cannot pad, a Whisper plan, pre_emph > 0, a rate not finite or outside [0.25, 4], M not
// max_b llrint(L_b / r_b) (or that below 1), the 31-bit limits (either workspace, the vocoder's buffers, audio [B][N] and out
// [B][M]; B <= 65535), mem kind, what (probe: what >= 0; the call itself: -1); fills `g`
inline int time_stretch_check(const char* who, const MelPlan* p, const float* audio, int B, int N, const int32_t* lengths,
                              const double* rates, const float* out, int M, int mem, int what, TsGeom* g, char* msg, size_t n) {
    if (!p || !audio || !out || !rates || B < 1 || N < 1) return audio_refuse(msg, n, who, "bad argument");
    int min_len;
    if (int rc = audio_rows_check(who, B, N, lengths, g->fwd.lens, &min_len, msg, n)) return rc;
    for (int b = 0; b < B; ++b)
        if (mel_dft_frames(*p, g->fwd.lens[b]) < 1)
            return audio_refuse(msg, n, who, "row %d: max(L = %d, win_length = %d) samples are not more than filter_length // 2 = %d",
                                b, g->fwd.lens[b], p->wl, p->half);
    if (p->kind != TTS_HIP_MEL_TACOTRON) return audio_refuse(msg, n, who, "refused for a Whisper plan");
    if (p->pre > 0) return audio_refuse(msg, n, who, "pre_emph = %g > 0 cannot be inverted", p->pre);
    for (int b = 0; b < B; ++b)
        if (!ts_rate_ok(rates[b]))
            return audio_refuse(msg, n, who, "rates[%d] = %g must be finite and lie in [%g, %g]", b, rates[b], kTsRateMin, kTsRateMax);
    g->rates.assign(rates, rates + B);
    g->fwd.fout.resize(B);
    g->inv.frames.resize(B);
    g->S.resize(B);
    g->keep.resize(B);
    long long want = 0;
    int T = 1;
    for (int b = 0; b < B; ++b) {
        g->fwd.fout[b] = mel_dft_frames(*p, g->fwd.lens[b]);
        g->inv.frames[b] = ts_out_frames(g->fwd.fout[b], rates[b]);
        T = std::max(T, g->inv.frames[b]);
        const long long S = ts_out_samples(g->fwd.lens[b], rates[b]);
        want = std::max(want, S);
        g->S[b] = (int)S;                                       // <= 4 N
        g->keep[b] = (int)std::min<long long>(S, stft_samples(*p, g->inv.frames[b]));
    }
    if (want < 1) return audio_refuse(msg, n, who, "every row stretches to 0 samples");
    if (M != want) return audio_refuse(msg, n, who, "M = %d, but max_b llrint(lengths[b] / rates[b]) = %lld", M, want);
    const long long cells = (long long)B * T * p->cut;
    if (B > 65535 || mel_geom_layout(*p, B, N, &g->fwd) >= kAudioLim || cells * 8 >= kAudioLim ||
        gl_geom_layout(*p, B, T, p->cut, -1, -1, &g->inv) >= kAudioLim || (long long)B * M * 4 >= kAudioLim)
        return audio_refuse(msg, n, who, "B = %d x N = %d (M %d) too large for 31-bit offsets (B <= 65535)", B, N, M);
    if (int rc = audio_mem_check(who, mem, msg, n)) return rc;
    if (what >= TS_STAGES) return audio_refuse(msg, n, who, "no stage %d (0 .. %d)", what, TS_STAGES - 1);
    g->M = M;
    Carve c;
    c.o = g->inv.total;
    g->off_rowinfo = c.take((size_t)B * 12);
    g->off_mag = c.take((size_t)cells * 4);
    g->off_owner = c.take((size_t)cells * 4);
    g->off_adv = c.take((size_t)cells * 8);
    g->off_rel = c.take((size_t)cells * 8);
    g->inv.total = c.o;
    return TTS_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- formant match (stft_inv.hip)
enum { FM_LOGMAG = 0, FM_ENVELOPE, FM_GAIN, FM_OPERAND, FM_FRAMES, FM_STAGES };
constexpr double kFmWarpMin = 0.5, kFmWarpMax = 2.0, kFmGainDbMax = 60.0;

inline bool fm_warp_ok(double w) { return std::isfinite(w) && w >= kFmWarpMin && w <= kFmWarpMax; }

// The liftering table of a plan, L [cut][cut] in double: L[j][k] = (w_j / n) sum_{q <= Q} v_q cos(2 pi q j / n) cos(2 pi q k / n),
// w_0 = w_{cut-1} = 1 and v_0 = 1, every other weight 2 -- the real cepstrum of the even extension of a row of cut values, cut
// after quefrency Q, transformed back (smoothed = row . L).  The phases are reduced exactly (q k mod n).
inline void fm_lifter_table(int fl, int Q, std::vector<double>& L) {
    const int cut = fl / 2 + 1;
    std::vector<double> C((size_t)(Q + 1) * cut);
    for (int q = 0; q <= Q; ++q)
        for (int k = 0; k < cut; ++k) C[(size_t)q * cut + k] = std::cos(2.0 * M_PI * (double)(((long long)q * k) % fl) / fl);
    L.assign((size_t)cut * cut, 0.0);
    for (int j = 0; j < cut; ++j) {
        double* row = L.data() + (size_t)j * cut;
        for (int q = 0; q <= Q; ++q) {
            const double c = (q ? 2.0 : 1.0) * C[(size_t)q * cut + j];
            const double* cq = C.data() + (size_t)q * cut;
            for (int k = 0; k < cut; ++k) row[k] += c * cq[k];
        }
        const double w = ((j == 0 || j == cut - 1) ? 1.0 : 2.0) / fl;
        for (int k = 0; k < cut; ++k) row[k] *= w;
    }
}

// A formant-match call is one or two transforms on the rows' own frames (`fwd`: lens, fout = F_b, its workspace in
// e->stft.ws, which holds the audio's spectrum Y from the last transform to the gain kernel) and an inverse on F = fwd.Fr
// frame slots (`inv`: frames = F_b, its workspace in e->stft.inv_ws).  Behind the inverse's own buffers that workspace holds
// `warps` [B] doubles; `logmag` [2 * B * F][MAGK] fp32, the envelope GEMM's A operand (the source's rows, then the audio's;
// zero in the K padding and in the frames behind a row's own); `env` [2 * B * F][cut] fp32, Sx then Sy; and for the probe's
// stage FM_GAIN `gain` [B * F][cut].  inv.total covers them.  Row b of the result holds keep[b] = min(lens[b],
// stft_samples(F_b)) samples.
struct FmGeom {
    MelGeom fwd;
    GlGeom inv;
    std::vector<double> warps;
    std::vector<int> keep;
    int Q;
    float G;                                // the clamp of the log gain, (float)(max_gain_db * ln(10) / 20)
    size_t off_warps, off_logmag, off_env, off_gain;
};

// What tts_hip_formant_match[_async, _probe] may be refused for -- order: pointers (plan, audio, out) / B / N, lengths[b], a
// row reflect cannot pad, a Whisper plan, pre_emph > 0, a warp not finite or outside [0.5, 2] (warps NULL: 1 for every row),
// Q outside [1, filter_length / 2 - 1], max_gain_db not finite, not above 0 or above 60, the 31-bit limits (either workspace,
// the 2 * B * F stacked rows of the envelope GEMM, audio and out [B][N]; B <= 65535), mem kind, what (probe: what >= 0; the
// call itself: -1); fills `g`.  `source` may be NULL (the audio itself) and is not looked at here.
inline int formant_match_check(const char* who, const MelPlan* p, const float* audio, int B, int N, const int32_t* lengths,
                               const double* warps, int Q, double max_gain_db, const float* out, int mem, int what, FmGeom* g,
                               char* msg, size_t n) {
    if (!p || !audio || !out || B < 1 || N < 1) return audio_refuse(msg, n, who, "bad argument");
    int min_len;
    if (int rc = audio_rows_check(who, B, N, lengths, g->fwd.lens, &min_len, msg, n)) return rc;
    for (int b = 0; b < B; ++b)
        if (mel_dft_frames(*p, g->fwd.lens[b]) < 1)
            return audio_refuse(msg, n, who, "row %d: max(L = %d, win_length = %d) samples are not more than filter_length // 2 = %d",
                                b, g->fwd.lens[b], p->wl, p->half);
    if (p->kind != TTS_HIP_MEL_TACOTRON) return audio_refuse(msg, n, who, "refused for a Whisper plan");
    if (p->pre > 0) return audio_refuse(msg, n, who, "pre_emph = %g > 0 cannot be inverted", p->pre);
    g->warps.assign(B, 1.0);
    if (warps)
        for (int b = 0; b < B; ++b) {
            if (!fm_warp_ok(warps[b]))
                return audio_refuse(msg, n, who, "warps[%d] = %g must be finite and lie in [%g, %g]", b, warps[b], kFmWarpMin, kFmWarpMax);
            g->warps[b] = warps[b];
        }
    if (Q < 1 || Q > p->fl / 2 - 1) return audio_refuse(msg, n, who, "lifter Q = %d outside [1, filter_length / 2 - 1 = %d]", Q, p->fl / 2 - 1);
    if (!(std::isfinite(max_gain_db) && max_gain_db > 0 && max_gain_db <= kFmGainDbMax))
        return audio_refuse(msg, n, who, "max_gain_db = %g must be finite and lie in (0, %g]", max_gain_db, kFmGainDbMax);
    const long long big = mel_geom_layout(*p, B, N, &g->fwd);
    const long long rows2 = 2ll * B * g->fwd.Fr;
    if (B > 65535 || big >= kAudioLim || rows2 * p->MAGK * 4 >= kAudioLim ||
        gl_geom_layout(*p, B, g->fwd.Fr, p->cut, -1, -1, &g->inv) >= kAudioLim)
        return audio_refuse(msg, n, who, "B = %d x N = %d too large for 31-bit offsets (B <= 65535)", B, N);
    if (int rc = audio_mem_check(who, mem, msg, n)) return rc;
    if (what >= FM_STAGES) return audio_refuse(msg, n, who, "no stage %d (0 .. %d)", what, FM_STAGES - 1);
    g->Q = Q;
    g->G = (float)(max_gain_db * std::log(10.0) / 20.0);
    g->fwd.fout.resize(B);
    g->keep.resize(B);
    for (int b = 0; b < B; ++b) {
        g->fwd.fout[b] = mel_dft_frames(*p, g->fwd.lens[b]);
        g->keep[b] = (int)std::min<long long>(g->fwd.lens[b], stft_samples(*p, g->fwd.fout[b]));
    }
    g->inv.frames = g->fwd.fout;
    Carve c;
    c.o = g->inv.total;
    g->off_warps = c.take((size_t)B * 8);
    g->off_logmag = c.take((size_t)rows2 * p->MAGK * 4);
    g->off_env = c.take((size_t)rows2 * p->cut * 4);
    g->off_gain = c.take(what == FM_GAIN ? (size_t)(rows2 / 2) * p->cut * 4 : 0);
    g->inv.total = c.o;
    return TTS_HIP_OK;
}
