// engine.h -- internal state behind the tts_hip C ABI (include/tts_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/tts_hip.h"

#include "ttsw_host.h"      // HostTensor + the TTSW parser (host-only code, also built under ASan / UBSan)
#include "wg_call.h"        // WgCall: one WaveGlow call, its checks and its staged table (host-only code, likewise)
#include "audio_call.h"     // the audio calls' checks and the geometry they rest on (host-only code, likewise)
#include "taco_call.h"      // TacoEncode / TacoRun: the Tacotron2 calls, their checks and the forward pass's buffer sizes (likewise)

// Growable device buffer (workspace).  Never shrinks; reallocated only when a larger request arrives.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    float* f() const { return (float*)p; }
};

// ---------------------------------------------------------------- WaveGlow (fixed reference geometry but for the WN width
// C = WaveGlowDev::channels, 512 or 256; the shapes in the comments below are written for C = 512: 1024 stands for 2 C,
// 1536 for 3 C; the Winograd operands exist at 512 only)
struct WgLayerDev {
    float* in_Bt = nullptr;     // [1024 (tanh/sigmoid interleaved per 128-tile)][3*512 taps] (first layer of a flow: [3*16])
    float* cond_Bt = nullptr;   // [32 phases][1024][320] conditioning conv folded with the upsampling kernel
    float* in_bias = nullptr;   // [1024] in_conv bias + cond bias (+ upsampling bias pushed through), same row order
    // fp16 operands, built on first use of a mode: [0] the fp16 path, [1] split fp16, the same three matrices as
    // [2 planes][...] (hi, lo)
    _Float16* in_Bt16[2] = {nullptr, nullptr};      // [1024][1536] (taps in chunks of 32)
    _Float16* cond_Bt16[2] = {nullptr, nullptr};    // [32][1024][4*96]
    _Float16* rs_Bt16[2] = {nullptr, nullptr};      // [512][512]
    float* wino_G = nullptr;    // Winograd form (wn_wino.hip; built on first use): [6][1024][512] tap combinations and the
    float* wino_W = nullptr;    //   conditioning weight planes [32][7][1024][80] (F(4, 4) along frames; every layer)
    float* wino_T = nullptr;    //   first layer only (it has no wino_G): its composed taps as one K = 16 chunk, [1024][16]
    float* rs_Bt = nullptr;     // [512][512] residual half of res_skip (layers 0..6)
    float* rs_bias = nullptr;   // [512]
    int rs_n = 0;
};
struct WgFlowDev {
    int n_rem = 0, n_half = 0;
    float* start_w = nullptr;   // [n_half][512]
    float* start_b = nullptr;   // [512]
    float* end_w = nullptr;     // [8 layers][8][512] skip halves folded into the end conv (rows >= 2*n_half are zero)
    float* end_b = nullptr;     // [8]
    float* inv = nullptr;       // [n_rem][n_rem]  out = audio @ inv
    float* fwd = nullptr;       // [n_rem][n_rem]  the kernel itself: out = audio @ fwd (forward flow, wg_encode.hip)
    double log_det = 0.0;       // log |det fwd|
    WgLayerDev layer[8];
};
struct WaveGlowDev {
    bool ready = false;
    int channels = 0;                        // n_channels of the finalized model (512 or 256; 0 while none is): per handle
    WgFlowDev flow[12];
    std::vector<void*> allocs;
    bool f16_ready = false, x3_ready = false;
    int form_mode = 1, last_form = -1;       // tts_hip_set_waveglow_form / tts_hip_last_waveglow_form
    int last_tiles = -1;                     // tts_hip_last_waveglow_tiles: WN GEMM tile family of the last call
    int probe_flow = -1, probe_layer = -1;   // tts_hip_waveglow_probe[_rows] (test hook): stop after this layer (what 0, 2) or flow
    int probe_what = 0;                      //   (what 1) and copy its gated activations [B][T * 32][C], the flow state
    float* probe_out = nullptr;              //   [B][T * 32][n] or the layer's conditioning plane [B][T * 32][1024] (what 2;
                                             //   Winograd form only) to this device buffer
    bool wino_ready = false;                 // Winograd form of the fp32 in-layer GEMM (wn_wino.hip)
    WgTable call_table;                      // host image of ragged_info (staged to the device once per call), counts
    // ---- workspace: every DevBuf of this struct is declared here ...
    DevBuf x, acts, audio, a0p, endp;        // fp32 path (layouts: waveglow.hip)
    DevBuf x16, acts16, a0p16, mel16;        // fp16 path: shadow of x, activations, first-layer operand, mel
    DevBuf io_mel, io_z, io_out, io_zgen;    // staging for host callers; the noise of seeded calls
    DevBuf mel_ragged, ragged_info;          // ragged calls: mel copy with cleared tails; [lengths | tail frame list] int32
    DevBuf packed_z, packed_out;             // packed calls: noise and audio of the one packed row (its mel is mel_ragged, its
                                             //   [segment table | frame flags | gap frames] goes through ragged_info)
    DevBuf wino_U, wino_P, wino_mel;         // mel planes; forms 2 / 3 only: transformed inputs [6][M/4][512], products [6][M/4][1024]
    DevBuf wino_cond;                        // conditioning plane of the current layer [32 PR][1024]
    DevBuf wino_taps;                        // tap operand of the current flow's first layer [32 PR][16]
    DevBuf enc_ws;                           // forward flow (wg_encode.hip): [sum_j s per position | partial sums of the statistics]
    DevBuf enc_audio, enc_z;                 // forward flow: a host caller's audio; [z | stats] of a host caller, or whichever of
                                             //   the two a device caller passed NULL for
    // ... and listed here, which is what waveglow_free releases
    template <class F>
    void for_each_buf(F f) {
        for (DevBuf* b : {&x, &acts, &audio, &a0p, &endp, &x16, &acts16, &a0p16, &mel16, &io_mel, &io_z, &io_out, &io_zgen, &mel_ragged,
                          &ragged_info, &packed_z, &packed_out, &wino_U, &wino_P, &wino_mel, &wino_cond, &wino_taps, &enc_ws, &enc_audio,
                          &enc_z})
            f(*b);
    }
};

// ---------------------------------------------------------------- Tacotron2
struct ConvBnDev {              // conv k5 with batch-norm folded in
    float* Bt = nullptr;        // [cout][5 * cin_pad]
    float* bias = nullptr;      // [cout]  folded bias at unmasked rows
    float* altbias = nullptr;   // [cout]  BN(0) = value at masked rows
    int cin = 0, cin_pad = 0, cout = 0;
};
struct LstmDev {                // weights packed gate-interleaved: row r = 4*u + gate
    float* W = nullptr;         // [4u][kin_total]  (input kernel rows then recurrent rows, K contiguous)
    float* b = nullptr;         // [4u]
    _Float16* W16 = nullptr;    // fp16 copy of W for tts_hip_tacotron2_infer_f16 (built on first use)
    int units = 0, kin = 0;
};
// Output of the Tacotron2 encoder for one batch (tts_hip_tacotron2_encode): what the decoder loop needs, in its own device
// buffer so that several encoded batches can be alive at once.
struct tts_hip_encoded {
    int B = 0, Tin = 0, enc = 0;
    DevBuf buf;
    uint8_t* mask = nullptr;            // [B * Tin]  token != pad
    int* enc_len = nullptr;             // [B]
    int* bl_err = nullptr;              // BiLSTM block-exchange status (0 = ok), checked at the decoder's first synchronization
    float* memory = nullptr;            // [B * Tin][enc]
    float* pm = nullptr;                // [B * Tin][128]  processed memory
};

// The three machines that can run the decoder loop; the values are what tts_hip_last_decoder_mode reports.
// (DEC_FORWARD only names the chunk graphs of the teacher-forced pass in the graph cache: it is never a last_path.)
enum DecMachine { DEC_STEP_GRAPH = 0, DEC_PERSISTENT = 1, DEC_FUSED = 2, DEC_FORWARD = 3 };

// Identity of an instantiated decoder-chunk hipGraph: every pointer and scalar its 225 kernel nodes have baked in.
// ws_layout says which exchange areas the workspace plan sized in (the offset of every later buffer depends on it).
struct DecGraphKey {
    const void* ws;
    const void* enc_buf;
    int B, Tin, max_len_bucket, masks, win_len, win_off, half_w, ws_layout;
    DecMachine machine;
    auto tied() const { return std::tie(ws, enc_buf, B, Tin, max_len_bucket, masks, win_len, win_off, half_w, ws_layout, machine); }
    bool operator<(const DecGraphKey& o) const { return tied() < o.tied(); }
};

// Instantiated decoder-chunk graphs, replayed by every later call with the same key: the workspace and the encoded batch
// are stable allocations, so the kernel nodes hold valid pointers.  At most kCapacity graphs; the oldest is evicted first.
class DecGraphCache {
public:
    // captures what `enqueue` puts on `st` and instantiates it; nothing is left behind when any step fails
    static int capture(tts_hip_engine* e, hipStream_t st, const std::function<int()>& enqueue, hipGraphExec_t* out);
    int get_or_capture(tts_hip_engine* e, const DecGraphKey& key, hipStream_t st, const std::function<int()>& enqueue,
                       hipGraphExec_t* out);
    void drop_if(const void* enc_buf);      // the graphs whose kernel nodes point into this encoded batch
    void clear();

private:
    static constexpr size_t kCapacity = 16;
    std::map<DecGraphKey, hipGraphExec_t> graphs;
    std::vector<DecGraphKey> order;         // insertion order
};

struct Tacotron2Dev {
    bool ready = false;
    int enc_dim = 512, spk_dim = 0;
    int vocab = 148;                    // rows of the embedding table (the checkpoint's vocabulary)
    float* embeddings = nullptr;        // [vocab][512]
    ConvBnDev enc_conv[3];
    float* bl_in_Bt[2] = {nullptr, nullptr};   // BiLSTM input kernels [1024][512]
    float* bl_in_b[2] = {nullptr, nullptr};    // [1024]
    float* bl_rec[2] = {nullptr, nullptr};     // recurrent kernels transposed [1024][256]
    float* prenet_w0 = nullptr;         // [20][256][4]  (k / 4, output, k % 4)
    float* prenet_w1 = nullptr;         // [256][256]
    float* prenet_w0_Bt = nullptr;      // [256][96]  layer 0 as a GEMM operand (K = 80, zero padded): the forward call's bulk prenet
    LstmDev att, dec;
    float* query_w = nullptr;           // [128][1024]
    float* memory_Bt = nullptr;         // [128][enc]
    float* value_w = nullptr;           // [128]
    float* loc_dense = nullptr;         // [128][32]   (transposed)
    float* proj_w = nullptr;            // [81][1024 + enc]  (80 mel rows + gate row)
    float* proj_b = nullptr;            // [81]
    float* pfold_w = nullptr;           // [256][1024 + enc]  prenet layer 1 folded with the frame projection (taco_persist.hip)
    float* pfold_b = nullptr;           // [256]
    int persist_mode = 3;               // tts_hip_set_decoder_mode: 0 per-step graph only, 1 persistent kernel when allowed, 2 fused
                                        // two-kernel step when allowed, 3 auto (persistent for 1 - 2 rows, fused above)
    int last_path = -1;                 // how the last call ran its loop: 2 fused step, 1 persistent kernel, 0 per-step graph
    int last_conv_paths = -1;           // how each k = 5 conv last ran (conv_gemm): bit i set = single pass; bits 0-2 encoder
                                        // convs 1-3, bits 3-7 postnet convs 1-5; -1 before the first conv
    bool persist_timed = true;          // persistent kernel: timed optimistic polls on (switched off if they mostly miss)
    int fused_backoff = 0;              // calls to keep off the fused step after one of its exchanges timed out (shared GPU)
    int fused_fail_streak = 0;
    ConvBnDev post_conv[5];
    std::vector<void*> allocs;
    DevBuf ws;                          // per-call workspace arena
    DevBuf io;                          // staging for host callers
    DevBuf loss_ws;                     // the one workspace of a loss call (TacoLossLayout, taco_loss.hip)
    tts_hip_encoded* enc_cache = nullptr;                 // encoder output of tts_hip_tacotron2_infer* calls (reused: stable pointers)
    DecGraphCache graphs;                                 // instantiated decoder-chunk graphs, replayed across calls
    void* pinned = nullptr;                               // pinned host ring for the decoder loop's chunk reports (2 x 64 bytes)
    hipEvent_t chunk_ev[2] = {nullptr, nullptr};
};

// ---------------------------------------------------------------- audio front end (mel_stft.hip, audio_proc.hip,
// resample.hip, silence.hip).  These structs hold weights, tables and per-call workspaces only: what a TTS_HIP_MEM_HOST
// caller passes in and gets back is staged through the engine's one `audio_io` (AudioStage below), and the per-row int
// table of a call through `audio_info_h` (stage_row_info).
// One mel plan (tts_hip_mel_fn_create): a checked configuration and its two tables on the device
struct tts_hip_mel_fn {
    MelPlan p;
    float* basis_Bt = nullptr;          // [NB][Kpad] windowed cos rows of bins 0 .. cut - 1, then the -sin rows; zero padded
    float* mel_Bt = nullptr;            // [n_mel][MAGK] Slaney filterbank, zero padded
    // stft_inv.hip, built on first use
    float* inv_Bt = nullptr;            // [filter_length][NB] windowed inverse basis: column r < cut the real row of bin r, cut + r the imaginary
    float* win2 = nullptr;              // [filter_length] the centred window squared
    float* minv_Bt = nullptr;           // [cut][EK] the filterbank's minimum-norm inverse (log-mel input), zero padded
    int minv_state = 0;                 //   0 not tried, 1 built, -1 the factorisation failed
    float* lift_Bt = nullptr;           // [cut][MAGK] the liftering table of tts_hip_formant_match: row k holds L[.][k], zero padded
    int lift_Q = 0;                     //   the cut it was built for (0: not built); a call with another Q rebuilds it
    std::vector<double> win;            // the window centred in filter_length (what the tables were built from)
    std::vector<void*> allocs;
};
struct MelStftDev {
    bool ready = false;                 // the default plan exists (tts_hip_finalize)
    tts_hip_mel_fn* def = nullptr;      // 1024 / 256 / 1024, 80 mels, 22 050 Hz, 0 - 8000 Hz: what tts_hip_mel_stft runs
    std::vector<tts_hip_mel_fn*> plans; // the caller's plans still alive
    DevBuf ws;                          // the one workspace of a call (MelGeom)
    DevBuf inv_ws;                      // the one workspace of an inverse / Griffin-Lim call (GlGeom, stft_inv.hip)
    std::vector<float> minv_h;          // host image of a caller's Minv while it is staged
};

// Waveform clean-up (audio_proc.hip): DFT bases built on first use, no weights
struct AudioProcDev {
    float* fwd_Bt = nullptr;            // [2080][2048] windowed cos / -sin rows
    float* inv_Bt = nullptr;            // [2048][2080] irfft terms x synthesis window
    double* win2 = nullptr;             // [2048] hann^2
    std::vector<void*> allocs;
    DevBuf ws, trim_win;                // workspace, trim window (+ its reversal) for window length trim_wl
    int trim_wl = -1;
};

// Resampling (resample.hip): the W_8192 twiddle table built on first use; the workspace holds, per row, the stage lines
// (signal and filter: 16 * max(L_fwd, L_inv) bytes) and the kept rfft bins (8 * (N_b // 2 + 1) bytes)
struct ResampleDev {
    DevBuf tw, ws;                      // twiddles, workspace
};

// MCD / DTW (mel_dtw.hip): no weights; the DCT tables built so far, per (n_mel, n_cep, c0), and the one workspace of a call
struct MelDtwDev {
    std::map<std::tuple<int, int, int>, float*> dct;      // device [R][n_mel]
    std::vector<int32_t> lens_h;        // host image of a call's [len_a | len_b] while it is staged
    DevBuf ws;                          // MelDtwLayout (mel_dtw_call.h)
};

// Pitch tracks and their comparison (pitch.hip): no weights and no tables, the one workspace of a call
struct PitchDev {
    std::vector<int32_t> lens_h;        // host image of a call's length tables while it is staged
    std::vector<float> tables_h;        // host image of a pYIN call's cumulative prior and transition tables (pyin_tables)
    DevBuf ws;                          // PitchLayout / PyinLayout / F0ErrorLayout (pitch_call.h)
};

struct TimedLaunch {
    hipEvent_t a, b;
    int kind;
};

struct tts_hip_engine {
    int device = 0;
    int n_cu = 0;                       // compute units of `device`
    hipStream_t stream = nullptr;
    mutable std::string err;
    std::map<std::string, HostTensor> host;
    WaveGlowDev wg;
    Tacotron2Dev taco;
    MelStftDev stft;
    AudioProcDev aproc;
    ResampleDev resamp;
    MelDtwDev dtw;
    PitchDev pitch;
    // Host staging of every synchronous audio call (AudioStage).  One buffer serves them all: calls on one handle are
    // serialised by the caller and a synchronous call drains the stream before it returns, so no call finds another's data
    // still in use here; a call that needs more than its predecessors reallocates it before it copies anything in.
    DevBuf audio_io;
    std::vector<int> audio_info_h;      // host image of a call's per-row int table (stage_row_info)
    // timing hooks
    bool timing = false;
    std::vector<TimedLaunch> timed;
    std::vector<TimedLaunch> ev_pool;
    double time_sum_us[5] = {0, 0, 0, 0, 0};
    int64_t time_cnt[5] = {0, 0, 0, 0, 0};
};

int set_err(const tts_hip_engine* e, int code, const char* fmt, ...);

// Calls on one handle are serialised by the caller; for the duration of a call its work goes to `stream` when the caller
// passed one (the *_async entry points, tacotron2 encode / decode), else to the handle's own stream.
struct StreamScope {
    tts_hip_engine* e;
    hipStream_t saved;
    StreamScope(tts_hip_engine* eng, void* stream) : e(eng), saved(eng->stream) {
        if (stream) e->stream = (hipStream_t)stream;
    }
    ~StreamScope() { e->stream = saved; }
};

#define HIPCHK(e, call)                                                                                         \
    do {                                                                                                        \
        hipError_t _err = (call);                                                                               \
        if (_err != hipSuccess)                                                                                 \
            return set_err((e), TTS_HIP_EHIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_err)); \
    } while (0)

// Winograd form of the WN in-layer GEMM (wn_wino.hip)
int waveglow_build_wino(tts_hip_engine* e);
int waveglow_wino_begin(tts_hip_engine* e, const float* d_mel, int PR, int BT, int T, int form);
int waveglow_wino_layer(tts_hip_engine* e, const WgLayerDev& ly, int i, const float* x, float* acts_i, int PR, int BT, int T);
int waveglow_wino_layer0(tts_hip_engine* e, const WgLayerDev& ly, int h, const float* a0p, float* acts_0, int PR, int BT, int T);
// timing helpers (engine.hip)
void timing_begin(tts_hip_engine* e, int kind);
void timing_end(tts_hip_engine* e);
void timing_collect(tts_hip_engine* e);

// model entry points (device pointers only)
int waveglow_finalize(tts_hip_engine* e);
// d_lens (device int32 [B], null = every row holds T frames), d_tail / n_tail: the frames beyond the rows' lengths
int waveglow_run(tts_hip_engine* e, const float* d_mel, int B, int T, const float* d_z, float sigma, float* d_audio,
                 int precision, const int* d_lens = nullptr, const int* d_tail = nullptr, int n_tail = 0,
                 const int* d_flags = nullptr);
// packed call: mel / z / audio in the batch layout, d_info = [start[B] | len[B] | flags[F] | gap frames[n_gap]] (waveglow.hip)
int waveglow_run_packed(tts_hip_engine* e, const float* d_mel, int B, int T, const float* d_z, float sigma, float* d_audio,
                        int precision, const int* d_info, int F, int n_gap);
// forward flow, audio -> z and its statistics (fp32; one run: B * T <= kMaxFramesPerRun).  d_z [B, T*32, 8] and d_stats
// [3, B] are device buffers, both written; d_lens / d_tail / n_tail as for waveglow_run.  probe (test hook, wg_call.h): the
// same run stops after that flow, copies what the probe asks for to its device buffer `out` and leaves d_stats unwritten
int waveglow_encode_run(tts_hip_engine* e, const float* d_audio, const float* d_mel, int B, int T, const int* d_lens,
                        const int* d_tail, int n_tail, float* d_z, float* d_stats, const WgEncodeProbe* probe = nullptr);
// its position-wise kernels (wg_encode.hip); mask: 0 every frame is real, 1 the first d_lens[b] of each row
int wg_encode_init(tts_hip_engine* e, const float* d_audio, const float* fwd0, float* state, int PR, int BT, const int* d_lens, int T);
struct WgEncodeEnd {
    int C;                          // n_channels of the handle
    const float* acts;              // gated activations of the flow's eight layers, layer_stride floats apart
    long long layer_stride;
    const float *wfold, *bfold;     // the flow's folded skip / end weights
    float* state;                   // [M][8] phase-major flow state, updated in place
    float* slog;                    // [M] sum over flows and coupling channels of s, per position
    int first;                      // flow 0: slog is stored, not added to
    const float* next;              // the next flow's matrix [n][n], n = 2 h - n_early; null after the last flow
    float* z;                       // [B, T*32, 8]: the n_early channels that leave go to z[.., zoff ..], the last flow's 4 to z[.., 0 ..]
    int zoff, n_early;
    long long M;
    int h, PR, BT;
    const int* d_lens;              // null: every frame is real
    int T;
};
int wg_encode_end(tts_hip_engine* e, const WgEncodeEnd& a);
size_t wg_encode_stats_bytes(int B);    // the partial sums of wg_encode_stats
int wg_encode_stats(tts_hip_engine* e, const float* d_z, const float* slog, double* part, const int* d_lens, int B, int T, int PR,
                    double log_det_sum, float* d_stats);
void waveglow_free(tts_hip_engine* e);

int tacotron2_finalize(tts_hip_engine* e);
void tacotron2_free(tts_hip_engine* e);

// ---- audio front end
// What a probe copies out of a workspace: `rows` rows of `width` floats, `pitch` floats apart
struct StageView {
    const void* p;
    size_t rows, width, pitch;
};
// the view's logical extent (row padding dropped) to `out`, host or device as `mem` says, on e->stream
int copy_stage_out(tts_hip_engine* e, const StageView& v, float* out, int mem);
// e->audio_info_h to d_info on e->stream (pageable source: the copy has left it when the call returns)
int stage_row_info(tts_hip_engine* e, int* d_info);

// One synchronous audio call's way in and out.  Declare the caller's inputs and outputs, begin(), run on ptr(slot), finish().
// TTS_HIP_MEM_HOST: begin() carves `audio_io` and copies the inputs in, ptr() is the slot's slice, finish() copies the
// outputs back; TTS_HIP_MEM_DEVICE: ptr() is the caller's own pointer.  finish() drains e->stream either way.  A NULL
// input stays NULL; scratch() is a device slice of audio_io whatever `mem` says.
class AudioStage {
public:
    AudioStage(tts_hip_engine* eng, int mem) : e(eng), host(mem == TTS_HIP_MEM_HOST) {}
    int in(const void* p, size_t bytes) { return add(const_cast<void*>(p), bytes, IN, host && p); }
    int out(void* p, size_t bytes) { return add(p, bytes, OUT, host && p); }
    int scratch(size_t bytes) { return add(nullptr, bytes, SCRATCH, true); }
    int begin();
    int finish();
    template <class T>
    T* ptr(int slot) const { return (T*)(slots[slot].staged ? (char*)e->audio_io.p + slots[slot].off : (char*)slots[slot].user); }

private:
    enum Kind { IN, OUT, SCRATCH };
    struct Slot { void* user; size_t bytes, off; Kind kind; bool staged; };
    int add(void* p, size_t bytes, Kind kind, bool staged) {
        slots.push_back(Slot{p, bytes, staged ? carve.take(bytes) : 0, kind, staged});
        return (int)slots.size() - 1;
    }
    tts_hip_engine* e;
    bool host;
    Carve carve;
    std::vector<Slot> slots;
};

int melstft_finalize(tts_hip_engine* e);
// mel_stft.hip for stft_inv.hip: the stages mel_fn_exec can stop at, the run itself (device pointers only, the call already
// checked; stop = -1 runs everything), its DFT product, and "NULL or a plan alive on this handle"
enum { MEL_PADDED = 0, MEL_SPECTRUM, MEL_MAGNITUDE, MEL_LINEAR, MEL_LOG, MEL_STAGES };
int mel_fn_exec(tts_hip_engine* e, const tts_hip_mel_fn& fn, const MelGeom& g, const float* d_audio, int B, int N, bool ragged,
                float* d_mel, int stop = -1, StageView* stop_out = nullptr);
int mel_dft_gemm(tts_hip_engine* e, const tts_hip_mel_fn& fn, const float* padded, float* gathered, float* ft, int B, int Fr, int NP);
int mel_plan_check(tts_hip_engine* e, const char* name, const tts_hip_mel_fn* fn);
void melstft_free(tts_hip_engine* e);
void audioproc_free(tts_hip_engine* e);
void resample_free(tts_hip_engine* e);
void mel_dtw_free(tts_hip_engine* e);
void pitch_free(tts_hip_engine* e);

// shared helpers
// n floats of device-side samples into `out` on `st` (engine.hip: Philox4x32-10; kind = TTS_HIP_RANDOM_*)
int philox_fill(tts_hip_engine* e, float* out, long long n, uint64_t seed, uint64_t offset, int kind, hipStream_t st);
// B rows, `row_stride` floats apart: row b = the first counts[b] (null = row_stride) elements of stream (keys[b], offsets[b]);
// keys / offsets / counts are host arrays, copied into the kernel arguments before the call returns
int philox_fill_rows(tts_hip_engine* e, float* out, int B, long long row_stride, const uint64_t* keys, const uint64_t* offsets,
                     const long long* counts, int kind, hipStream_t st);
const HostTensor* find_tensor(const tts_hip_engine* e, const std::string& name);
// uploads a host tensor to a fresh device allocation tracked in `allocs`
int upload(tts_hip_engine* e, const float* src, size_t n, float** dst, std::vector<void*>& allocs);
int dev_alloc(tts_hip_engine* e, size_t n_floats, float** dst, std::vector<void*>& allocs, bool zero);
