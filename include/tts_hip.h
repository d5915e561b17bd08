/*
 * tts_hip.h -- C ABI of the MI355X (gfx950) Tacotron2 + WaveGlow + mel-STFT inference engine.
 *
 * This is the drop-in boundary for the reference's runtime seam: `BaseModel(runtime=...)`
 * (/root/reference/models/interfaces/base_model.py:139-209) hands `compiled_infer` calls
 * (base_model.py:367-375) to a `Runtime` object (utils/keras/runtimes/runtime.py:19-41) registered in
 * `_runtimes` (utils/keras/runtimes/__init__.py:39-45).  The Python class `text_to_speech_amd.runtime.HipRuntime`
 * is that object; it binds the functions below with ctypes.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success, a negative TTS_HIP_E* code otherwise; `tts_hip_last_error` gives the text;
 *   - all tensors are dense, row-major, float32 (tokens/lengths int32), channels-last like the reference ([B, T, C]);
 *   - `mem` says where caller buffers live: TTS_HIP_MEM_HOST (pageable/pinned host memory) or TTS_HIP_MEM_DEVICE
 *     (pointers into the engine's GPU, e.g. torch tensors' data_ptr()); the engine never keeps caller pointers;
 *   - one HIP stream per handle; calls on one handle are serialised by the caller (the reference calls
 *     `infer` sequentially from one thread, base_model.py:702); different handles are independent;
 *   - no global state besides the handle.
 */
#ifndef TTS_HIP_H_
#define TTS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tts_hip_engine tts_hip_engine;

enum {
    TTS_HIP_OK = 0,
    TTS_HIP_EINVAL = -1,   /* bad argument / shape */
    TTS_HIP_ENOTREADY = -2,/* weights missing or not finalized */
    TTS_HIP_EHIP = -3,     /* HIP runtime error (text in last_error) */
    TTS_HIP_EIO = -4,      /* weight file error */
    TTS_HIP_ENOMEM = -5
};

enum { TTS_HIP_MEM_HOST = 0, TTS_HIP_MEM_DEVICE = 1 };

/* ---- lifetime ---------------------------------------------------------------------------------------------------
 * Replaces Runtime.load_engine(path) / Runtime.__init__ (runtimes/runtime.py:22-29).                               */
int tts_hip_create(int device, tts_hip_engine** out);
int tts_hip_destroy(tts_hip_engine* e);
const char* tts_hip_last_error(const tts_hip_engine* e);
/* ABI version of this header (bumped on any signature change). */
int tts_hip_abi_version(void);

/* ---- weights ----------------------------------------------------------------------------------------------------
 * Replaces BaseModel._restore_model -> CheckpointManager.load (base_model.py:760-783,
 * custom_train_objects/checkpoint_manager.py:169-215).  Tensor names and Keras layouts: text_to_speech_amd/weights.py.
 * `tts_hip_set_tensor` copies `data` (host float32) into the engine; `tts_hip_load_weights` reads a TTSW file and
 * calls it per tensor.  `tts_hip_finalize` builds the derived device buffers (transposed / permuted kernels, folded
 * batch-norm, inverted 1x1 matrices -- the analogue of WaveGlow.set_weights -> build_inverse,
 * waveglow_arch.py:308-310) for every model whose tensors are complete.  `speaker_embedding_dim` is 0 or 256.        */
int tts_hip_set_tensor(tts_hip_engine* e, const char* name, const float* data, const int64_t* dims, int ndim);
int tts_hip_load_weights(tts_hip_engine* e, const char* ttsw_path);
int tts_hip_finalize(tts_hip_engine* e);
/* Validates the container structure of a TTSW file (magic, version, entry table, dims, payload ranges against the file
 * size) without an engine or a GPU; 0 if `tts_hip_load_weights` would accept it, else TTS_HIP_EIO / TTS_HIP_ENOMEM with the
 * reason in `errbuf` (may be NULL).  The reference's loader trusts its checkpoint files
 * (custom_train_objects/checkpoint_manager.py:169-215); a C loader cannot.                                           */
int tts_hip_check_weights_file(const char* ttsw_path, char* errbuf, int errbuf_len);
/* 1 if the model ("waveglow" | "tacotron2" | "mel_stft") is ready to run, else 0. */
int tts_hip_has_model(const tts_hip_engine* e, const char* model);

/* ---- WaveGlow.infer  (architectures/waveglow_arch.py:244-306; called at models/tts/waveglow.py:82,96,104,112,128)
 * mel   [B, T, 80]
 * z     NULL (=> zeros: the reference's deterministic=True) or [B, T*32, 8] noise, consumed in the reference's order
 *       (channels 0..3 initial audio, 4..5 early output after flow 8, 6..7 after flow 4)
 * audio [B, T*256] out
 *
 * The shared contract of every tts_hip_waveglow_infer* call (this one, _f16, _f16x3, _seeded, _ragged, _packed, _rows_seeded and
 * the _async forms further down; each comment below only says what its entry adds):
 *   - `precision`, where a call has the argument: 0 f32 (in the form tts_hip_set_waveglow_form selects), 1 f16, 2 f16x3;
 *   - a call with `mem` runs on the handle's stream and returns when it has drained; mel, z and audio live where `mem` says.
 *     An _async call takes device pointers and a `stream` (NULL = the handle's), enqueues and returns without synchronizing.
 *     `lengths`, `keys` and `offsets` are host arrays in every mode, read before the call returns;
 *   - a call is refused with TTS_HIP_EINVAL before anything is copied or launched, and the message starts with the name of the
 *     symbol that was called.  The reasons, first match first: precision outside 0 .. 2; a `mem` that is no TTS_HIP_MEM_*;
 *     keys or offsets NULL; B <= 0; mel or audio NULL or T <= 0; B * T above 2^25 frames; packed without lengths; a
 *     lengths[b] outside [0, T]; more frames than one run takes (31744): T of a call that is not packed -- a larger B * T runs
 *     as slices of whole rows inside the call, a longer single row needs windowed inference -- or F of a packed call;
 *   - the same arguments give the same bits through every entry point and memory kind that can express them.           */
int tts_hip_waveglow_infer(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                           float* audio, int mem);
/* Same contract with fp16 GEMM operands (the reference's Keras mixed_float16 policy, utils/keras/gpu.py:32-34; BASELINE
 * configs 3 and 5): activations, mel and weights are fp16 in HBM, accumulation and epilogue math are fp32, the residual
 * stream and the flow state keep fp32 master copies; inputs / outputs stay float32.  The fp16 operands are derived from
 * the finalized fp32 weights on first use.                                                                          */
int tts_hip_waveglow_infer_f16(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                               float* audio, int mem);

/* Same contract in split-fp16 arithmetic: every GEMM operand (activations, mel, weights) is held as two fp16 planes
 * hi = fp16(v), lo = fp16(v - hi) (~22 significant bits) and a product is the three MFMAs hi*hi + hi*lo + lo*hi
 * accumulated in fp32 -- the "3x" emulation of fp32 GEMM on half-precision matrix cores: fp32-class results (waveform RMS
 * error ~1e-6 against the fp32 oracle) at 3/16 of the fp32 MFMA cost.  Everything outside the GEMM operands is fp32.      */
int tts_hip_waveglow_infer_f16x3(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                                 float* audio, int mem);

/* ---- device-side sampling
 * The reference draws WaveGlow's noise and the prenet dropout inside `infer`, on the device
 * (architectures/waveglow_arch.py:272-274,299-302: `keras.random.normal`; tacotron2_arch.py:197-201: dropout p = 0.5).
 * `tts_hip_random_fill` writes n floats to a DEVICE buffer `out` on `stream` (NULL = the handle's stream) without
 * synchronizing; kind TTS_HIP_RANDOM_NORMAL: N(0, 1); kind TTS_HIP_RANDOM_PRENET_MASK: 2.0 with probability 0.5 else 0.0
 * (the multiplicative masks `tts_hip_tacotron2_infer` takes).  Generator: Philox4x32-10, key = seed, block counter =
 * offset + i / 4, element i = word i % 4; normals by Box-Muller on word pairs (see csrc/engine.hip; restated in
 * oracle/philox_ref.py).  The same (seed, offset) always gives the same values; consecutive calls should advance `offset`
 * by ceil(n / 4).
 * `tts_hip_waveglow_infer_seeded` = WaveGlow.infer(mel, z=None, deterministic=False): z [B, T*32, 8] is generated on the
 * device from (seed, offset) and never crosses PCIe.                                                                    */
enum { TTS_HIP_RANDOM_NORMAL = 0, TTS_HIP_RANDOM_PRENET_MASK = 1 };
int tts_hip_random_fill(tts_hip_engine* e, int kind, uint64_t seed, uint64_t offset, float* out, int64_t n, void* stream);
int tts_hip_waveglow_infer_seeded(tts_hip_engine* e, const float* mel, int B, int T, uint64_t seed, uint64_t offset,
                                  float sigma, float* audio, int precision, int mem);

/* Per-row streams: seeded output that does not depend on how rows were batched.  Row b owns the stream (keys[b],
 * offsets[b]); `tts_hip_random_fill_rows` writes out[b * row_stride + i] = element i of that stream -- the element rule of
 * `tts_hip_random_fill`: word i % 4 of block offsets[b] + i / 4 under key keys[b] -- for i < counts[b] (counts NULL =
 * row_stride for every row; 0 <= counts[b] <= row_stride) and touches nothing at i >= counts[b].  keys, offsets and counts
 * are HOST arrays of B entries, read before the call returns; `out` is a DEVICE buffer; enqueued on `stream` (NULL = the
 * handle's stream) without synchronizing.  B = 1 is `tts_hip_random_fill` bit for bit.
 * `tts_hip_waveglow_infer_rows_seeded[_async]`: tts_hip_waveglow_infer_ragged[_async] (packed == 0; lengths may be NULL) or
 * tts_hip_waveglow_infer_packed[_async] (packed != 0; needs lengths) with the noise drawn inside the engine:
 * z[b, p, c] = normal element p * 8 + c of row b's stream, only lengths[b] * 256 values per row when lengths are given.  A
 * row's noise -- and, where a row's arithmetic is its own (lengths given), its audio up to fp32 re-association -- is the
 * same whichever batch, row position or neighbours it is vocoded with.  Without lengths the rows are a padded batch and
 * every row still hears its neighbours' padding as in tts_hip_waveglow_infer.                                           */
int tts_hip_random_fill_rows(tts_hip_engine* e, int kind, const uint64_t* keys, const uint64_t* offsets, int B,
                             int64_t row_stride, const int64_t* counts, float* out, void* stream);
int tts_hip_waveglow_infer_rows_seeded(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                       const uint64_t* keys, const uint64_t* offsets, float sigma, float* audio, int precision,
                                       int packed, int mem);
int tts_hip_waveglow_infer_rows_seeded_async(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                             const uint64_t* keys, const uint64_t* offsets, float sigma, float* audio,
                                             int precision, int packed, void* stream);

/* ---- Tacotron2.infer  (architectures/tacotron2_arch.py:866-925; called at models/tts/tacotron2.py:162)
 * tokens        int32 [B, Tin], 0 = pad
 * speaker       NULL or [B, speaker_embedding_dim]
 * max_len       decoder steps allocated (the caller resolves the reference's float `max_length`, :886-892)
 * early_stop    1: stop when every row has fired its stop token (:625-627); 0: run max_len steps
 * prenet_masks  NULL (=> deterministic prenet) or [B, max_len, 2, 256] multiplicative dropout masks
 * win_len/win_offset  attention window (:630-638); win_len <= 0 disables it
 * outputs (any may be NULL): mel [B, max_len, 80], decoder_output [B, max_len, 80], stop_tokens [B, max_len],
 *                            attention [B, max_len, Tin], lengths int32 [B]; *steps_run = loop iterations executed    */
int tts_hip_tacotron2_infer(tts_hip_engine* e, const int32_t* tokens, int B, int Tin, const float* speaker,
                            int max_len, int early_stop, const float* prenet_masks, int win_len, int win_offset,
                            float* mel, float* decoder_output, float* stop_tokens, float* attention,
                            int32_t* lengths, int32_t* steps_run, int mem);

/* Same contract with the two decoder LSTM weight matrices (98 % of the bytes a decoder step streams) held in fp16
 * (BASELINE configs 3 and 5: "fp16 weights, fp32 accumulate"); inputs, recurrent state, accumulation, attention, prenet,
 * projections, encoder and postnet stay float32.  The fp16 copies are derived from the finalized weights on first use. */
int tts_hip_tacotron2_infer_f16(tts_hip_engine* e, const int32_t* tokens, int B, int Tin, const float* speaker,
                                int max_len, int early_stop, const float* prenet_masks, int win_len, int win_offset,
                                float* mel, float* decoder_output, float* stop_tokens, float* attention,
                                int32_t* lengths, int32_t* steps_run, int mem);

/* ---- stream-ordered variants ("... , hipStream_t" entry points) ------------------------------------
 * The calls above run on the handle's own stream and return when it has drained.  These take a caller `stream`
 * (a hipStream_t passed as void*; NULL = the handle's stream), only accept device pointers, enqueue their work and return
 * WITHOUT synchronizing, so a caller can queue transfers, several calls and its own kernels back to back.  A handle still
 * has one workspace per model: two calls on the same handle must be ordered (same stream, or an event between streams).
 * precision: as the WaveGlow contract above says; 0 = f32, 1 = fp16 LSTM weights (Tacotron2).
 *
 * Tacotron2 in two calls -- Tacotron2Encoder (tacotron2_arch.py:235-333, once per batch) and the decoder loop + postnet
 * (:609-749, :915-917):  `encode` is asynchronous and returns an opaque encoded batch (its own device buffer; free it with
 * tts_hip_encoded_free; several may be alive, e.g. the next sentence's encoder running ahead); `decode` may be called any
 * number of times on it (the retry loop of models/tts/tacotron2.py:160-179 re-runs only the decoder with new dropout
 * masks) and synchronizes `stream` before it returns, because the loop's exit is data dependent and `steps_run` is a host
 * value.  tts_hip_tacotron2_infer == encode + decode.
 *
 * Why a Tacotron2 call is refused (csrc/taco_call.h: the two checks every entry point below and tts_hip_tacotron2_infer* go
 * through; a NULL handle is TTS_HIP_EINVAL without a message).  Before any GPU work, first match wins, the message is
 * "<symbol without tts_hip_>: <reason>":
 *   an encoder run (encode, reencode, probe_encoder, the first half of infer*): bad mem kind; weights not finalized
 *     (TTS_HIP_ENOTREADY); tokens NULL, B outside [1, 1024] or Tin outside [1, 4096]; a model with speaker embeddings and
 *     speaker NULL.
 *   a run on an encoded batch (decode*, forward, the second half of infer*): precision not 0 / 1; bad mem kind; weights not
 *     finalized (TTS_HIP_ENOTREADY); encoded batch NULL or empty; encoded batch of another width than the handle's weights;
 *     keys / offsets NULL (decode_rows_seeded), mel_input / mel_lengths NULL (forward); max_len or T < 1; and for forward
 *     B * T > 65536, then mel_lengths[b] outside [1, T].
 * infer* passes both checks, in that order, before its encoder is enqueued.                                             */
typedef struct tts_hip_encoded tts_hip_encoded;
int tts_hip_waveglow_infer_async(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma,
                                 float* audio, int precision, void* stream);
int tts_hip_mel_stft_async(tts_hip_engine* e, const float* audio, int B, int N, float* mel, void* stream);
int tts_hip_tacotron2_encode(tts_hip_engine* e, const int32_t* tokens, int B, int Tin, const float* speaker, int mem,
                             void* stream, tts_hip_encoded** out);
int tts_hip_tacotron2_decode(tts_hip_engine* e, const tts_hip_encoded* encoded, int max_len, int early_stop,
                             const float* prenet_masks, int win_len, int win_offset, int precision, float* mel,
                             float* decoder_output, float* stop_tokens, float* attention, int32_t* lengths,
                             int32_t* steps_run, int mem, void* stream);
/* `decode` with the prenet dropout masks drawn on the device from (seed, offset) (tts_hip_random_fill, kind
 * TTS_HIP_RANDOM_PRENET_MASK, n = B * max_len * 512): the reference's default inference path keeps this dropout on
 * (tacotron2_arch.py:197-201), and a retry only needs another offset.                                                  */
int tts_hip_tacotron2_decode_seeded(tts_hip_engine* e, const tts_hip_encoded* encoded, int max_len, int early_stop,
                                    uint64_t seed, uint64_t offset, int win_len, int win_offset, int precision,
                                    float* mel, float* decoder_output, float* stop_tokens, float* attention,
                                    int32_t* lengths, int32_t* steps_run, int mem, void* stream);
/* `decode_seeded` with one stream per row (keys / offsets: HOST arrays of B entries, B = the encoded batch's rows): row b's
 * masks [max_len, 2, 256] are mask elements 0 .. max_len * 512 of stream (keys[b], offsets[b]), so step t of a row reads the
 * same bits whatever max_len the batch imposes and whichever rows it is decoded with.  All three decoder machines.      */
int tts_hip_tacotron2_decode_rows_seeded(tts_hip_engine* e, const tts_hip_encoded* encoded, int max_len, int early_stop,
                                         const uint64_t* keys, const uint64_t* offsets, int win_len, int win_offset,
                                         int precision, float* mel, float* decoder_output, float* stop_tokens,
                                         float* attention, int32_t* lengths, int32_t* steps_run, int mem, void* stream);
/* Teacher-forced forward pass of an encoded batch (Tacotron2.call, tacotron2_arch.py:806-849 with :526-607): step t of the
 * decoder reads frame t of `mel_input` [B, T, 80] -- ALREADY SHIFTED: frame 0 is the zero go-frame, frame t is target frame
 * t - 1 (models/tts/tacotron2.py:243-259) -- instead of its own previous output.  Every row runs all T steps (no stop test,
 * no attention window); mel_lengths: HOST int32 [B], each in 1 .. T.  prenet_masks: NULL (deterministic) or [B, T, 2, 256]
 * multiplicative dropout masks; precision 0 = f32, 1 = fp16 copies of the two decoder LSTM matrices in the loop.
 * Outputs (any may be NULL): decoder_output [B, T, 80] = where(t <= mel_lengths[b], frame, 0), mel = decoder_output +
 * postnet(decoder_output) under that mask, stop_tokens [B, T] = sigmoid(gate), unmasked, attention [B, T, Tin].  Frames at
 * and past a row's length are consumed as given.  mel_input, prenet_masks and the outputs live where `mem` says.
 * Refused as the block below says; its own limits are B * T <= 65536 and mel_lengths[b] in [1, T].  Synchronizes `stream`
 * (NULL: the handle's) before returning, like `decode`; a following tts_hip_tacotron2_infer* / decode call on the handle is
 * unaffected.                                                                                                           */
int tts_hip_tacotron2_forward(tts_hip_engine* e, const tts_hip_encoded* encoded, const float* mel_input, int T,
                              const int32_t* mel_lengths, const float* prenet_masks, int precision, float* mel,
                              float* decoder_output, float* stop_tokens, float* attention, int mem, void* stream);
/* The reference's TacotronLoss (custom_train_objects/losses/tacotron_loss.py: call, compute_mel_loss) on the outputs of
 * `forward` and the targets of Tacotron2.prepare_data, per row -- evaluation only, no gradient.  mel_target, decoder_output,
 * mel: [B, T, 80]; gate_target, stop_tokens: [B, T].  kinds: HOST int32 [n_kinds], 1 .. 4 distinct TTS_HIP_LOSS_* in the
 * caller's order (the reference's `mel_loss` list).  out: float32 [K, B], K = 2 + 2 n_kinds, rows in the order of the
 * reference's output_names: loss, one <kind>_mel_loss per kind (on decoder_output), one <kind>_mel_postnet_loss per kind (on
 * mel), gate_loss.  Per row b:
 *   mask[t] = 1 - gate_target[b, t] if mask_mel_padding (a float weight on the error, not a branch: targets need not be 0 / 1);
 *   e = (y - p)^2 (mse kinds) or |y - p| (mae kinds), times w = (y - ymin + 1) / (ymax - ymin + 1) for the weighted kinds,
 *       ymin / ymax over all T x 80 values of the row's mel_target, padded frames included;
 *   mel loss = sum_t(mask[t] sum_c e) / (80 sum_t mask[t]), 0 where that divisor is 0 (divide_no_nan); unmasked: sum e / (80 T);
 *   gate loss = (1 / T) sum_t bce[t] (g finish_weight + (1 - g) not_finish_weight) -- over the padded length T -- with
 *       bce = max(x, 0) - x g + log1p(exp(-|x|)) if from_logits, else -(g log o + (1 - g) log(1 - o)) on
 *       o = clip(x, float32(1e-7), float32(1 - 1e-7)) (the engine's stop_tokens are sigmoid outputs: from_logits = 0);
 *   loss = gate loss + every mel loss + every postnet mel loss.
 * Specified for finite inputs only (the mask multiplies, so a non-finite value in a masked frame propagates, as in the
 * reference).  One reduction pass: no floating-point atomics, partial sums in float64, a row's result independent of the
 * rows beside it (bit for bit at the same T).  The five inputs and `out` live where `mem` says; device pointers to the
 * three [B, T, 80] arrays must be 16-byte aligned.  Needs no weights: a handle that is not finalized is accepted.  Refused,
 * first match wins: a NULL pointer, B or T < 1, B * T > 65536, n_kinds outside 1 .. 4, an unknown or repeated kind, a bad
 * mem kind, a non-finite or negative weight, a misaligned device pointer.  Synchronizes `stream` (NULL: the handle's) before
 * returning.                                                                                                            */
enum { TTS_HIP_LOSS_MSE = 0, TTS_HIP_LOSS_MAE = 1, TTS_HIP_LOSS_WEIGHTED_MSE = 2, TTS_HIP_LOSS_WEIGHTED_MAE = 3 };
int tts_hip_tacotron2_loss(tts_hip_engine* e, const float* mel_target, const float* gate_target, const float* decoder_output,
                           const float* mel, const float* stop_tokens, int B, int T, const int32_t* kinds, int n_kinds,
                           int mask_mel_padding, int from_logits, double finish_weight, double not_finish_weight, float* out,
                           int mem, void* stream);
/* Mel-cepstral distortion of two ragged batches of log-mels along a dynamic-time-warping path (MCD-DTW), per row: what a
 * free-running synthesis is compared with its recording by.  a: [B, Ta, n_mel], b: [B, Tb, n_mel], float32 log-mels; len_a,
 * len_b: HOST int32 [B], each in 1 .. Ta / 1 .. Tb, NULL = every row full.  Nothing at or behind a row's length is read (a NaN
 * there reaches no output).  flags: TTS_HIP_DTW_ALIGN | TTS_HIP_DTW_C0.  Per row, la = len_a[b], lb = len_b[b]:
 *   cepstra   c[r] = sum_k D[r][k] m[k], D the orthonormal DCT-II, D[r][k] = sqrt(2 / n_mel) cos(pi (k + 1/2) r / n_mel), row 0
 *             divided by sqrt 2; rows 1 .. n_cep are used, rows 0 .. n_cep with TTS_HIP_DTW_C0.  The table is computed on the
 *             host in float64, rounded once to float32 and kept on the handle per (n_mel, n_cep, c0).  These are the DCT of
 *             the model's own log-mel, not WORLD / SPTK mel-cepstra.
 *   distance  d(i, j) = sqrt(sum_r (ca[i][r] - cb[j][r])^2)
 *   ALIGN     C(0, 0) = d(0, 0); C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1)), a missing neighbour = +inf, all
 *             three steps of unit weight; one float32 add per cell, and min is exact, so C does not depend on how the cells
 *             are spread over the machine.  The step code of a cell is the argmin: 0 diagonal, 1 from (i-1, j), 2 from
 *             (i, j-1), ties resolved in that order (cell (0, 0): 0).  cost = C(la-1, lb-1); the path is the backtrack from
 *             that cell along the step codes, path_len its number of cells.
 *   no ALIGN  the path is the diagonal (t, t), t < min(la, lb) = path_len; cost = sum_t d(t, t) (float64 sum, rounded once).
 *   mcd       (10 sqrt 2 / ln 10) cost / path_len, in dB.
 * stats: float32 [3, B] = cost, path_len, mcd.  path: NULL or int32 [B, Ta + Tb - 1, 2], the pairs (i, j) from (0, 0)
 * onwards, -1 behind the path's end.  a, b, stats and path live where `mem` says.  A row's results do not depend on the rows
 * beside it or on `mem`, bit for bit.  Needs no weights.  Refused (TTS_HIP_EINVAL, first match wins, nothing copied or
 * launched; csrc/mel_dtw_call.h): a NULL a, b or stats; B, Ta or Tb < 1; n_mel outside 2 .. 128; n_cep outside
 * 1 .. n_mel - 1; unknown flag bits; a bad mem kind; a length outside its range; Ta or Tb > 8192; B * Ta * Tb > 2^25 cells
 * (the aligned programme keeps 10 bytes per cell: 320 MiB of workspace at the limit); B * (Ta + Tb) > 2^19 frames (cepstra and
 * a host caller's staged mels, up to 512 bytes per frame each: 256 MiB each at the limit -- the workspace of an accepted call
 * stays below 840 MiB whatever its shape, path and tables included).  Synchronizes `stream` (NULL: the
 * handle's) before returning.
 * Test hook mel_dtw_probe: the same arguments, runs the aligned programme up to the stage `what` and returns it dense, zeros
 * at and behind the lengths: TTS_HIP_DTW_CEPSTRA_A [B, Ta, R], CEPSTRA_B [B, Tb, R] (R = n_cep, + 1 with C0), DISTANCE, COST,
 * STEP [B, Ta, Tb] (step codes as float32).  Any other `what` is TTS_HIP_EINVAL, after the mem kind.                       */
enum { TTS_HIP_DTW_ALIGN = 1, TTS_HIP_DTW_C0 = 2 };
enum { TTS_HIP_DTW_CEPSTRA_A = 0, TTS_HIP_DTW_CEPSTRA_B = 1, TTS_HIP_DTW_DISTANCE = 2, TTS_HIP_DTW_COST = 3, TTS_HIP_DTW_STEP = 4 };
int tts_hip_mel_dtw(tts_hip_engine* e, const float* a, const float* b, int B, int Ta, int Tb, int n_mel, const int32_t* len_a,
                    const int32_t* len_b, int n_cep, int flags, float* stats, int32_t* path, int mem, void* stream);
int tts_hip_mel_dtw_probe(tts_hip_engine* e, const float* a, const float* b, int B, int Ta, int Tb, int n_mel,
                          const int32_t* len_a, const int32_t* len_b, int n_cep, int flags, int what, float* out, int mem,
                          void* stream);
/* Pitch of a ragged batch of recordings, YIN (de Cheveigne & Kawahara 2002, steps 1 to 5).  audio: [B, N] float32; lengths:
 * HOST int32 [B], each in 1 .. N, NULL = every row full; W = win.  Row b has F_b = 1 + lengths[b] / hop frames of the
 * F = 1 + N / hop the output holds; for 1024 samples or more and hop = 256 that is the frame count of the default mel plan, so
 * a track lines up with the mel's frames.  Frame t reads x[s + j], j = 0 .. W + tau_max - 1, s = t * hop - W / 2; a sample
 * outside [0, lengths[b]) reads as 0.  Nothing at or behind a row's length is read (a NaN there reaches no output).
 *   difference   d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2, tau = 0 .. tau_max: a direct float32 sum of non-negative
 *                terms in the order of j (no autocorrelation, nothing cancels).
 *   normalised   S(tau) = sum_{k = 1 .. tau} d(k);  d'(0) = 1;  d'(tau) = d(tau) * tau / S(tau), or 1 where S(tau) = 0
 *                (silence and DC come out unvoiced).
 *   pick         the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; then, while tau + 1 <= tau_max and
 *                d'(tau + 1) < d'(tau), tau advances by one: that is tau*, and the frame is voiced.  If no tau qualifies the
 *                frame is unvoiced and tau* is the argmin of d' over [tau_min, tau_max], the smallest tau on ties.
 *   interpolate  a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1); if both neighbours lie in [1, tau_max] and a - 2b + c > 0,
 *                delta = (a - c) / (2 (a - 2b + c)), else 0: computed in double from the three float32 values, as are
 *                period = tau* + delta and f0 = rate / period, each rounded once to float32.
 * out: float32 [3, B, F] = f0 in Hz (0 where unvoiced), period in samples (also of unvoiced frames), aperiodicity = d'(tau*)
 * bit for bit; zeros at and behind F_b.  audio and out live where `mem` says.  A row's results do not depend on the rows
 * beside it or on `mem`, bit for bit.  Needs no weights.  Refused (TTS_HIP_EINVAL, first match wins, nothing copied or
 * launched; csrc/pitch_call.h): a NULL audio or out; B or N < 1; rate < 1; hop outside 1 .. win; win outside 2 .. 2048;
 * tau_min < 1, tau_min >= tau_max or tau_max > 1024; a threshold outside (0, 1]; a bad mem kind; a length outside 1 .. N;
 * N > 2^24; a buffer of the call at or above 2^31 bytes.  Synchronizes `stream` (NULL: the handle's) before returning.
 * Test hook pitch_probe: the same arguments, returns the stage `what` dense, zeros at and behind F_b: TTS_HIP_PITCH_DIFF (d)
 * and TTS_HIP_PITCH_CMND (d') [B, F, tau_max + 1], TTS_HIP_PITCH_PICK [2, B, F] (the voiced flag and tau* as float32).  Any
 * other `what` is TTS_HIP_EINVAL, after the mem kind; the buffer limit covers the probe's result.                            */
enum { TTS_HIP_PITCH_DIFF = 0, TTS_HIP_PITCH_CMND = 1, TTS_HIP_PITCH_PICK = 2 };
int tts_hip_pitch(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop, int win,
                  int tau_min, int tau_max, float threshold, float* out, int mem, void* stream);
int tts_hip_pitch_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop, int win,
                        int tau_min, int tau_max, float threshold, int what, float* out, int mem, void* stream);
/* Pitch of a ragged batch of recordings, probabilistic YIN (Mauch & Dixon 2014; the Boltzmann prior over the trough index is
 * left out): every trough of d' is a pitch candidate with a probability, and a Viterbi decode over pitch bins x {voiced,
 * unvoiced} chooses the track and the voicing.  Frames, d and d' are those of tts_hip_pitch, bit for bit.
 *   troughs      lag tau in [tau_min, tau_max] is a trough when d'(tau) < d'(tau - 1) (d'(0) = 1) and (tau = tau_max or
 *                d'(tau) <= d'(tau + 1)).
 *   thresholds   s_i = float32(i) / float32(n_thresh), i = 1 .. n_thresh; prior: HOST float32 [n_thresh], the mass of each
 *                threshold; cum(k) = prior[0] + ... + prior[k - 1] in double, rounded once to float32.
 *   probability  troughs by ascending lag, m = the smallest d' of the troughs before (+inf for the first): a trough with
 *                d' < m takes p = the prior of the thresholds with d' < s_i <= m, computed as cum(#{s_i <= m}) - cum(#{s_i <=
 *                d'}) in float32 (comparisons in float32 on the float32 d'); any other trough p = 0.  The trough of smallest d'
 *                (smallest lag on ties) adds no_trough_prob * cum(#{s_i <= d'}), product and sum rounded to float32.
 *   period, bin  a trough's delta is the interpolation of tts_hip_pitch (so |delta| <= 1/2), period = tau + delta, f = rate /
 *                period, pos = 12 bps log2(f / fmin), all in double; bin = clip(floor(pos + 1/2), 0, n_bins - 1).
 *   observation  obs[t, j] = the sum of p over the troughs of bin j by ascending lag in float32; cand[t, j] = float32(period)
 *                of the bin's trough of largest p (smallest lag on ties), 0 if the bin has none.  v_t = min(sum_j obs[t, j],
 *                1) (a fixed tree of float32 sums).  log-observations: log(max(obs[t, j], 2^-100)) of voiced state j, log(max((1 -
 *                v_t) / n_bins, 2^-100)) of every unvoiced state.
 *   states       0 .. n_bins - 1 voiced, n_bins .. 2 n_bins - 1 unvoiced.  Bins i -> j: w = max(0, max_step + 1 - |i - j|)
 *                over the sum of w over the bins j of the range; times 1 - switch_prob where voicing is kept, switch_prob where it
 *                changes.  The tables log w, log norm(i), log(1 - switch_prob), log(switch_prob) are computed in double and
 *                rounded once.  The initial distribution is uniform and dropped.
 *   decode       delta_0(j) = logobs_0(j); delta_t(j) = logobs_t(j) + max_i [((delta_{t-1}(i) - log norm(i)) + log w(i, j)) +
 *                log keep-or-switch] in float32, the smallest predecessor index on ties; after every frame the frame's maximum
 *                is subtracted.  The last state is the argmax (smallest index on ties); the path follows the stored
 *                predecessors.  Only a row's own F_b frames are decoded.
 * out: float32 [3, B, F] = f0 in Hz (0 where the decoded state is unvoiced; else rate / cand[t, j] of the decoded bin j, or
 * the bin's centre fmin 2^(j / (12 bps)) where the bin has no candidate; computed in double, rounded once), the same pitch of
 * the decoded bin whether voiced or not, v_t; zeros at and behind F_b.  audio and out live where `mem` says.  A row's results
 * do not depend on the rows beside it or on `mem`, bit for bit: no floating-point atomics.  Needs no weights.  Refused
 * (TTS_HIP_EINVAL, first match wins, nothing copied or launched; csrc/pitch_call.h): everything tts_hip_pitch refuses, in its
 * order; n_bins outside 1 .. 1024; bps outside 1 .. 100; max_step outside 1 .. n_bins; n_thresh outside 1 .. 1024; a NULL prior;
 * a prior entry that is not finite or negative; switch_prob outside (0, 1); no_trough_prob outside [0, 1]; fmin not finite and
 * positive; a buffer of the call (out, the observations, the uint16 backpointers [B, F, 2 n_bins]) at or above 2^31 bytes.
 * Synchronizes `stream` (NULL: the handle's) before returning.
 * Test hook pyin_probe: the same arguments, returns the stage `what` dense, zeros at and behind F_b: TTS_HIP_PYIN_TROUGH (p per
 * lag) [B, F, tau_max + 1], TTS_HIP_PYIN_OBS [2, B, F, n_bins] (obs, cand), TTS_HIP_PYIN_DELTA [B, F, 2 n_bins] (after the
 * frame's maximum is subtracted), TTS_HIP_PYIN_BACK [B, F, 2 n_bins] (the predecessor state as float32; frame 0: the state
 * itself), TTS_HIP_PYIN_PATH [B, F] (the decoded state as float32).  Any other `what` is TTS_HIP_EINVAL, after fmin.          */
enum { TTS_HIP_PYIN_TROUGH = 0, TTS_HIP_PYIN_OBS = 1, TTS_HIP_PYIN_DELTA = 2, TTS_HIP_PYIN_BACK = 3, TTS_HIP_PYIN_PATH = 4 };
int tts_hip_pyin(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop, int win,
                 int tau_min, int tau_max, const float* prior, int n_thresh, float no_trough_prob, double fmin, int bps, int n_bins,
                 int max_step, float switch_prob, float* out, int mem, void* stream);
int tts_hip_pyin_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int hop, int win,
                       int tau_min, int tau_max, const float* prior, int n_thresh, float no_trough_prob, double fmin, int bps,
                       int n_bins, int max_step, float switch_prob, int what, float* out, int mem, void* stream);
/* Two F0 tracks compared along a path, per row: F0 RMSE, voicing error and gross pitch error, the figures reported beside
 * MCD-DTW.  f0_a: [B, Fa], f0_b: [B, Fb] float32 in Hz; a frame is voiced iff its value is > 0 (a NaN is unvoiced).  len_a,
 * len_b: HOST int32 [B], each in 1 .. Fa / 1 .. Fb, NULL = every row full.  path: NULL = the diagonal (t, t), t < min(la, lb);
 * else int32 [B, P, 2] as tts_hip_mel_dtw writes it, living where `mem` says: a row's path ends at its first pair with a
 * negative index or an index at or beyond its row's frames (i >= la or j >= lb), so a malformed path can shorten a result
 * but never cause a read out of range.  Over the pairs (i, j) of a row, with c = 1200 log2(f0_a[i] / f0_b[j]) in double:
 *   stats: float32 [6, B] = pairs; voiced_pairs (both frames voiced); rmse_cents = sqrt(mean c^2) and mean_cents = mean c over
 *   the voiced pairs (0 where there are none); vuv_errors (exactly one frame voiced); gross_errors (both voiced and
 *   |c| > gross_cents).  Sums in double, rounded once; counts exact.
 * A row's results do not depend on the rows beside it or on `mem`, bit for bit.  Refused (TTS_HIP_EINVAL, first match wins;
 * csrc/pitch_call.h): a NULL f0_a, f0_b or stats; B, Fa or Fb < 1; with a path, P < 1; a gross_cents that is not finite and
 * positive; a bad mem kind; a length outside its range; Fa or Fb > 8192; with a path, P > Fa + Fb; B * (Fa + Fb) > 2^19.
 * Synchronizes `stream` (NULL: the handle's) before returning.                                                                */
int tts_hip_f0_error(tts_hip_engine* e, const float* f0_a, const float* f0_b, int B, int Fa, int Fb, const int32_t* len_a,
                     const int32_t* len_b, const int32_t* path, int P, float gross_cents, float* stats, int mem, void* stream);
/* Runs the encoder for another token batch INTO an existing encoded batch (its device buffer is reused and only grows):
 * what a caller that synthesizes sentence after sentence wants -- no hipMalloc / hipFree per sentence, and the decoder's
 * cached step graphs (keyed by the buffer) survive from one sentence to the next.  Asynchronous like `encode`.        */
int tts_hip_tacotron2_reencode(tts_hip_engine* e, tts_hip_encoded* encoded, const int32_t* tokens, int B, int Tin,
                               const float* speaker, int mem, void* stream);
int tts_hip_encoded_free(tts_hip_engine* e, tts_hip_encoded* encoded);

/* How the autoregressive loop (tacotron2_arch.py:710-735, K.while_loop) is executed.  mode 1: one persistent,
 * weight-stationary persistent kernel for the whole loop when the call shape allows it (batch <= 4, B * Tin small enough
 * for LDS, a device with >= 256 CUs that can host the whole grid); mode 2: the fused two-kernel step (batch <= 8, at most
 * 256 tokens; csrc/taco_fused.hip); mode 3 (default): persistent for 1 - 2 rows, fused for 3 - 8, whichever applies
 * otherwise; mode 0 -- and the fallback of every other mode -- one hipGraph of 7 kernels per decoder step.  All give the
 * same results up to fp32 re-association.                                                                              */
int tts_hip_set_decoder_mode(tts_hip_engine* e, int mode);
/* Which one the last tts_hip_tacotron2_infer* call on this handle used: 2 fused step, 1 persistent kernel, 0 per-step graph
 * (also after a fallback), -1 before the first call.                                                                          */
int tts_hip_last_decoder_mode(const tts_hip_engine* e);

/* Test hooks of the encoder and postnet convolutions (no effect on later calls; used by tests/, and probe_postnet what 5 by
 * `predict(batch_backlog=...)` to give a row cut at its own frame cap the postnet of its own frames).  Both run the code of
 * tts_hip_tacotron2_infer, not a copy, up to a stop point and copy what it computed there to `out` (fp32):
 * probe_encoder: the encoder of `tokens` [B, Tin] (+ speaker, as tts_hip_tacotron2_encode; B <= 1024, Tin <= 4096) --
 *   what 0 .. 2: output of encoder conv 1 .. 3 (MaskedConv1D -> BN -> relu), [B, Tin, 512], padded positions stored as 0;
 *   what 3: memory [B, Tin, enc] (BiLSTM output, then the speaker columns at 512 .. enc); what 4: processed memory
 *   [B, Tin, 128] (memory @ memory_layer).
 * probe_postnet: the postnet + residual on caller `frames` [B, T, 80] (in place of the decoder output) with `lengths` [B]
 *   (int32, HOST memory in every mode; mask t <= lengths[b], as after the decoder loop; B <= 1024, B * T <= 2^18) --
 *   what 0 .. 3: output of postnet conv 1 .. 4 (tanh), [B, T, 512], masked positions stored as 0; what 4: conv 5 (the
 *   residual, no activation), [B, T, 80], masked positions BN(0); what 5: mel = frames + residual, [B, T, 80].          */
int tts_hip_tacotron2_probe_encoder(tts_hip_engine* e, const int32_t* tokens, int B, int Tin, const float* speaker, int what,
                                    float* out, int mem);
int tts_hip_tacotron2_probe_postnet(tts_hip_engine* e, const float* frames, int B, int T, const int32_t* lengths, int what,
                                    float* out, int mem);
/* How each k = 5 conv + folded batch-norm last ran on this handle (encode, decode or probe): bit i set = one GEMM over the five
 * shifted segments with bias, row mask and activation in its epilogue ("single pass", 512 output tiles of 64 x 64 or more),
 * clear = one GEMM per tap into a scratch buffer plus a reduction pass ("split").  Bits 0 - 2: encoder convs 1 - 3, bits
 * 3 - 7: postnet convs 1 - 5; a conv that has not run yet reads 0.  -1 before the first conv.                             */
int tts_hip_last_conv_paths(const tts_hip_engine* e);

/* ---- WaveGlow forward flow: audio -> z and the terms of its log-likelihood (Prenger et al. 2018, section 2; the direction the
 * published model is trained and scored with, which the reference's `call` does not contain: waveglow_arch.py:241-242).
 * fp32, at both model widths, in the form tts_hip_set_waveglow_form selects for a call of B * T frames.
 *   audio [B, T*256], mel [B, T, 80]; `lengths` NULL or host int32 [B] in [0, T] (read before the call returns).
 *   z [B, T*32, 8] in exactly the layout tts_hip_waveglow_infer* consumes (channels 0..3 the final state, 4..5 what left before
 *     flow 8, 6..7 what left before flow 4): tts_hip_waveglow_infer(mel, z, sigma = 1) returns the audio.
 *   stats [3, B], per row over its real positions: stats[0] = sum z^2 (all 8 channels), stats[1] = sum over flows, positions
 *     and coupling channels of s, stats[2] = lengths[b] * 32 * sum_k log |det kernel_k[0]|.  The negative log-likelihood per
 *     sample under N(0, sigma^2) is (stats[0] / (2 sigma^2) - stats[1] - stats[2]) / (lengths[b] * 256).
 *   z or stats may be NULL (not both).  With lengths: audio and mel beyond a row's length are never read by a kernel, z is 0
 *   there, and a row gets what a call on its own frames gives it (the contract of tts_hip_waveglow_infer_ragged).
 * The sums use no floating-point atomics and float64 partial sums in a fixed order: repeats are bit-equal.
 * `mem`, `stream`, and when the call returns: the shared contract of the tts_hip_waveglow_infer* block.  Refused with
 * TTS_HIP_EINVAL before anything is copied or launched, the message starting with the symbol's name, first match wins: bad
 * `mem`; B <= 0; audio or mel NULL, or T <= 0; z and stats both NULL; a lengths[b] outside [0, T]; B * T above one run
 * (31 744 frames: the call is one run, slice the batch by rows).  The stop points of tts_hip_waveglow_probe belong to the
 * inverse direction and never apply here; this direction's test hook is tts_hip_waveglow_encode_probe below.            */
int tts_hip_waveglow_encode(tts_hip_engine* e, const float* audio, const float* mel, int B, int T, const int32_t* lengths,
                            float* z, float* stats, int mem);
int tts_hip_waveglow_encode_async(tts_hip_engine* e, const float* audio, const float* mel, int B, int T, const int32_t* lengths,
                                  float* z, float* stats, void* stream);

/* How the fp32 WaveGlow path evaluates the k = 3 dilated convolution of WN layers 1 .. 7 (waveglow_arch.py:117-127).
 * form 1 (default): Winograd minimal filtering along the tap axis for calls of 144 frames or more (any utterance length;
 * csrc/wn_wino.hip) -- F(4,3), six products per four outputs: K per output ~800 + 320 instead of 1536 + 320, fp32 operands
 * and accumulators, ONE kernel per layer (input transform in the operand reads, the six products as accumulator sets of one
 * block, output transform + gate in the epilogue); results within fp32 rounding of the direct form (6.0e-7 vs 5.0e-7
 * waveform RMS error against the oracle);
 * form 0: always the direct form;
 * forms 2, 3 (measurement only, same results as form 1): the three-pass form of round 3 (pre-pass, per-product GEMM, combine
 * pass) and the fused GEMM behind the pre-pass.
 * The Winograd form exists for 512-channel models only: on a 256-channel handle (tts_hip_waveglow_channels) the call is
 * accepted and has no effect -- every fp32 call takes the direct form.                                                  */
int tts_hip_set_waveglow_form(tts_hip_engine* e, int form);
/* Which one the last tts_hip_waveglow_infer* call on this handle used: 1 Winograd, 0 direct, -1 before the first call.  */
int tts_hip_last_waveglow_form(const tts_hip_engine* e);
/* n_channels (the WN width C) of this handle's WaveGlow: 512 or 256, fixed by the tensors present at tts_hip_finalize
 * (waveglow/block-0/start_conv/kernel [1, 4, C]; any other width, or a tensor that disagrees with it, fails finalize with
 * TTS_HIP_EINVAL).  0 while no WaveGlow is finalized and for a NULL handle.  Handles of both widths may live in one process. */
int tts_hip_waveglow_channels(const tts_hip_engine* e);

/* Test hook (used by tests/ only; no effect on later calls): runs the fp32 path of tts_hip_waveglow_infer -- in the form
 * selected by tts_hip_set_waveglow_form -- up to WN layer `layer` (0 .. 7) of flow `flow` (flows run 11 .. 0) and copies that
 * layer's gated activations tanh(.) * sigmoid(.) (waveglow_arch.py:19-24,117-127), i.e. the values BEFORE the res/skip and
 * `end` convolutions attenuate an error, to `acts` [B, T*32, C] (C = tts_hip_waveglow_channels) in the reference's position
 * order.  B*T <= 31744.                                                                                                  */
int tts_hip_waveglow_probe_acts(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma, int flow,
                                int layer, float* acts, int mem);
/* Test hook, any precision (used by tests/ only; no effect on later calls): runs tts_hip_waveglow_infer in `precision`
 * (0 f32 in the form tts_hip_set_waveglow_form selects, 1 f16, 2 f16x3) up to a stop point of flow `flow` (11 .. 0):
 *   what 0: the gated activations of WN layer `layer` (0 .. 7), as tts_hip_waveglow_probe_acts, to `out` [B, T*32, C] fp32
 *           (f16: the fp16 activations widened; f16x3: hi + lo summed in fp32);
 *   what 1: the flow state right after the flow (affine coupling, inverse 1x1 conv, and the early output that flows 8 and 4
 *           prepend), to `out` [B, T*32, n] with n = 4, 6 (flow 8), 6, 8 (flow 4), 8 for flows 11-9, 8, 7-5, 4, 3-0 --
 *           the channel order of the reference's audio after that flow (waveglow_arch.py:284-304); `layer` is not used;
 *   what 2: (precision 0 only) the conditioning plane that the Winograd form builds for WN layer `layer` (1 .. 7) -- the
 *           layer's conditioning term plus its in-layer bias, columns in the engine's gate-interleaved order (64 j + c: tanh
 *           channel 32 j + c, 64 j + 32 + c: its sigmoid channel) -- to `out` [B, T*32, 1024]; an error when the call does
 *           not take the Winograd form (fewer than 144 frames, form 0, a 256-channel model).
 * B*T <= 31744.                                                                                                            */
int tts_hip_waveglow_probe(tts_hip_engine* e, const float* mel, int B, int T, const float* z, float sigma, int precision,
                           int flow, int what, int layer, float* out, int mem);
/* The same test hook for calls with row lengths (used by tests/ only; no effect on later calls); the two symbols above are
 * calls of this one with lengths NULL and packed 0, bit for bit.  `lengths`: NULL or host int32 [B] in [0, T].
 *   lengths, packed 0: the ONE run of tts_hip_waveglow_infer_ragged on these arguments (the same table, staged the same way),
 *     stopped at the probe; `out` [B, T*32, W] in the batch layout, W as above.  what 1: `out` is exactly 0 behind a row's
 *     length.  what 0 and 2: what lies behind a row's length is whatever the run computed there -- NOT SPECIFIED.
 *   packed != 0 (needs lengths): the gather of tts_hip_waveglow_infer_packed, then its one-row run with per-frame flags,
 *     stopped at the probe; there is no scatter.  `out` [F*32, W] in the packed row's OWN layout, F = sum(lengths) +
 *     TTS_HIP_WG_GAP_FRAMES * (rows with frames - 1): row b's frames start at frame sum over the rows before it that hold
 *     frames of (their length + the gap).  what 1: `out` is exactly 0 on gap frames; what 0 and 2: not specified there.  F = 0:
 *     nothing is written.
 * mel and z behind a row's length are never read.  Refused with TTS_HIP_EINVAL before anything is copied or launched, the
 * message starting with the symbol's name (also for the two symbols above), first match wins (csrc/wg_call.h,
 * wg_probe_check): whatever tts_hip_waveglow_infer_ragged / _packed refuses of the same mel / B / T / lengths / packed /
 * precision / mem, then flow outside [0, 11], what outside [0, 2], layer outside [0, 7], what 2 with precision != 0, B * T
 * (packed: F) above one run (31 744 frames: the probe does not slice), out NULL.                                          */
int tts_hip_waveglow_probe_rows(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths, int packed,
                                const float* z, float sigma, int precision, int flow, int what, int layer, float* out, int mem);
/* Test hook of the forward direction (used by tests/ only; no state is kept on the handle, so no effect on later calls):
 * runs tts_hip_waveglow_encode on audio / mel / lengths -- same plan, form and fall-back, same tail handling -- and stops
 * after the position-wise kernel that ends flow `flow` (0 .. 11; -1: right after the init step audio @ kernel_0):
 *   what 0: the flow state AS STORED, to `out` [B, T*32, n] in the reference's position order: what flow `flow` + 1 reads,
 *           i.e. the early channels already gone and that flow's matrix already applied; n = 8 for flows -1 .. 2, 6 for
 *           3 .. 6, 4 for 7 .. 10.  After flow 11 nothing is stored: `out` [B, T*32, 4] gets z's channels 0 .. 3;
 *   what 1: the running sum over flows 0 .. `flow` and coupling channels of s, per position, to `out` [B, T*32].
 * With lengths, `out` is exactly 0 behind a row's length.  tts_hip_last_waveglow_form / _tiles report what ran.  Refused with
 * TTS_HIP_EINVAL before anything is copied or launched, the message starting with the symbol's name: whatever
 * tts_hip_waveglow_encode refuses (its two outputs aside), then flow outside [-1, 11], what outside [0, 1], what 1 with
 * flow -1, out NULL.                                                                                                    */
int tts_hip_waveglow_encode_probe(tts_hip_engine* e, const float* audio, const float* mel, int B, int T, const int32_t* lengths,
                                  int flow, int what, float* out, int mem);
/* WN GEMM tile family the last tts_hip_waveglow_infer* (or probe) call on this handle used for its in-layer (direct form) and
 * residual GEMMs: 3 64-row tiles (64 x 128), 2 128 x 64 tiles, 1 128-row tiles, 0 256-row tiles (fp16: 256 x 256), -1 before
 * the first call.  Split fp16 (f16x3) has two families only: 3 and 0.                                                    */
int tts_hip_last_waveglow_tiles(const tts_hip_engine* e);

/* ---- WaveGlow.infer on a batch of unequal rows
 * Row b holds lengths[b] (0 <= lengths[b] <= T) real frames; lengths NULL = T for every row: then the call IS
 * tts_hip_waveglow_infer* / _async (same kernels, same launches, bit-equal audio).  With lengths, in every precision and
 * every tile family:
 *   - audio[b, :lengths[b]*256] is what a one-row call on mel[b, :lengths[b]], z[b, :lengths[b]*32] returns, up to the fp32
 *     re-association that already separates tile families and forms (a padded row of the calls above is NOT: its WN
 *     convolutions read the padding where the row alone reads zeros, 3e-2 .. 5e-2 RMS on the row's samples);
 *   - audio[b, lengths[b]*256:] = 0 exactly;
 *   - nothing read beyond a row's length: mel[b, lengths[b]:] and z[b, lengths[b]*32:] may hold anything, NaN and Inf
 *     included (e.g. uninitialised padding), and two calls that differ only there return bit-equal audio.
 * T is what counts towards the limits, not the lengths: tail frames still occupy rows of the GEMMs.                      */
int tts_hip_waveglow_infer_ragged(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths, const float* z,
                                  float sigma, float* audio, int precision, int mem);
int tts_hip_waveglow_infer_ragged_async(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                        const float* z, float sigma, float* audio, int precision, void* stream);

/* ---- the same results, computed as ONE packed row
 * Arguments and results as tts_hip_waveglow_infer_ragged[_async] (lengths must not be NULL).  Only the way it is computed
 * differs: the real frames of all rows are laid one after
 * another in one row of F = sum(lengths) + TTS_HIP_WG_GAP_FRAMES * (rows with frames - 1) frames, separated by runs of zero
 * "gap" frames that are marked as not real (rows of length 0 take no space and no gap), and that row runs as an ordinary
 * one-row call -- the work follows the frames that exist, not B * max(lengths).  A gather builds the packed mel / z from
 * the batch layout and a scatter writes every sample of `audio` (zero tails included) from the packed result.
 * tts_hip_last_waveglow_form / _tiles then describe the packed run (B = 1, T = F).  The packed row is one run: F above
 * 31744 frames is TTS_HIP_EINVAL (the message names F and the limit; nothing is launched, and there is no fall-back to the
 * ragged call), while T alone is not limited.
 *
 * The gap length follows from the model.  A frame that is not real is held at 0 in the WN residual stream (after the start
 * conv and after every residual sum), in the first-layer operand, in the flow state and in the mel, so to its neighbours
 * it looks like the zero padding a run of the row alone has there.  One WN layer reaches at most 2^7 positions = 4 frames
 * to either side (kernel 3, dilation 2^i, i <= 7, 32 positions per frame) and the residual stream is re-zeroed after every
 * layer, so nothing travels further than that; the folded conditioning reads mel frames t-3 .. t.  With 4 gap frames no
 * tap of a real position lands on another row's frame; with 3 the dilation-128 taps do (numpy oracle, segments of 6, 1
 * and 5 frames: RMS against the solo runs 2.6e-7 with 4 gap frames, 1.2e-2 .. 5.5e-2 with 3; tests/test_waveglow_packed.py). */
#define TTS_HIP_WG_GAP_FRAMES 4
int tts_hip_waveglow_infer_packed(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths, const float* z,
                                  float sigma, float* audio, int precision, int mem);
int tts_hip_waveglow_infer_packed_async(tts_hip_engine* e, const float* mel, int B, int T, const int32_t* lengths,
                                        const float* z, float sigma, float* audio, int precision, void* stream);

/* ---- TacotronSTFT.mel_spectrogram  (utils/audio/stft.py:242-274,306-314)
 * audio [B, N] (N >= 1024) -> mel [B, N/256 + 1, 80]                                                                */
int tts_hip_mel_stft(tts_hip_engine* e, const float* audio, int B, int N, float* mel, int mem);
/* Test hook (no effect on later calls; used by tests/): runs the code of tts_hip_mel_stft, not a copy, on the same
 * arguments (and refuses the same ones) up to stage `what` and copies that stage's logical extent to `out` (fp32), with
 * F = N/256 + 1 frames per row --
 *   what 0: the reflect-padded rows [B, N + 1024]; what 1: the spectrum [B, F, 1026] (real parts of bins 0 .. 512, then
 *   the imaginary parts at 513 .. 1025); what 2: the magnitudes [B, F, 513]; what 3: the linear mel [B, F, 80], before
 *   log(max(., 1e-5)).  Any other `what` is TTS_HIP_EINVAL and launches nothing.                                        */
int tts_hip_mel_stft_probe(tts_hip_engine* e, const float* audio, int B, int N, int what, float* out, int mem);

/* ---- mel plans: any TacotronSTFT configuration and WhisperSTFT (utils/audio/stft.py:101-124, 242-274, 306-314, 350-364)
 * A plan holds the windowed-DFT basis and the Slaney filterbank of one configuration on the device.  It belongs to the
 * engine handle it was created on, needs no weights and no tts_hip_finalize, and is freed by tts_hip_mel_fn_free or with
 * the handle.  `window` is a HOST array of win_length doubles (get_window(name, win_length, fftbins=periodic)), NULL = the
 * periodic Hann window; it is centred in filter_length (pad_center: (filter_length - win_length) // 2 zeros before it).
 * tts_hip_mel_stft[_async, _probe] are calls on the handle's default plan: kind Tacotron, 22 050 Hz, 1024 / 256 / 1024,
 * 80 mels, 0 - 8000 Hz, no pre-emphasis, no normalisation.
 *
 * run: audio [B, N] -> mel [B, Fmax, n_mel_channels], Fmax = tts_hip_mel_fn_frames(fn, N).  Row b holds lengths[b]
 * (1 <= lengths[b] <= N) samples; `lengths` is a HOST array in every mode, NULL = N for every row.  Row b of the result is
 * what a one-row call on audio[b, :lengths[b]] returns, frames at and beyond tts_hip_mel_fn_frames(fn, lengths[b]) are 0,
 * and nothing at or beyond lengths[b] is read (it may hold NaN).  Per row of L samples:
 *   1. L' = max(L, win_length), zeros on the right;
 *   2. pre_emph > 0: y[0] = x[0], y[i] = x[i] - (float)pre_emph * x[i-1] (one fp32 product, one fp32 difference) on the L'
 *      samples, so the first padded zero becomes -pre_emph * x[L-1] as in the reference;
 *   3. numpy 'reflect' padding of filter_length // 2 on each side; F = (L' + 2 * (filter_length // 2) - filter_length)
 *      // hop_length + 1 frames;
 *   4. the windowed DFT as a GEMM against cos / -sin rows (phase reduced exactly, rounded to fp32, times the float64 window,
 *      rounded once), bins 0 .. filter_length // 2;
 *   5. magnitude sqrt(re^2 + im^2), times the Slaney filterbank of (sampling_rate, filter_length, n_mel_channels, mel_fmin,
 *      mel_fmax) built in double (librosa.filters.mel defaults);
 *   6. kind TACOTRON: log(max(., 1e-5)) in double, rounded once; then normalize_mode: PER_FEATURE (x - mean) / std per mel
 *      channel over the row's own F frames, ALL_FEATURE the same over the row's own F x n_mel cells -- the reference's
 *      all_feature reduces over the batch too; here a row's result never depends on its neighbours -- population std, 0
 *      where std is 0, sums / subtraction / division in double and rounded once;
 *   7. kind WHISPER: the row's last frame is dropped (F - 1 frames come out); log10(max(., 1e-10)) in double, rounded once;
 *      m = max(x, rowmax - 8.0f) with rowmax the fp32 maximum over the row's own cells; (m + 4.0f) / 4.0f in fp32;
 *      normalize_mode has no effect.
 * Refusals (TTS_HIP_EINVAL, first match wins, nothing copied or launched; csrc/audio_call.h) --
 *   create: NULL cfg / out; kind; normalize_mode; sampling_rate < 1; filter_length outside [2, 4096]; win_length outside
 *     [1, filter_length]; hop_length < 1; n_mel_channels outside [1, 1024]; not 0 <= mel_fmin < mel_fmax <= sampling_rate / 2;
 *     pre_emph negative or not finite; a window value that is not finite;
 *   run / probe: NULL fn / audio / mel, B < 1, N < 1; a lengths[b] outside [1, N]; a row whose L' is not above
 *     filter_length // 2 (reflect needs it); a Whisper row with F < 2; B > 65535 or one of the call's buffers at 2^31 - 65536
 *     bytes or more -- the padded rows [B][max(N, win_length) + 2 * (filter_length // 2) (+ up to 6)] fp32, the gathered
 *     frames [B * F][filter_length up to 32] (hop_length % 4 != 0 only), the spectrum [B * F][2 * bins up to 32], the
 *     magnitudes [B * F][bins up to 32], the linear mel [B * F][n_mel], audio, with F the frames of N; a bad mem kind; the
 *     probe's `what` outside 0 .. 4.
 * All plans of a handle share one workspace: an _async call must be ordered before the next mel call on the handle.
 * probe (test hook; runs the code of run, not a copy, up to a stage; F = the DFT frames of N, Whisper's last one included):
 *   what 0 `padded` [B, max(N, win_length) + 2 * (filter_length // 2)] after steps 1 - 3; 1 `spectrum` [B, F, 2 * bins]
 *   (real parts, then imaginary parts); 2 `magnitude` [B, F, bins]; 3 `mel_linear` [B, F, n_mel]; 4 `mel_log` [B, Fmax,
 *   n_mel] after the logarithm, before the normalisation / clamp (frames beyond a row's own already 0).  In stages 1 - 3 the
 *   frames beyond a row's own hold what the zero-padded row gives there.                                                  */
typedef struct tts_hip_mel_fn tts_hip_mel_fn;
enum { TTS_HIP_MEL_TACOTRON = 0, TTS_HIP_MEL_WHISPER = 1 };
enum { TTS_HIP_MEL_NORM_NONE = 0, TTS_HIP_MEL_NORM_PER_FEATURE = 1, TTS_HIP_MEL_NORM_ALL_FEATURE = 2 };
typedef struct {
    int kind, sampling_rate, n_mel_channels, filter_length, hop_length, win_length, normalize_mode;
    double mel_fmin, mel_fmax, pre_emph;
} tts_hip_mel_config;
int tts_hip_mel_fn_create(tts_hip_engine* e, const tts_hip_mel_config* cfg, const double* window, tts_hip_mel_fn** out);
int tts_hip_mel_fn_free(tts_hip_engine* e, tts_hip_mel_fn* fn);
/* frames a row of n_samples yields (the default plan: max(n, 1024) / 256 + 1); < 0 if run would refuse the row */
int tts_hip_mel_fn_frames(const tts_hip_mel_fn* fn, int n_samples);
int tts_hip_mel_fn_run(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                       float* mel, int mem);
int tts_hip_mel_fn_run_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths,
                             const tts_hip_mel_fn* fn, float* mel, void* stream);
int tts_hip_mel_fn_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                         int what, float* out, int mem);

/* ---- STFT with phase, its inverse, and Griffin-Lim (csrc/stft_inv.hip; utils/audio/stft.py:194-274, the STFT class).
 * All of these take a Tacotron-kind plan, are refused for a Whisper plan, and build the tables they need on first use.
 * With cut = filter_length / 2 + 1 bins, half = filter_length / 2:
 *
 * transform: audio [B, N], lengths as tts_hip_mel_fn_run -> out0, out1 [B, Fmax, cut], Fmax = tts_hip_mel_fn_frames(fn, N):
 *   steps 1 - 4 of the mel plan (zero pad, pre-emphasis, reflect pad, windowed DFT), then what = 0: magnitude
 *   sqrt(re^2 + im^2) and phase atan2f(im, re); what = 1: real and imaginary parts.  Frames at and beyond a row's own are 0.
 *
 * inverse: two planes [B, F, cut] (form 0: magnitude and phase, re = m cosf(p), im = m sinf(p); form 1: real and imaginary
 *   parts) and frames[b] in [1, F] (host array; NULL = F for every row) -> audio [B, F * hop_length].  Per row: time frames
 *   [re_f, im_f] . inverse_basis (filter_length samples; the windowed pseudo-inverse of stft.py:220-236), overlap-added at
 *   f * hop_length, y[i] /= ws[i] wherever ws[i] > FLT_MIN with ws[i] = sum_f window^2[i - f * hop_length] over the row's own
 *   frames, y *= filter_length / hop_length, and half samples dropped at each end: row b holds
 *   tts_hip_mel_fn_samples(fn, frames[b]) = hop_length * (frames[b] - 1) + filter_length - 2 * half samples, zeros beyond.
 *   Each output sample sums its frames in frame order (a gather, no atomics): the result is bit-reproducible, nothing
 *   behind a row's frames is read, and a row never depends on its neighbours.
 *
 * griffin_lim: spec [B, F, C] -> audio [B, F * hop_length].  input_kind 0: spec is the linear magnitude S, C = cut;
 *   1: spec is a Tacotron log-mel, C = n_mel_channels, S = max(0, exp(spec) . Minv) with Minv [n_mel, cut] a host double
 *   array (whatever `mem` says), NULL = the minimum-norm inverse W^T (W W^T)^-1 of the plan's filterbank (Cholesky in
 *   double; the call is refused when that fails -- a mel channel without a bin -- and for a plan that normalises).
 *   With P(re, im) = (re, im) / |(re, im)|, P(0, 0) = (1, 0): p_0 = P(init) (init [B, F, cut, 2]; NULL = (1, 0)),
 *   t_prev = 0, and n_iters times: x = inverse(S p); Y = transform(x) of the row's own samples (no pre-emphasis: a plan with
 *   pre_emph > 0 is refused; exactly frames[b] frames); c = Y - momentum / (1 + momentum) * t_prev; t_prev = Y; p = P(c).
 *   The result is inverse(S p); n_iters = 0 is a single inverse of the initial phase.  The _async form takes device
 *   pointers (Minv stays a host array) and a stream.
 *
 * griffin_lim_probe (test hook): the code of the call, not a copy, stopped at stage `what` of iteration k in [0, n_iters]:
 *   0 target S [B, F, cut]; 1 operand S p_k [B, F, 2 cut] (real parts, then imaginary parts); 2 frames [B, F, filter_length];
 *   3 signal [B, hop_length * (F - 1) + filter_length], the reflect-padded row of x_k; 4 spectrum Y_k [B, F, 2 cut];
 *   5 phasor p_{k+1} [B, F, 2 cut].  The call makes n_iters phase updates and then one more inverse: iteration k = n_iters is
 *   that last inverse (operand, frames, signal) and takes no transform, so it has no spectrum and no phasor -- stages 4 and 5
 *   exist for k < n_iters only and are refused at k = n_iters.
 *
 * Refusals (TTS_HIP_EINVAL, first match wins, nothing copied or launched): a plan that is not a plan of this handle
 * (checked first: nothing of a dead plan is read); a NULL pointer; B or F < 1; a frames[b] outside [1, F]; C not the plan's
 * width for the kind; n_iters < 0; momentum outside [0, 1) or not finite; a Whisper plan; pre_emph > 0 (griffin_lim); a
 * normalising plan (kind 1); a griffin_lim row whose samples are not more than half (the reflect needs them); a buffer at or
 * above 2^31 - 65536 bytes; a bad mem kind; a bad `what`, or k outside [0, n_iters]. */
long long tts_hip_mel_fn_samples(const tts_hip_mel_fn* fn, int frames);
int tts_hip_stft_transform(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                           int what, float* out0, float* out1, int mem);
int tts_hip_stft_inverse(tts_hip_engine* e, const float* plane0, int B, int F, const float* plane1, const int32_t* frames,
                         const tts_hip_mel_fn* fn, int form, float* audio, int mem);
int tts_hip_griffin_lim(tts_hip_engine* e, const float* spec, int B, int F, int C, const int32_t* frames, const tts_hip_mel_fn* fn,
                        int input_kind, const double* Minv, const float* init, int n_iters, double momentum, float* audio, int mem);
int tts_hip_griffin_lim_async(tts_hip_engine* e, const float* spec, int B, int F, int C, const int32_t* frames,
                              const tts_hip_mel_fn* fn, int input_kind, const double* Minv, const float* init, int n_iters,
                              double momentum, float* audio, void* stream);
int tts_hip_griffin_lim_probe(tts_hip_engine* e, const float* spec, int B, int F, int C, const int32_t* frames,
                              const tts_hip_mel_fn* fn, int input_kind, const double* Minv, const float* init, int n_iters,
                              double momentum, int k, int what, float* out, int mem);

/* ---- WaveGlow denoiser (csrc/stft_inv.hip): spectral subtraction of a model's bias spectrum, the phase kept.
 * A WaveGlow checkpoint fed a silent mel and no noise still emits a faint tonal hum; the published vocoder ships with a
 * denoiser that takes the magnitude spectrum of that hum once per model and subtracts strength x it from every frame.
 *
 * denoise: audio [B, N], lengths as tts_hip_mel_fn_run, bias [cut] >= 0 (follows `mem`; device memory for the _async form),
 *   strength >= 0 (used as s = (float)strength) -> out [B, N], under a Tacotron-kind plan:
 *   X = the transform's spectrum of every row (steps 1 - 4 of the mel plan: what tts_hip_mel_fn_probe returns as stage 1);
 *   per bin, with m = |X| taken from the pair scaled by its larger component: Y = max(m - s * bias[c], 0) * X / m, Y = 0
 *   where m = 0 (no atan2 / sin / cos); frames at and beyond a row's own are 0; out = inverse(Y) as tts_hip_stft_inverse
 *   computes it, cut to the row: row b holds min(lengths[b], tts_hip_mel_fn_samples(fn, frames_b)) samples, frames_b =
 *   tts_hip_mel_fn_frames(fn, lengths[b]), and zeros beyond.  A vocoder row of frames * 256 samples under the default
 *   geometry (1024 / 256 / 1024) gets back exactly its samples; a row shorter than win_length is zero-padded by the plan and
 *   cut back to its length.  Nothing behind a row's length is read, nothing is accumulated with atomics: a row is
 *   bit-equal to the row called alone and a repeat gives the same bits.  out == audio is allowed for device memory (the
 *   transform has consumed the audio before the overlap-add writes).  The transform runs in the mel workspace of the
 *   handle, the inverse in the inverse workspace, with no host round trip between them: the _async form (device pointers,
 *   a stream) does not synchronize.
 *
 * denoise_probe (test hook): the code of the call, not a copy, stopped after stage `what`, with F =
 *   tts_hip_mel_fn_frames(fn, N): 0 spectrum X [B, F, 2 cut] (real parts, then imaginary parts); 1 the gated operand Y
 *   [B, F, 2 cut]; 2 time frames [B, F, filter_length].  The call itself is the last stage.
 *
 * Refusals (TTS_HIP_EINVAL, first match wins, nothing copied or launched): a plan that is not a plan of this handle; a NULL
 * plan, audio or out, B or N < 1; a lengths[b] outside [1, N]; a row the reflect cannot pad (as tts_hip_mel_fn_run); a
 * Whisper plan; bias NULL; strength negative or not finite; a buffer at or above 2^31 - 65536 bytes or B > 65535; a bad
 * mem kind; a `what` outside 0 .. 2 (probe). */
int tts_hip_denoise(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                    const float* bias, double strength, float* out, int mem);
int tts_hip_denoise_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                          const float* bias, double strength, float* out, void* stream);
int tts_hip_denoise_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const tts_hip_mel_fn* fn,
                          const float* bias, double strength, int what, float* out, int mem);

/* ---- time stretch (csrc/stft_inv.hip): a phase vocoder with identity phase locking (Laroche and Dolson 1999) between the
 * transform and the inverse of a Tacotron-kind plan.  Only spectral peaks accumulate phase; every other bin keeps the
 * analysis-phase relation to its nearest peak, so the bins of one partial cannot drift apart when the rate is below 1.
 *
 * time_stretch: audio [B, N], lengths as tts_hip_mel_fn_run, rates [B] (HOST doubles in every mode) -> out [B, M].  With
 *   cut = filter_length / 2 + 1, row b of L_b samples at rate r_b (> 1 faster, < 1 slower):
 *   1. X_b[f][k], f < F_b = tts_hip_mel_fn_frames(fn, L_b), is the spectrum of steps 1 - 4 of the mel plan (stage 1 of
 *      tts_hip_mel_fn_probe); X_b[F_b][k] = 0.
 *   2. T_b is the smallest T with (double)T * r_b >= F_b; for t < T_b: pos = (double)t * r_b, i = floor(pos),
 *      a = (float)(pos - i).
 *   3. With c0 = X[i], c1 = X[i+1]: m[t][k] = (1 - a) * |c0[k]| + a * |c1[k]| in fp32, |z| = sqrtf(re * re + im * im), every
 *      operation rounded on its own (no fused multiply-add): two products, a sum and a square root per magnitude; the
 *      difference 1 - a, two products and a sum for m.  P(z) = z / |z|, P(0) = (1, 0) (taken from the pair scaled by its
 *      larger component; its products may be fused).  A[t][k] = P(c1[k] * conj(c0[k])), R[t][k] = P(c0[k] * conj(c0[own[t][k]])).
 *   4. k is a peak of frame t if m[t][k] > 0, m[t][k] > m[t][k-1], m[t][k] > m[t][k-2], m[t][k] >= m[t][k+1] and
 *      m[t][k] >= m[t][k+2]; neighbours outside 0 .. cut - 1 count as minus infinity.  own[t][k] is the nearest peak of frame
 *      t, a tie goes to the lower peak; a frame without a peak (all of its m are 0) has no owners.
 *   5. U[0][k] = P(X[0][k]); for t >= 1: U[t][k] = P(U[t-1][p] * A[t-1][p] * R[t][k]) with p = own[t][k] (the products in
 *      that order), and in a frame without peaks U[t][k] = U[t-1][k] * A[t-1][k].  Y[t][k] = m[t][k] * U[t][k].  No atan2,
 *      sin or cos; the chain re-normalises at every step.
 *   6. out_b = inverse(Y_b) exactly as tts_hip_stft_inverse computes it for T_b frames.  Row b of out holds S_b =
 *      llrint((double)L_b / r_b) samples (ties to even): the leading min(S_b, tts_hip_mel_fn_samples(fn, T_b)) come from the
 *      inverse, everything behind them is 0.  M must equal max_b S_b (and be >= 1).
 *   tts_hip_time_stretch_samples(fn, n, rate) = S and tts_hip_time_stretch_frames(fn, n, rate) = T of a row of n samples
 *   (host only); both are negative where the call would refuse the row, the rate or the plan.
 *   Nothing behind a row's length is read, nothing is accumulated with atomics: a row is bit-equal to the row called alone
 *   and a repeat gives the same bits.  rate = 1 gives a = 0, A = the analysis phase advance and the input's own phases up to
 *   rounding: the STFT round trip.  The transform runs in the mel workspace of the handle, the vocoder and the inverse in the
 *   inverse workspace, with no host round trip: the _async form (device pointers, a stream; lengths and rates stay host
 *   arrays) does not synchronize.
 *
 * time_stretch_probe (test hook): the code of the call, not a copy, stopped after stage `what`, with F =
 *   tts_hip_mel_fn_frames(fn, N) and T = max_b T_b: 0 spectrum X [B, F, 2 cut] (real parts, then imaginary parts); 1 m
 *   [B, T, cut]; 2 own as floats [B, T, cut], -1 where a frame has no peak; 3 operand Y [B, T, 2 cut]; 4 time frames
 *   [B, T, filter_length].  Output frames at and beyond T_b hold m = 0, own = -1, Y = 0.  The call itself is the last stage.
 *
 * Refusals (TTS_HIP_EINVAL, first match wins, nothing copied or launched; time_stretch_check in csrc/audio_call.h): a plan
 * that is not a plan of this handle; a NULL plan, audio, out or rates, B or N < 1; a lengths[b] outside [1, N]; a row the
 * reflect cannot pad (as tts_hip_mel_fn_run); a Whisper plan; pre_emph > 0 (the inverse does not undo it); a rate that is
 * not finite or lies outside [0.25, 4]; M not max_b S_b, or that below 1; a buffer at or above 2^31 - 65536 bytes or
 * B > 65535; a bad mem kind; a `what` outside 0 .. 4 (probe). */
long long tts_hip_time_stretch_samples(const tts_hip_mel_fn* fn, int n_samples, double rate);
int tts_hip_time_stretch_frames(const tts_hip_mel_fn* fn, int n_samples, double rate);
int tts_hip_time_stretch(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const double* rates,
                         const tts_hip_mel_fn* fn, float* out, int M, int mem);
int tts_hip_time_stretch_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const double* rates,
                               const tts_hip_mel_fn* fn, float* out, int M, void* stream);
int tts_hip_time_stretch_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const double* rates,
                               const tts_hip_mel_fn* fn, int what, float* out, int M, int mem);

/* ---- formant match (csrc/stft_inv.hip): the spectral envelope of one signal put onto another, the phases kept.
 * A pitch shift by resampling moves the vocal-tract resonances along with the harmonics; this call multiplies the shifted
 * signal's spectrum, on the same frame grid, by the ratio of the original's cepstrally smoothed envelope to its own.  Warping
 * the source envelope along frequency moves the formants with or without a pitch change.
 *
 * formant_match: audio [B, N] (the signal to correct), source [B, N] or NULL = the audio itself (the signal whose envelope is
 *   wanted; both follow `mem`, device memory for the _async form), lengths as tts_hip_mel_fn_run (they hold for both signals),
 *   warps [B] (HOST doubles in every mode, in [0.5, 2]; NULL = 1 for every row), the lifter cut Q = `lifter`,
 *   max_gain_db in (0, 60] -> out [B, N], under a Tacotron-kind plan.  With cut = filter_length / 2 + 1, n = filter_length,
 *   F_b = tts_hip_mel_fn_frames(fn, lengths[b]):
 *   1. X_b, Y_b are the spectra of source and audio: steps 1 - 4 of the mel plan (stage 1 of tts_hip_mel_fn_probe).  With
 *      source NULL there is one transform and X = Y.
 *   2. lx[f][k] = logf(max(|X[f][k]|, 1e-5f)) and ly the same from Y, |z| = sqrtf(re * re + im * im) with every operation
 *      rounded on its own (as step 3 of the time stretch); 1e-5 is the clip of the mel plan's logarithm.
 *   3. Sx = lx . L and Sy = ly . L with the liftering table L [cut, cut], L[j][k] = (w_j / n) * sum_{q = 0 .. Q} v_q
 *      cos(2 pi q j / n) cos(2 pi q k / n), w_0 = w_{cut-1} = 1 and v_0 = 1, every other weight 2: the real cepstrum of the even
 *      extension of a row, cut after quefrency Q, transformed back.  L is built on the host in double at first use for a
 *      (plan, Q), rounded once to fp32 and kept with the plan's tables (a call with another Q rebuilds it); both products are
 *      one fp32 GEMM over the 2 * B * F stacked rows, K = cut padded to a multiple of 32.
 *   4. Per row, beta = warps[b], per bin k: pos = (double)k / beta, i = floor(pos), a = (float)(pos - i);
 *      E[f][k] = (1 - a) * Sx[f][i] + a * Sx[f][i + 1] - Sy[f][k] in fp32, no fused multiply-add (the difference 1 - a, two
 *      products, a sum, a difference); where i >= cut - 1 the top bin is held: Sx[f][cut - 1] - Sy[f][k].  beta = 1 gives
 *      a = 0 and E = Sx - Sy exactly.
 *   5. g = expf(min(max(E, -G), G)), G = (float)(max_gain_db * ln(10) / 20).
 *   6. Per frame e0 = sum_k |Y[f][k]|^2 and e1 = sum_k (g[f][k] |Y[f][k]|)^2 over the cut bins, fp32, in a fixed order (one
 *      workgroup per frame, no atomics; products and sums not fused); s = sqrtf(e0 / e1), s = 1 where e1 == 0;
 *      gain = g * s.  The mean-log envelope of a higher-pitched voice sits lower between its sparser harmonics; s removes
 *      that bias and keeps every frame's energy.
 *   7. Y' = gain * Y, both components; frames at and beyond F_b are 0.
 *   8. out = inverse(Y') exactly as tts_hip_denoise finishes: row b holds min(lengths[b], tts_hip_mel_fn_samples(fn, F_b))
 *      samples and zeros beyond.
 *   source NULL with warps 1 gives E = 0, gain = 1 and Y' = Y bit for bit: the STFT round trip.  Nothing behind a row's
 *   length is read, in either signal; nothing is accumulated with atomics: a row is bit-equal to the row called alone and a
 *   repeat gives the same bits.  The transforms run one after the other in the mel workspace of the handle (the source's
 *   log-magnitudes are taken before the audio's transform runs; the audio's spectrum stays there until step 7), everything
 *   else in the inverse workspace, with no host round trip: the _async form (device pointers, a stream; lengths and warps
 *   stay host arrays) does not synchronize once the tables of the (plan, Q) exist.
 *
 * formant_match_probe (test hook): the code of the call, not a copy, stopped after stage `what`, with F =
 *   tts_hip_mel_fn_frames(fn, N): 0 logmag [2, B, F, cut] (source, then audio); 1 envelope [2, B, F, cut] (Sx, then Sy);
 *   2 gain [B, F, cut] after step 6; 3 operand Y' [B, F, 2 cut] (real parts, then imaginary parts); 4 time frames
 *   [B, F, filter_length].  Frames at and beyond F_b are 0 in every stage.  The call itself is the last stage.
 *
 * Refusals (TTS_HIP_EINVAL, first match wins, nothing copied or launched; formant_match_check in csrc/audio_call.h): a plan
 * that is not a plan of this handle; a NULL plan, audio or out, B or N < 1; a lengths[b] outside [1, N]; a row the reflect
 * cannot pad (as tts_hip_mel_fn_run); a Whisper plan; pre_emph > 0 (the inverse does not undo it); a warp that is not finite
 * or lies outside [0.5, 2]; Q outside [1, filter_length / 2 - 1]; max_gain_db not finite, not above 0 or above 60; a buffer
 * at or above 2^31 - 65536 bytes (the 2 * B * F stacked rows included) or B > 65535; a bad mem kind; a `what` outside 0 .. 4
 * (probe). */
int tts_hip_formant_match(tts_hip_engine* e, const float* audio, const float* source, int B, int N, const int32_t* lengths,
                          const tts_hip_mel_fn* fn, const double* warps, int lifter, double max_gain_db, float* out, int mem);
int tts_hip_formant_match_async(tts_hip_engine* e, const float* audio, const float* source, int B, int N, const int32_t* lengths,
                                const tts_hip_mel_fn* fn, const double* warps, int lifter, double max_gain_db, float* out,
                                void* stream);
int tts_hip_formant_match_probe(tts_hip_engine* e, const float* audio, const float* source, int B, int N, const int32_t* lengths,
                                const tts_hip_mel_fn* fn, const double* warps, int lifter, double max_gain_db, int what, float* out,
                                int mem);

/* ---- waveform clean-up (csrc/audio_proc.hip; DFT bases built on first use, no weights needed)
 * reduce_noise: utils/audio/noisereducev1.py:175-290 with the defaults utils/audio/audio_processing.py:65-83 uses.
 *   audio [B, N] -> out [B, N]; row b has lengths[b] (1 <= lengths[b] <= N) samples, lengths NULL = N for every row, and
 *   out[b, lengths[b]:] = 0.  noise NULL = each row's first min(noise_len, lengths[b]) samples (audio_processing.py:71-75),
 *   else an explicit clip [B, noise_len].  renormalize != 0: then normalize_audio(max_val=1.) over each row's own samples.
 *   `lengths` is host memory in every mode (read during the call); audio, noise and out follow `mem` / live on the device
 *   for the _async form.  All three calls share one workspace per handle: an _async call must have finished on its stream
 *   (or be ordered before the next call, e.g. same stream) before the next reduce_noise / trim_silence on the handle.
 * trim_silence: audio_processing.py:274-370 (method 'window': power 2, triangular window of window_length samples,
 *   adaptive thresholds, max_trim_factor 5); mode 0 start_end, 1 start, 2 end; start / end int32 [B] (follow `mem`) with
 *   trimmed row b = audio[b, start[b]:end[b]].  add_start, add_end >= 0 (margins in window lengths).                     */
int tts_hip_reduce_noise(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, const float* noise,
                         int noise_len, int renormalize, float* out, int mem);
int tts_hip_reduce_noise_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths,
                               const float* noise, int noise_len, int renormalize, float* out, void* stream);
int tts_hip_trim_silence(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int window_length,
                         double threshold, double add_start, double add_end, int mode, int32_t* start, int32_t* end,
                         int mem);
/* Test hooks (no effect on later calls; used by tests/): they run the code of the calls above, not a copy, on the same
 * arguments (and refuse the same ones).
 * reduce_noise_probe stops after stage `what` and copies that stage's logical extent to `out` (fp32, follows `mem`), with
 * Fr = ceil((N + 2560) / 512) frame slots per row, of which row b uses F_b = 1 + (lengths[b] + 512) / 512, and
 * Frn = ceil((noise_len + 2048) / 512) noise frame slots, of which row b uses 1 + nl_b / 512 (nl_b = noise_len, or
 * min(noise_len, lengths[b]) for the default clip).  Slots past a row's own frames hold hop-strided reads into the next
 * row's padded samples up to `gated`, where they become 0 --
 *   what 0 padded [B, Fr * 512]: 1024 zeros, the row's lengths[b] samples, zeros; 1 noise_padded [B, Frn * 512] likewise;
 *   2 spectrum [B, Fr, 2050]: real parts of bins 0 .. 1024, then the imaginary parts, before the gate; 3 noise_spectrum
 *   [B, Frn, 2050]; 4 power_max [2, B]: max |X|^2 over each row's own signal frames, then over its own noise frames;
 *   5 threshold [B, 1025] in dB; 6 mask [B, Fr, 1025] as 0 / 1 (0 in the slots past F_b); 7 gated [B, Fr, 2050]: the
 *   spectrum times 1 - smoothed mask (0 in the slots past F_b); 8 frames [B, Fr, 2048]: the windowed inverse-DFT rows before
 *   the overlap-add.  Any other `what` is TTS_HIP_EINVAL and launches nothing.  The un-normalised output is the ordinary
 *   call with renormalize = 0.
 * trim_silence_probe runs the convolution launches of trim_silence and copies conv [B, max(N, W) + 1] (fp64, follows `mem`),
 *   W = 2 * (window_length / 2): conv[b, :nc_b] = np.convolve(x_b^2, window, 'valid'), nc_b = |lengths[b] - W| + 1; what
 *   lies at and beyond nc_b is unspecified.                                                                              */
int tts_hip_reduce_noise_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths,
                               const float* noise, int noise_len, int what, float* out, int mem);
int tts_hip_trim_silence_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths,
                               int window_length, double* conv, int mem);

/* ---- silence removal (csrc/silence.hip; no weights needed): the remaining numpy trim methods of
 * utils/audio/audio_processing.py, sample for sample, with the kept samples compacted on the device.
 * audio [B, N] -> out [B, N]: row b's kept samples in order, then zeros (out[b, out_lengths[b]:] = 0); out_lengths int32
 * [B] (follows `mem` / device memory for the _async form; a row may come out empty: 0).  Row b holds lengths[b]
 * (1 <= lengths[b] <= N) samples, lengths NULL = N for every row; nothing at or beyond lengths[b] is read (it may hold NaN)
 * and a row's result equals a one-row call on audio[b, :lengths[b]].  `lengths` is host memory in every mode.
 * method TTS_HIP_SILENCE_RMS (audio_processing.py:100-200): blocks of block_size samples (the last one zero-padded), a block
 *   is silent when sqrtf(max x*x) < (float)10^(threshold / 20) (threshold in dB); a run of silent blocks [i, j) lasting
 *   >= min_silence seconds is a silence with bounds s = i * bt, e = min(L / rate, j * bt) seconds (bt = block_size / rate,
 *   doubles); neighbours closer than min_voice_time seconds merge (0: never); sample bounds are (int)(s * rate) and
 *   (int)(e * rate), the truncated double products, not i * block_size.  mode 0 start_end, 1 start, 2 end keep one slice
 *   [a, b): a leading silence is cut to its last replace_by samples, a trailing one (ending within one sample of the row's
 *   end) to its first replace_by samples; mode 3 remove also cuts every interior silence to replace_by / 2 samples at each
 *   side.  A row without any silence is returned unchanged in every mode (the reference raises IndexError in modes 0 - 2).
 *   block_size >= 1 and replace_by >= 0 are in samples.
 * method TTS_HIP_SILENCE_THRESHOLD (:385-394): m = (float)mean(x) (an fp64 sum rounded once; numpy's fp32 pairwise mean may
 *   differ from it in the last bit, so a sample within that of the threshold may be judged differently); with idx the samples where fabsf(x - m) >
 *   (float)threshold, the row keeps [first idx (mode 0, 1) or 0, last idx exclusive (mode 0, 2) or L); no such sample:
 *   unchanged.  Uses threshold and mode only.
 * method TTS_HIP_SILENCE_MEAN_WINDOW (:372-383, the reference's 'remove' method): w = (int)(min_silence * rate); conv =
 *   np.convolve(x * x, ones(w) / (w * threshold), 'same') with fp32 squares and fp64 sums; keeps the samples whose conv >
 *   min(threshold, mean(conv) / 2).  Uses threshold, min_silence and rate; mode must be 0, 1 or 2 and is ignored.
 * Parameters a method does not use are ignored.  Refused with TTS_HIP_EINVAL before anything is copied or launched (the
 * message starts with "remove_silence" / "remove_silence_async"): a method or mode out of range; mode 3 with a method other
 * than rms; rate <= 0; block_size < 1 or replace_by < 0 (rms); a non-finite or negative threshold, min_silence or
 * min_voice_time where the method uses it (the rms threshold, in dB, need only be finite); threshold <= 0, w < 1 or a row
 * shorter than w (mean-window; the reference fails with IndexError there; the message names L and w); out overlapping
 * audio; B > 65535, N > 2^24 or B * N * 4 >= 2^31.  The call shares the clean-up workspace of the handle (see reduce_noise) and is
 * enqueued whole, without a host round trip between its stages: the _async form does not synchronize.                   */
enum { TTS_HIP_SILENCE_RMS = 0, TTS_HIP_SILENCE_THRESHOLD = 1, TTS_HIP_SILENCE_MEAN_WINDOW = 2 };
int tts_hip_remove_silence(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int method, int mode,
                           int rate, double threshold, double min_silence, int block_size, int replace_by,
                           double min_voice_time, float* out, int32_t* out_lengths, int mem);
int tts_hip_remove_silence_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int method,
                                 int mode, int rate, double threshold, double min_silence, int block_size, int replace_by,
                                 double min_voice_time, float* out, int32_t* out_lengths, void* stream);
/* Test hook (no effect on later calls; used by tests/): runs the code of tts_hip_remove_silence, not a copy, on the same
 * arguments (and refuses the same ones) up to stage `what`, and copies that stage's rows to `out` (follows `mem`), `*width`
 * elements per row.  `*width` (host memory in every mode) is set by every accepted call; out NULL asks for it alone and
 * launches nothing.  With NB = ceil(N / block_size) block flags, cap silences and NT = ceil(N / 2048) tiles per row --
 *   what 0 flags uint8 [B, NB] (rms): 1 = silent block; row b holds ceil(lengths[b] / block_size) of them;
 *   1 intervals int32 [B, 2 + 2 * cap] (rms, threshold): n, cut, d0[cap], d1[cap] -- the mask keeps t < cut outside every
 *     [d0[m], d1[m]), m < n (sorted by d0; d1 <= d0: empty); entries at and beyond n are unspecified;
 *   2 mask uint8 [B, N]: 1 = kept (unspecified at and beyond lengths[b]);
 *   3 tile_offsets int32 [B, NT]: kept samples before each tile of 2048, for the row's ceil(lengths[b] / 2048) tiles;
 *   4 prefix fp64 [B, N + 1] (mean-window): P[t] = sum of the fp32 squares x[0 .. t), t <= lengths[b].
 * A `what` out of range or a stage the method does not have is TTS_HIP_EINVAL and launches nothing.                      */
int tts_hip_remove_silence_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int method, int mode,
                                 int rate, double threshold, double min_silence, int block_size, int replace_by,
                                 double min_voice_time, int what, void* out, int32_t* width, int mem);

/* ---- resampling (csrc/resample.hip; no weights needed)
 * scipy.signal.resample(x, int(n / rate * target_rate)) per row (utils/audio/audio_processing.py:30-35), window=None, in
 * fp32 (scipy returns float64).  audio [B, N] -> out [B, M]; M must be (int)((double)N / rate * target_rate) >= 1.  Row b
 * holds lengths[b] (1 <= lengths[b] <= N) samples, lengths NULL = N for every row; out row b holds
 * (int)((double)lengths[b] / rate * target_rate) samples, then zeros, and equals a one-row call on audio[b, :lengths[b]].
 * At most 2^24 samples per row in and out, B * N * 4 and B * M * 4 below 2^31.  rate == target_rate copies the rows and
 * launches nothing.  `lengths` is host memory in every mode; audio and out follow `mem` / live on the device for the _async
 * form.  One workspace per handle: an _async call must have finished on its stream (or be ordered before the next call)
 * before the next resample on the handle.                                                                               */
int tts_hip_resample(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int target_rate,
                     float* out, int M, int mem);
int tts_hip_resample_async(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate,
                           int target_rate, float* out, int M, void* stream);
/* Test hooks (no effect on later calls; used by tests/).
 * resample_probe takes the arguments of tts_hip_resample (and refuses the same ones; rate == target_rate, which runs no
 *   transform, as well), forms the same groups and runs the same launches up to the end of the forward chain, and copies what
 *   stands in the workspace there to `spectrum` [B][N / 2 + 1][2] (fp32 re, im; follows `mem`): row b holds bins
 *   0 .. lengths[b] / 2 of rfft(audio[b, :lengths[b]]), zeros beyond.
 * resample_fft_probe runs the complex fp32 FFT every chain is made of on `lines` lines of 2^logL points, `in` -> `out`
 *   [lines][2^logL][2] (HOST memory, blocking), 6 <= logL <= 25, lines * 2^logL * 8 < 2^31; anything else is TTS_HIP_EINVAL,
 *   launches nothing and leaves `out` as it was.  Up to 2^13 points a line is transformed in natural order.  Above, the
 *   forward transform (inverse = 0) of a line in natural order leaves bin k2 + L2 * k1 (L2 = 2^logL / 8192, k2 < L2,
 *   k1 < 8192) at k2 * 8192 + k1, and the inverse transform (inverse != 0; exponent +, not scaled by 1 / L) takes its
 *   input in that order and returns the natural one.                                                                     */
int tts_hip_resample_probe(tts_hip_engine* e, const float* audio, int B, int N, const int32_t* lengths, int rate, int target_rate,
                           float* spectrum, int M, int mem);
int tts_hip_resample_fft_probe(tts_hip_engine* e, const float* in, int lines, int logL, int inverse, float* out);

/* ---- measurement hooks (used by bench.py; no effect on results) -------------------------------------------------
 * Average duration in microseconds of the dominant kernel's launches (HIP events on the engine's stream) since the
 * last reset, and how many launches were timed.  kind: 0 = WaveGlow WN in-layer GEMM (layers 1..7 of a flow: K = 2176),
 * 1 = WN residual GEMM, 2 = Tacotron2 decoder step, 3 = first WN layer of a flow (start conv composed into its taps: direct
 * form one GEMM of K = 48 + 320; Winograd form the tap operand kernel and wino_layer0_kernel, K = 16 + 140 per output).
 * A tts_hip_griffin_lim call files the four parts of its iterations under the same kinds: 0 = inverse-frames GEMM, 1 = gather
 * overlap-add, 2 = forward DFT GEMM (with its gather, where the plan has one), 3 = phase update.  A tts_hip_denoise call
 * files its four parts there too: 2 = forward DFT (padding and gather included), 3 = gate, 0 = inverse-frames GEMM, 1 =
 * overlap-add.  A tts_hip_mel_dtw call files its launches as 0 = cepstra, 1 = distances, 2 = sweep, 3 = backtrack (without
 * alignment: the diagonal's reduction).  A tts_hip_time_stretch call files five parts: 2 = forward DFT, 3 = the vocoder's
 * parallel pass, 4 = its chain over the frames, 0 = inverse-frames GEMM, 1 = overlap-add.  A tts_hip_formant_match call files
 * its parts as 2 = forward DFT (one launch group per transform: two with a source), 3 = log-magnitudes and the envelope GEMM,
 * 4 = the gain kernel (kind 4 has these two uses), 0 = inverse-frames GEMM, 1 = overlap-add.
 * Timing is off unless enabled (events perturb nothing but cost a few us each).        */
int tts_hip_kernel_timing(tts_hip_engine* e, int enable);
/* Box probe: TFLOP/s a bare v_mfma_f32_32x32x2_f32 loop sustains on this device right now (every CU, 2 waves per SIMD, ~20 ms)
 * and the shader clock (GHz) it holds meanwhile -- what the fp32 MFMA roofline of THIS box is; boxes of one pool differ.    */
int tts_hip_probe_mfma_f32(tts_hip_engine* e, double* tflops, double* shader_clock_ghz);
int tts_hip_kernel_time_us(tts_hip_engine* e, int kind, double* avg_us, int64_t* launches);
int tts_hip_synchronize(tts_hip_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* TTS_HIP_H_ */
