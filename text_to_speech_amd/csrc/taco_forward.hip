// taco_forward.hip -- Tacotron2 teacher-forced forward pass on gfx950: what leaves the sequential loop.
//
// Replaces /root/reference/architectures/tacotron2_arch.py:806-849 (Tacotron2.call) with :526-607 (Tacotron2Decoder.call):
// step t of the decoder reads frame t of a GIVEN mel, not its own previous output.  Pinned semantics:
//   * mel_input [B, T, 80] is already shifted -- frame 0 is the zero go-frame, frame t is target frame t - 1 -- as the
//     reference's wrapper builds it (models/tts/tacotron2.py:243-259: mel = pad(mel, [(1, 0), (0, 0)]), input mel[:-1]);
//   * every row runs all T steps: no stop test, no attention window (call has neither); frames at and past a row's length
//     are consumed as given;
//   * step t = prenet(mel_input[:, t]) (* the dropout mask of (b, t), :188-203) -> attention LSTM on [prenet | context] ->
//     location-sensitive attention over the whole unpadded memory -> decoder LSTM on [h_att | context] ->
//     cell_out = [h_dec | context]: the cell of :422-486, the one infer runs, from the same initial state;
//   * decoder_output = where(t <= mel_lengths[b], cell_out @ linear_projection + bias, 0) (:555, :577, :587 -- note the <=);
//   * stop_tokens = sigmoid(cell_out @ gate + bias), unmasked (:584);
//   * mel = decoder_output + postnet(decoder_output, mask) with that mask (:846-847);
//   * attention [B, T, Tin]: the alignments of every step (call drops them; returned here as infer returns them).
//
// With every input known up front only the two LSTMs and the attention are sequential (tacotron2.hip: five kernels per step
// in chunk graphs, no host read-back between chunks).  This file holds the rest, each one GEMM over the B * T frames on
// gemm_f32.h and at most one small pass behind it:
//   prenet       [B*T][80] -> relu -> [B*T][256] -> relu -> [B*T][256], the multiplicative masks in a pass behind each
//   gate term    G = p2 @ W_att[:, 0:256]^T, [B*T][4096] in LstmDev's gate-interleaved row order (always the fp32 matrix):
//                the step's attention LSTM then streams only the enc + 1024 remaining columns and adds G[b, t]
//   projection   [B*T][1024 + enc] x proj_w^T -> 80 frame columns | gate, then the bias, the <= mask and the sigmoid
#include "taco_forward.h"

#include "gemm_f32.h"

using namespace ttsgemm;

namespace {

constexpr int PRE = 256, NMEL = 80, DRNN = 1024, GATES = 4096;

// p[row][c] *= masks[row][layer][c]   (masks [frames][2][256])
__global__ void prenet_mask_kernel(float* __restrict__ p, const float* __restrict__ masks, int layer, long long n4) {
    const long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i4 >= n4) return;
    const long long row = i4 / (PRE / 4);
    const int c = (int)(i4 % (PRE / 4)) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(p + i4 * 4);
    v *= *reinterpret_cast<const f32x4*>(masks + (row * 2 + layer) * PRE + c);
    *reinterpret_cast<f32x4*>(p + i4 * 4) = v;
}

// proj [frames][81] (+ bias) -> dec_out [frames][80] masked with t <= lengths[b], stop_out [frames] = sigmoid(gate).
// The bias is added here, behind the sum: the GEMM would start its k-ordered chain from it, and the gate's bias is an order
// of magnitude above its 1.5 k products, so every one of them would be rounded at the bias's ulp (measured: stop tokens 6e-7
// off, five times the frames' error class; the frames' biases are small and did not show it).
__global__ void forward_finish_kernel(const float* __restrict__ proj, const float* __restrict__ bias,
                                      const int* __restrict__ lengths, float* __restrict__ dec_out,
                                      float* __restrict__ stop_out, int T, long long frames) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= frames * (NMEL + 1)) return;
    const long long row = idx / (NMEL + 1);
    const int o = (int)(idx % (NMEL + 1));
    const int b = (int)(row / T), t = (int)(row % T);
    const float v = proj[idx] + bias[o];
    if (o < NMEL) dec_out[row * NMEL + o] = t <= lengths[b] ? v : 0.f;
    else stop_out[row] = sigmoid_exact(v);
}

}  // namespace

int forward_bulk_prenet(tts_hip_engine* e, const ForwardBufs& f, long long frames, const float* masks) {
    const Tacotron2Dev& tc = e->taco;
    hipStream_t st = e->stream;
    const int M = (int)frames;
    const long long n4 = frames * (PRE / 4);
    const unsigned mask_blocks = (unsigned)((n4 + 255) / 256);
    {   // layer 0: K = 80 of a 96-wide zero-padded weight row
        GemmArgs g = gemm_linear(f.mel_in, NMEL, NMEL, tc.prenet_w0_Bt, 96, PRE, M, f.p1);
        g.seg[0].kpad = 96;
        g.act = ACT_RELU;
        HIPCHK(e, gemm_small(g, 1, st));
    }
    if (masks) {
        hipLaunchKernelGGL(prenet_mask_kernel, dim3(mask_blocks), dim3(256), 0, st, f.p1, masks, 0, n4);
        HIPCHK(e, hipGetLastError());
    }
    {
        GemmArgs g = gemm_linear(f.p1, PRE, PRE, tc.prenet_w1, PRE, PRE, M, f.p2);
        g.act = ACT_RELU;
        HIPCHK(e, gemm_small(g, 1, st));
    }
    if (masks) {
        hipLaunchKernelGGL(prenet_mask_kernel, dim3(mask_blocks), dim3(256), 0, st, f.p2, masks, 1, n4);
        HIPCHK(e, hipGetLastError());
    }
    {   // the prenet columns are the first 256 of every packed attention-LSTM row
        const GemmArgs g = gemm_linear(f.p2, PRE, PRE, tc.att.W, tc.att.kin + tc.att.units, GATES, M, f.gates);
        HIPCHK(e, gemm_small(g, 1, st));
    }
    return TTS_HIP_OK;
}

int forward_project(tts_hip_engine* e, const ForwardBufs& f, int B, int T, float* dec_out, float* stop_out) {
    const Tacotron2Dev& tc = e->taco;
    hipStream_t st = e->stream;
    const long long frames = (long long)B * T;
    const int K = DRNN + tc.enc_dim;
    const GemmArgs g = gemm_linear(f.hist, K, K, tc.proj_w, K, NMEL + 1, (int)frames, f.proj);
    HIPCHK(e, gemm_small(g, 1, st));
    const long long n = frames * (NMEL + 1);
    hipLaunchKernelGGL(forward_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f.proj, tc.proj_b, f.lengths,
                       dec_out, stop_out, T, frames);
    HIPCHK(e, hipGetLastError());
    return TTS_HIP_OK;
}
