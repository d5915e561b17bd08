// taco_forward.h -- the stages of the teacher-forced pass (tts_hip_tacotron2_forward) that leave the sequential loop
// (taco_forward.hip); the loop itself and the call's driver are in tacotron2.hip.
#pragma once
#include "engine.h"

// Forward-call buffers beside the per-step graph machine's (decoder_layout in tacotron2.hip puts them behind its histories)
struct ForwardBufs {
    float* hist;                        // [B * bucket(T)][1024 + enc]  cell_out = [h_dec | ctx] of every step, row b * T + t
    float* gates;                       // [B * T][4096]  p2 @ W_att[:, 0:256]^T in LstmDev's gate-interleaved row order
    float* mel_in;                      // [B * T][80]    the caller's shifted mel
    float* p1; float* p2;               // [B * T][256]   prenet layers
    float* proj;                        // [B * T][81]    projection | gate before bias, mask and sigmoid
    int* lengths;                       // [B]            mel_lengths
};

// prenet of every frame and the attention LSTM's prenet columns, on e->stream: p1 = relu(mel_in W0) (* mask 0),
// p2 = relu(p1 W1) (* mask 1), gates = p2 W_att[:, 0:256]^T.  masks: null or device [frames][2][256].
int forward_bulk_prenet(tts_hip_engine* e, const ForwardBufs& f, long long frames, const float* masks);
// proj = hist x proj_w^T over every frame, then dec_out[b][t] = t <= lengths[b] ? proj[:, 0:80] + bias : 0 and
// stop_out = sigmoid(proj[:, 80] + bias) (unmasked), on e->stream
int forward_project(tts_hip_engine* e, const ForwardBufs& f, int B, int T, float* dec_out, float* stop_out);
