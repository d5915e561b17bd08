// taco_fused.h -- interface of the fused two-kernel Tacotron2 decoder step (taco_fused.hip): batches of 3 .. 8 rows.
#pragma once
#include "taco_decode.h"

constexpr int FUSED_CHUNK = 64;          // decoder steps per enqueued chunk (= per hipGraph replay); even
constexpr int FUSED_MAX_B = 8;

// Device-resident loop state of one call (32 bytes, one scalar load per kernel).  Zero-initialised = before step 0.
struct FusedState {
    int t0;                              // first step of the current chunk
    int n_fin;                           // rows whose stop token has fired (counted after the last computed stop token)
    int steps_run;                       // decoder steps fully executed
    int exec_t;                          // t + 1 of the step whose first half (kernel X) decided to run
    int B, max_len, early_stop;
    int pad;
};

size_t fused_xch_u64(int B, int Tin, int enc);
// true if this call shape can run on the fused kernels on the engine's device
bool fused_applicable(const tts_hip_engine* e, int B, int Tin);
// sets the loop state for a new call (enqueued on st; c.ws.fstate must be zero)
int fused_init(tts_hip_engine* e, hipStream_t st, const DecodeCall& c);
// enqueues FUSED_CHUNK decoder steps (2 kernels each), the chunk's tail projection and the chunk advance on st
// (capturable: no synchronisation, no host reads)
int fused_enqueue_chunk(tts_hip_engine* e, hipStream_t st, const DecodeCall& c);
