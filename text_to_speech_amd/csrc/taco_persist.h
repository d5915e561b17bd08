// taco_persist.h -- interface of the persistent, weight-stationary Tacotron2 decoder loop (taco_persist.hip).
#pragma once
#include "taco_decode.h"

constexpr int PERSIST_NPM = 4096 + 4096 + 256 + 128;     // columns of pm_fold: att LSTM | dec LSTM | folded prenet | projection
constexpr int PERSIST_COL_ATT = 0, PERSIST_COL_DEC = 4096, PERSIST_COL_F = 8192, PERSIST_COL_P = 8448;
constexpr int PERSIST_MAX_B = 4;

// number of 8-byte entries of the exchange area for a call
size_t persist_xch_u64(int B, int Tin);
// true if this call shape can run on the persistent kernel on the engine's device (batch, LDS footprint, CU count)
bool persist_applicable(const tts_hip_engine* e, int B, int Tin);
// Runs the whole decoder loop (all steps, device-side early stop) in ONE launch on `st`; needs c.ws.pm_fold (computed by
// the caller: tacotron2.hip, run_persistent) and the zeroed part of the workspace.
// Returns TTS_HIP_OK and *steps_run; DEC_FALL_BACK if the blocks could not all become resident (nothing was modified) or
// if a hop timed out in mid-loop (outputs partial) -- the caller resets the loop state and runs the per-step graph; or a
// negative TTS_HIP_E* code.  Synchronizes `st`.
int persist_decode(tts_hip_engine* e, hipStream_t st, const DecodeCall& c, int* steps_run);
// load-time part: folded prenet-1 matrix etc. (called from tacotron2_finalize)
int persist_finalize(tts_hip_engine* e, const HostTensor* prenet0, const HostTensor* proj_k, const HostTensor* proj_b,
                     int enc, std::vector<void*>& allocs);
