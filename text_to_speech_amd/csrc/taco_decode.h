// taco_decode.h -- what the three decoder machines share on the host: the workspace plan of a decode call and the one
// description of the call that the driver (tacotron2.hip) hands to whichever machine runs it.
#pragma once
#include "engine.h"

#include <algorithm>

struct FusedState;

// Bump allocator over a device buffer; every buffer starts on a 256-byte boundary.  `take` is pure arithmetic, so a layout
// function is run twice: against a null base to learn the size (`off`), then against the allocation to get the pointers.
struct Arena {
    char* base = nullptr;
    size_t off = 0;
    template <class T>
    T* take(size_t n) {
        T* p = (T*)mark();
        off += n * sizeof(T);
        return p;
    }
    char* mark() {                       // where the next buffer will start
        off = (off + 255) / 256 * 256;
        return (char*)((uintptr_t)base + off);
    }
};

// split-path scratch of conv_gemm for a conv over `rows` rows (512 tiles x 64 rows at most take that path)
inline size_t conv_scratch_floats(long long rows) { return (size_t)5 * std::min<long long>(rows, 32768) * 512; }

struct PostnetBufs {
    uint8_t* dmask;                     // [B * T]
    float* xm;                          // [B * T][80]  masked decoder output
    float* pa;                          // [B * T][512] x 2: ping-pong of the tanh convs
    float* pb;
    float* post;                        // [B * T][80]  residual
    float* mel;                         // [B * T][80]
    float* convtmp;                     // split-path scratch of conv_gemm
    size_t convtmp_n;
};

// Workspace of one decode call.  [zero_begin, zero_end) is everything that must be zero when a machine starts the loop;
// the three histories are sized for max_len rounded up to its bucket and cleared for the real B * max_len rows.
struct DecoderWs {
    int layout_id;                      // bit 0 / 1: sized for the persistent kernel's / the fused step's exchange area
    float* masks;                       // prenet dropout masks [B][max_len][2][256] (staged or drawn here; 1 float without)
    float* pm_fold;                     // persistent: [B * Tin][PERSIST_NPM] memory folded through every consumer of the context
    char* zero_begin;
    void* state;                        // per-step graph: its DecState
    FusedState* fstate;                 // fused step: loop state (zeroed, then fused_init)
    int* freport;                       // [16] fused chunk report written at the end of every chunk: FusedState, abort code, bl_err
    unsigned long long* xch;            // exchange area of the chosen machine (persist_xch_u64 / fused_xch_u64 entries)
    int* pflags;                        // [0] abort code; persistent: [1] rendezvous counter, [2] steps run, [3..4] timed polls
    float* hatt; float* catt;           // [2][B][1024] ping-pong hidden state, [B][1024] cell state of the attention LSTM
    float* hdec; float* cdec;           //   ... and of the decoder LSTM
    float* ctx;                         // [B][enc]
    float* p2; float* q; float* frame;  // per-step graph: prenet output [B][256], query [B][128], last frame [B][80]
    float* energy;                      // per-step graph: [B][Tin]
    float* wprev; float* wcum;          // [B][Tin] previous / cumulated attention weights
    int* finished; int* lengths;        // [B]
    int* mainatt;                       // [2][B]
    char* zero_end;
    float* dec_out;                     // [B][max_len][80]
    float* stop_out;                    // [B][max_len]
    float* attn_hist;                   // [B][max_len][Tin]
    PostnetBufs post;
};

// Everything a machine needs for one call; all pointers are device memory that stays valid (and in place) until the call
// returns and while the chunk graphs of the call's shape bucket are replayed.
struct DecodeCall {
    int B, Tin, max_len, early_stop, win_len, win_off;
    bool half_w;                        // LSTM matrices in fp16
    const void* enc_buf;                // the encoded batch's allocation (graph identity)
    const float* memory;                // [B * Tin][enc]   encoder outputs, zero at padded tokens
    const float* pm;                    // [B * Tin][128]   processed memory
    const uint8_t* mask;                // [B * Tin]
    const int* enc_len;                 // [B]
    const int* bl_err;                  // encoder status word
    const float* masks;                 // ws.masks, or null for a call without prenet masks
    const DecoderWs& ws;
    long long* trace = nullptr;         // fused step, debug builds only: [128 steps][2 kernels][4 blocks][16 slots] timestamps
};

// a machine's "not this time": the caller resets the loop state and runs the per-step graph (errors are negative)
constexpr int DEC_FALL_BACK = 1;
