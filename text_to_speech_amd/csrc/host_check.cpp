// host_check.cpp -- CPU-only build of the host code that reads untrusted input (ttsw_host.h, the call checks), for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all host_check.cpp -o ttsw_check_asan
// (csrc/build_host_asan.sh; GPU AddressSanitizer is not available on the pool, and this code needs no GPU).
// usage: ttsw_check_asan [--load] file...   -- one line per file: "<status> <tensors> <floats> <message>"; --load also reads
// every payload (what tts_hip_load_weights does), without it only the container is validated (tts_hip_check_weights_file).
//        ttsw_check_asan --wg-plan LO HI [STEP]  -- the WaveGlow dispatch (wg_plan.h), one line "BT precision form PR tiles
// wino_wanted" for every STEP-th (default: every) frame count LO..HI, the three precisions and forms 0..3
// (tests/test_wg_plan.py compares them with pick_variant).
//        ttsw_check_asan --wn-taps H T LEN...  -- the tap operand of a flow's first WN layer in the Winograd form (wn_tap_row,
// wn_tap_of_col, wn_tap_src_col of wg_plan.h, the functions wino_tap_operand_kernel runs) for a call of B = number of LEN rows
// of T frames, H coupling channels: a model a0p -- column c < H of row m holds 1 + 8 m + c, column H holds 1, rows of frames
// t >= LEN[b] are zero as after the tail clearing -- goes in, one line of 16 integers per phase-major row comes out, behind a
// first line "PR" (tests/test_wino_layer0_map.py restates it by positions).
//        ttsw_check_asan --wg-call T PACKED CHUNKB [KEY=VALUE...] [LEN...]  -- the front end of a WaveGlow call (wg_call.h)
// for a batch of B = number of LEN rows (no LEN: lengths NULL, B from B=) run as an entry point named "who".  CHUNKB 0:
// rows per run as the engine derives them.  Settings: B= precision= mem= async=1 noise=0|1|2 (WgNoise) and
// null=mel,audio,keys,offsets to pass that pointer as NULL.  First line "<status> <message>" of wg_call_check; when the call
// is accepted: "F n_gap", then the lines "info ...", "run_tails ..." and "counts ..." of wg_call_table
// (tests/test_wg_call.py compares them with packing_plan and a numpy restatement).  flow= what= or layer= (default 0): the
// inverse direction's test hook instead (wg_probe_check; null=out for its output, c.audio is not looked at); the same lines.
//        ttsw_check_asan --wg-encode T [KEY=VALUE...] [LEN...]  -- the front end of a forward-flow call (wg_encode_check of
// wg_call.h) for a batch of B = number of LEN rows (no LEN: lengths NULL, B from B=) run as an entry point named "who".
// Settings: B= mem= async=1 and null=audio,mel,z,stats.  One line "<status> <message>" (tests/test_waveglow_encode.py compares
// it with a Python restatement of the refusal order).  flow= or what= (default 0): the test hook's front end instead
// (wg_encode_probe_check; null=out for its output; tests/test_waveglow_encode_flows.py).
//        ttsw_check_asan --audio-call KIND [KEY=VALUE...] [LEN...]  -- the front end of an audio call (audio_call.h), KIND one
// of reduce_noise, trim, resample, silence, for a batch of B = number of LEN rows of N samples (no LEN: lengths NULL, B from
// B=) run as an entry point named "who".  Settings: B= N= mem= (default 1, device), null=audio,out,lens (out: every output
// pointer; lens: out_lengths), overlap=1 (out one float behind audio) and the call's own arguments under their C names
// (noise_len; window_length threshold add_start add_end mode; rate target_rate M; method mode rate threshold min_silence
// block_size replace_by min_voice_time).  First line "<status> <message>"; when the call is accepted the geometry the check
// derived: reduce_noise "Fr NP Frn NQ total", trim "W Wp Cst", silence "NT NB cap w total", resample one line
// "logf logi M_b" per row (tests/test_audio_call.py compares them with a Python restatement).  KIND silence with probe=1
// what=STAGE: the check of tts_hip_remove_silence_probe (null=out asks for the width alone, null=lens takes its width
// away); accepted: a further line "width elem" (tests/test_silence_stages.py).  KIND resample_fft: the check
// of tts_hip_resample_fft_probe (settings lines logL, null=audio,out); accepted: the bytes of the staged lines.  KIND
// mel_fn: the plan check and the call check of a mel plan (mel_cfg_check, then mel_call_check); settings mel_kind (the config's kind) sampling_rate n_mel_channels
// filter_length hop_length win_length normalize_mode mel_fmin mel_fmax pre_emph, window=I:VALUE (an explicit window of ones
// with window[I] = VALUE; else NULL) and null=cfg,fn,audio,out (fn: the call gets no plan).  First line as above, from
// whichever check refuses first; accepted: "K4 Kpad NB MAGK gathered", "Fr Fout PW NP total" and "F_b ..." (the result's
// frames per row), then "mel_fn_frames(N)" (tests/test_mel_fn_call.py).
// stft_inv: the check of tts_hip_stft_inverse (input_kind=-1) / tts_hip_griffin_lim[_probe] (stft_inv_check) on a plan of the
// mel_fn settings; settings F C input_kind n_iters momentum what k, the positional values are frames[b]; prints the status
// line, then "PW NP EK Sout total", the eleven workspace offsets, the rows' sample counts, and with minv=1 whether the
// filterbank's Cholesky inverse exists and its n_mel * cut values (tests/test_stft_inv.py).
// denoise: the check of tts_hip_denoise[_probe] (denoise_check) on a plan of the mel_fn settings; settings N strength what and
// null=audio,out,fn,bias, the positional values are lengths[b]; prints the status line, then "Fr PW NP off_padded off_spectrum
// total" of the transform's workspace, "F off_operand off_tframes total" of the inverse's, the rows' frames and the samples
// each row of the result holds (tests/test_denoise.py).
//        ttsw_check_asan --taco-call KIND [KEY=VALUE...] [LEN...]  -- the front end of a Tacotron2 call (taco_call.h) run as an
// entry point named "who", KIND one of encode, decode, forward, infer (= the encode check, then the decode check on the batch the
// encoder would fill, as tts_hip_tacotron2_infer* does).  Refused, first match wins -- encode: mem kind, weights not finalized,
// tokens / B / Tin, speaker; decode and forward: precision, mem kind, weights not finalized, encoded batch, its width, pointers
// (keys / offsets | mel_input / mel_lengths), max_len | T, and for forward B * T and mel_lengths[b].  Settings: B= Tin= mem=
// ready=0|1 and null=...; encode: spk_dim=, null=tokens,speaker; decode: max_len= enc= model_enc= precision= masks=0..3
// (TacoMasks), null=encoded,keys,offsets; forward: T= enc= model_enc= precision=, null=encoded,mel,lens, and the LEN are
// mel_lengths (no LEN: B from B=, every length T).  First line "<status> <message>"; when a forward call is accepted "frames
// mel_in prenet gates history proj" of taco_forward_sizes (tests/test_taco_call.py compares them with a Python restatement).
//        ttsw_check_asan --taco-loss [KEY=VALUE...] [KIND...]  -- the front end of a TacotronLoss call (taco_loss_call.h) run as an
// entry point named "who" with the kind codes KIND (TTS_HIP_LOSS_*; n_kinds = their number unless n_kinds= says otherwise: the
// array always holds at least 4 entries).  Settings: B= T= mem= n_kinds= mask= logits= fw= nfw= (the two weights; nan and inf are
// understood), null=target,gate,dec,mel,stop,kinds,out and odd=target,dec,mel (that pointer 4 bytes past a 16-byte boundary).
// First line "<status> <message>"; when the call is accepted "K chunks weighted bytes" of taco_loss_layout
// (tests/test_taco_loss.py compares them with a Python restatement).
//        ttsw_check_asan --mel-dtw [KEY=VALUE...]  -- the front end of an MCD / DTW call (mel_dtw_call.h) run as an entry point named
// "who".  Settings: B= Ta= Tb= n_mel= n_cep= flags= mem= probe=1 what= (the probe's check) path=0|1 (the call asks for the
// path), la=N,N,... lb=N,N,... (the length tables; absent: NULL), null=a,b,stats,out and dct=1.  First line "<status>
// <message>"; when the call is accepted "R W K skew_i aligned" and the thirteen offsets, out_elems and bytes of mel_dtw_layout,
// and with dct=1 the R * n_mel values of mel_dtw_dct, one per line (tests/test_mel_dtw.py compares them with a Python
// restatement).
//        ttsw_check_asan --pitch [KEY=VALUE...]  -- the front end of a pitch call or of an F0 comparison (pitch_call.h) run as an
// entry point named "who".  Settings of a pitch call: B= N= rate= hop= win= tau_min= tau_max= threshold= (nan and inf are
// understood) mem= probe=1 what= len=N,N,... (the length table; absent: NULL), null=audio,out.  With f0=1 an F0 comparison: B=
// Fa= Fb= P= path=0|1 gross= mem= la=N,N,... lb=N,N,... null=f0_a,f0_b,stats.  First line "<status> <message>"; when the call is
// accepted "F threads lens in out out_elems bytes" of pitch_layout, or "lens in_a in_b path stats bytes" of f0_error_layout
// (tests/test_pitch.py compares them with a Python restatement).
//        ttsw_check_asan --pyin [KEY=VALUE...]  -- the front end of a probabilistic-YIN call (pyin_check, pyin_layout and pyin_tables
// of pitch_call.h) run as an entry point named "who".  Settings: those of a pitch call but threshold=, and n_bins= bps= max_step=
// n_thresh= prior=P,P,... (absent: 1 / n_thresh each; nan and inf are understood) switch= no_trough= fmin= probe=1 what=
// null=audio,out,prior and tables=1.  First line "<status> <message>"; when the call is accepted "F threads vit_threads" and the
// ten offsets, out_elems and bytes of pyin_layout, and with tables=1 the cumulative prior and the transition tables, one value
// a line (tests/test_pyin.py compares them with a Python restatement).
//        ttsw_check_asan --time-stretch [KEY=VALUE...] [LEN...]  -- the front end of a time-stretch call (time_stretch_check of
// audio_call.h) for a batch of B = number of LEN rows of N samples (no LEN: lengths NULL, B from B=) run as an entry point named
// "who", on a Tacotron-kind plan of filter_length= hop_length= win_length= pre_emph= (mel_kind=1: a Whisper plan).  Settings:
// B= N= M= mem= what= rates=R,R,... (one value: every row's) and null=fn,audio,out,rates.  First line "<status> <message>"; when
// the call is accepted "Fr T M", the five offsets of the vocoder's buffers and the inverse workspace's extent, then F_b, T_b,
// S_b and the kept samples per row.  helpers=1: no check; "frames samples" of ts_row_frames / ts_row_samples per LEN
// (tests/test_time_stretch.py compares all of it with a Python restatement).
//        ttsw_check_asan --formant-match [KEY=VALUE...] [LEN...]  -- the front end of a formant-match call (formant_match_check of
// audio_call.h) for a batch of B = number of LEN rows of N samples (no LEN: lengths NULL, B from B=) run as an entry point named
// "who", on a plan as --time-stretch takes it.  Settings: B= N= Q= max_gain_db= mem= what= warps=W,W,... (one value: every
// row's; absent: warps NULL) and null=fn,audio,out.  First line "<status> <message>"; when the call is accepted "Fr Q" and the
// bits of the fp32 clamp G, the four offsets of the call's own buffers and the inverse workspace's extent, then F_b and the kept
// samples per row.  table=1: no check; the liftering table fm_lifter_table(filter_length, Q), one value a line
// (tests/test_formant.py compares all of it with a Python restatement).
// Exit status 0 unless a sanitizer aborts the process.
#include <cstdlib>
#include <vector>

#include "audio_call.h"
#include "mel_dtw_call.h"
#include "pitch_call.h"
#include "taco_call.h"
#include "taco_loss_call.h"
#include "ttsw_host.h"
#include "wg_call.h"
#include "wg_plan.h"

static int print_wg_plans(int lo, int hi, int step) {
    for (int bt = lo; bt <= hi; bt += step)
        for (int precision = 0; precision < 3; ++precision)
            for (int form = 0; form < 4; ++form) {
                const WgPlan p = wg_plan(bt, precision, form);
                if (p.BT != bt || p.M != 32ll * p.PR || p.NP != (precision == 2 ? 2 : 1)) return 2;
                printf("%d %d %d %d %d %d\n", bt, precision, form, p.PR, (int)p.tiles, (int)p.wino_wanted);
            }
    return 0;
}

static int print_wn_taps(int h, int T, const std::vector<int>& lens) {
    const int B = (int)lens.size(), BT = B * T;
    if (h < 1 || h > 4 || T < 1 || B < 1) return 2;
    const int PR = wg_plan(BT, 0, 1).PR;
    std::vector<long long> a0p((size_t)32 * PR * 16, 0);
    for (int m = 0; m < 32 * PR; ++m) {
        const int f = m % PR;
        if (f < BT && f % T >= lens[f / T]) continue;                          // a cleared tail row
        for (int c = 0; c < h; ++c) a0p[(size_t)m * 16 + c] = 1 + 8ll * m + c;
        a0p[(size_t)m * 16 + h] = 1;
    }
    printf("%d\n", PR);
    for (int m = 0; m < 32 * PR; ++m)
        for (int k = 0; k < 16; ++k) {
            const int tap = wn_tap_of_col(k, h);
            const long long src = tap < 3 ? wn_tap_row(m / PR, m % PR, tap - 1, PR, BT, T) : -1;
            if (src >= 32ll * PR) return 2;
            printf("%lld%c", src >= 0 ? a0p[(size_t)src * 16 + wn_tap_src_col(k, h)] : 0ll, k == 15 ? '\n' : ' ');
        }
    return 0;
}

static int print_wg_call(int argc, char** argv) {
    static float mel, audio, out;                                              // never read: the front end only tests pointers
    static uint64_t keys, offsets;
    WgProbe probe{0, 0, 0, &out};
    bool probing = false;
    WgCall c{};
    c.who = "who", c.mel = &mel, c.audio = &audio, c.keys = &keys, c.offsets = &offsets;
    c.T = atoi(argv[2]), c.packed = atoi(argv[3]) != 0, c.sigma = 1.f;
    int chunkB = atoi(argv[4]), B = -1;
    std::vector<int32_t> lens;
    for (int i = 5; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            lens.push_back((int32_t)atoi(argv[i]));
            continue;
        }
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        const int v = atoi(eq + 1);
        if (key == "B") B = v;
        else if (key == "precision") c.precision = v;
        else if (key == "mem") c.mem = v;
        else if (key == "async") c.async = v != 0;
        else if (key == "noise") c.noise = (WgNoise)v;
        else if (key == "flow") probe.flow = v, probing = true;
        else if (key == "what") probe.what = v, probing = true;
        else if (key == "layer") probe.layer = v, probing = true;
        else if (key == "null") {
            if (strstr(eq, "out")) probe.out = nullptr;
            if (strstr(eq, "mel")) c.mel = nullptr;
            if (strstr(eq, "audio")) c.audio = nullptr;
            if (strstr(eq, "keys")) c.keys = nullptr;
            if (strstr(eq, "offsets")) c.offsets = nullptr;
        } else return 2;
    }
    c.lengths = lens.empty() ? nullptr : lens.data();
    c.B = lens.empty() ? B : (int)lens.size();
    char why[512] = "";
    const int rc = probing ? wg_probe_check(c, probe, why, sizeof why) : wg_call_check(c, why, sizeof why);
    printf("%d %s\n", rc, why);
    if (rc) return 0;
    if (chunkB <= 0) chunkB = c.packed ? c.B : kMaxFramesPerRun / c.T;
    WgTable t;
    wg_call_table(c.B, c.T, c.lengths, c.packed, chunkB, &t);
    printf("%d %d\ninfo", t.F, t.n_gap);
    for (int v : t.info) printf(" %d", v);
    printf("\nrun_tails");
    for (int v : t.run_tails) printf(" %d", v);
    printf("\ncounts");
    for (long long v : t.counts) printf(" %lld", v);
    printf("\n");
    return 0;
}

static int print_wg_encode(int argc, char** argv) {
    static float audio, mel, z, stats, out;                                    // never read: the front end only tests pointers
    WgEncode c{"who", &audio, &mel, -1, atoi(argv[2]), nullptr, &z, &stats, false, 0, nullptr};
    WgEncodeProbe probe{0, 0, &out};
    bool probing = false;
    std::vector<int32_t> lens;
    for (int i = 3; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            lens.push_back((int32_t)atoi(argv[i]));
            continue;
        }
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        const int v = atoi(eq + 1);
        if (key == "B") c.B = v;
        else if (key == "mem") c.mem = v;
        else if (key == "async") c.async = v != 0;
        else if (key == "flow") probe.flow = v, probing = true;
        else if (key == "what") probe.what = v, probing = true;
        else if (key == "null") {
            if (strstr(eq, "out")) probe.out = nullptr;
            if (strstr(eq, "audio")) c.audio = nullptr;
            if (strstr(eq, "mel")) c.mel = nullptr;
            if (strstr(eq, "z")) c.z = nullptr;
            if (strstr(eq, "stats")) c.stats = nullptr;
        } else return 2;
    }
    if (!lens.empty()) c.lengths = lens.data(), c.B = (int)lens.size();
    char why[512] = "";
    const int rc = probing ? wg_encode_probe_check(c, probe, why, sizeof why) : wg_encode_check(c, why, sizeof why);
    printf("%d %s\n", rc, why);
    return 0;
}

static int print_audio_call(int argc, char** argv) {
    // never read: the checks only test and compare the pointers, so two addresses 4 GiB apart stand for the buffers
    const float* audio = (const float*)(uintptr_t)0x100000000ull;
    float* out = (float*)(uintptr_t)0x200000000ull;
    static int32_t out_lengths;
    const int32_t* lens_out = &out_lengths;
    const std::string kind = argv[2];
    std::map<std::string, double> v{{"B", -1}, {"N", 0}, {"mem", TTS_HIP_MEM_DEVICE}, {"noise_len", 1}, {"window_length", 2},
                                    {"threshold", 0.1}, {"add_start", 0}, {"add_end", 0}, {"mode", 0}, {"rate", 1},
                                    {"target_rate", 1}, {"M", 0}, {"method", 0}, {"min_silence", 0.1}, {"block_size", 1},
                                    {"replace_by", 0}, {"min_voice_time", 0}, {"overlap", 0}, {"mel_kind", 0},
                                    {"sampling_rate", 22050}, {"n_mel_channels", 80}, {"filter_length", 1024},
                                    {"hop_length", 256}, {"win_length", 1024}, {"normalize_mode", 0}, {"mel_fmin", 0},
                                    {"mel_fmax", 8000}, {"pre_emph", 0}, {"lines", 1}, {"logL", 6}, {"F", 0}, {"C", 0},
                                    {"input_kind", 0}, {"n_iters", 0}, {"momentum", 0}, {"what", -1}, {"k", 0}, {"minv", 0},
                                    {"strength", 0.1}, {"probe", 0}};
    bool null_cfg = false, null_fn = false, null_bias = false;
    int window_at = -1;
    double window_value = 1;
    std::vector<int32_t> lengths;
    for (int i = 3; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            lengths.push_back((int32_t)atoi(argv[i]));
            continue;
        }
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "null") {
            if (strstr(eq, "audio")) audio = nullptr;
            if (strstr(eq, "out")) out = nullptr;
            if (strstr(eq, "lens")) lens_out = nullptr;
            if (strstr(eq, "cfg")) null_cfg = true;
            if (strstr(eq, "fn")) null_fn = true;
            if (strstr(eq, "bias")) null_bias = true;
        } else if (key == "window") {
            const char* colon = strchr(eq, ':');
            if (!colon) return 2;
            window_at = atoi(eq + 1), window_value = atof(colon + 1);
        } else if (v.count(key)) {
            v[key] = atof(eq + 1);
        } else {
            return 2;
        }
    }
    if (v["overlap"] != 0 && audio) out = const_cast<float*>(audio) + 1;
    const int32_t* lp = lengths.empty() ? nullptr : lengths.data();
    const int B = lengths.empty() ? (int)v["B"] : (int)lengths.size(), N = (int)v["N"], mem = (int)v["mem"];
    char why[256] = "";
    std::vector<int> lens, mlens;
    if (kind == "reduce_noise") {
        const int rc = rn_check("who", audio, B, N, lp, (int)v["noise_len"], out, mem, lens, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        const RnGeom g = rn_geom(B, N, (int)v["noise_len"]);
        printf("%d %d %d %d %zu\n", g.Fr, g.NP, g.Frn, g.NQ, g.total);
    } else if (kind == "trim") {
        TrimGeom g{};
        const int rc = trim_check("who", audio, out != nullptr, B, N, lp, (int)v["window_length"], v["threshold"], v["add_start"],
                                  v["add_end"], (int)v["mode"], mem, lens, &g, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        printf("%d %d %d\n", g.W, g.Wp, g.Cst);
    } else if (kind == "resample") {
        const int rc = rs_check("who", audio, B, N, lp, (int)v["rate"], (int)v["target_rate"], out, (int)v["M"], mem, lens, mlens,
                                why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        if ((int)lens.size() != B || (int)mlens.size() != B) return 2;
        for (int b = 0; b < B; ++b) {
            const RsLens l = rs_lens(lens[b], mlens[b]);
            printf("%d %d %d\n", l.logf, l.logi, mlens[b]);
        }
    } else if (kind == "resample_fft") {
        const int rc = rs_fft_probe_check("who", audio, (int)v["lines"], (int)v["logL"], out, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        printf("%lld\n", ((long long)v["lines"] << (int)v["logL"]) * 8);
    } else if (kind == "silence") {
        SilCall c;
        SilStage s{};
        const bool probing = v["probe"] != 0;           // lens_out stands for the probe's width
        const int rc = probing ? sil_probe_check("who", audio, B, N, lp, (int)v["method"], (int)v["mode"], (int)v["rate"],
                                                 v["threshold"], v["min_silence"], (int)v["block_size"], (int)v["replace_by"],
                                                 v["min_voice_time"], (int)v["what"], out, lens_out, mem, c, &s, why, sizeof why)
                               : sil_check("who", audio, B, N, lp, (int)v["method"], (int)v["mode"], (int)v["rate"], v["threshold"],
                                           v["min_silence"], (int)v["block_size"], (int)v["replace_by"], v["min_voice_time"], out,
                                           lens_out, mem, c, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        if ((int)c.lens.size() != B) return 2;
        printf("%d %d %d %d %zu\n", c.NT, c.NB, c.cap, c.w, c.total);
        if (probing) printf("%d %d\n", s.width, s.elem);
    } else if (kind == "mel_fn") {
        const tts_hip_mel_config cfg{(int)v["mel_kind"], (int)v["sampling_rate"], (int)v["n_mel_channels"], (int)v["filter_length"],
                                     (int)v["hop_length"], (int)v["win_length"], (int)v["normalize_mode"], v["mel_fmin"],
                                     v["mel_fmax"], v["pre_emph"]};
        std::vector<double> window;
        if (window_at >= 0 && cfg.win_length > 0 && cfg.win_length <= 4096) {
            window.assign((size_t)cfg.win_length, 1.0);
            if (window_at < cfg.win_length) window[(size_t)window_at] = window_value;
        }
        MelPlan p{};
        int rc = mel_cfg_check("who", null_cfg ? nullptr : &cfg, window.empty() ? nullptr : window.data(), true, &p, why, sizeof why);
        MelGeom g;
        if (!rc) rc = mel_call_check("who", null_fn ? nullptr : &p, audio, B, N, lp, out, mem, &g, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        if ((int)g.lens.size() != B || (int)g.fout.size() != B) return 2;
        printf("%d %d %d %d %d\n%d %d %d %d %zu\n", p.K4, p.Kpad, p.NB, p.MAGK, (int)p.gather, g.Fr, g.Fout, g.PW, g.NP, g.total);
        for (int b = 0; b < B; ++b) printf("%d%c", g.fout[b], b == B - 1 ? '\n' : ' ');
        printf("%d\n", mel_out_frames(p, N));
    } else if (kind == "stft_inv") {
        // the positional values are frames[b]; N is unused
        const tts_hip_mel_config cfg{(int)v["mel_kind"], (int)v["sampling_rate"], (int)v["n_mel_channels"], (int)v["filter_length"],
                                     (int)v["hop_length"], (int)v["win_length"], (int)v["normalize_mode"], v["mel_fmin"],
                                     v["mel_fmax"], v["pre_emph"]};
        MelPlan p{};
        int rc = mel_cfg_check("who", &cfg, nullptr, true, &p, why, sizeof why);
        GlGeom g;
        const int F = (int)v["F"], ik = (int)v["input_kind"];
        if (!rc)
            rc = stft_inv_check("who", null_fn ? nullptr : &p, audio, audio, out, B, F, (int)v["C"], lp, ik, (int)v["n_iters"],
                                v["momentum"], mem, (int)v["what"], (int)v["k"], &g, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        if ((int)g.frames.size() != B) return 2;
        printf("%d %d %d %lld %zu\n", g.PW, g.NP, g.EK, g.Sout, g.total);
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", g.off_info, g.off_target, g.off_operand, g.off_tprev, g.off_phasor,
               g.off_tframes, g.off_padded, g.off_gathered, g.off_spectrum, g.off_expmel, g.off_minv);
        for (int b = 0; b < B; ++b) printf("%lld%c", stft_samples(p, g.frames[b]), b == B - 1 ? '\n' : ' ');
        if (v["minv"] != 0) {
            std::vector<double> Minv;
            const bool ok = mel_min_norm_inverse(p, Minv);
            printf("%d\n", (int)ok);
            if (ok)
                for (size_t i = 0; i < Minv.size(); ++i) printf("%.17g\n", Minv[i]);
        }
    } else if (kind == "denoise") {
        const tts_hip_mel_config cfg{(int)v["mel_kind"], (int)v["sampling_rate"], (int)v["n_mel_channels"], (int)v["filter_length"],
                                     (int)v["hop_length"], (int)v["win_length"], (int)v["normalize_mode"], v["mel_fmin"],
                                     v["mel_fmax"], v["pre_emph"]};
        MelPlan p{};
        int rc = mel_cfg_check("who", &cfg, nullptr, true, &p, why, sizeof why);
        DnGeom g;
        if (!rc)
            rc = denoise_check("who", null_fn ? nullptr : &p, audio, B, N, lp, null_bias ? nullptr : audio, v["strength"], out, mem,
                               (int)v["what"], &g, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        if ((int)g.fwd.lens.size() != B || (int)g.fwd.fout.size() != B || (int)g.inv.frames.size() != B || (int)g.keep.size() != B)
            return 2;
        printf("%d %d %d %zu %zu %zu\n", g.fwd.Fr, g.fwd.PW, g.fwd.NP, g.fwd.off_padded, g.fwd.off_spectrum, g.fwd.total);
        printf("%d %zu %zu %zu\n", g.inv.F, g.inv.off_operand, g.inv.off_tframes, g.inv.total);
        for (int b = 0; b < B; ++b) printf("%d%c", g.inv.frames[b], b == B - 1 ? '\n' : ' ');
        for (int b = 0; b < B; ++b) printf("%d%c", g.keep[b], b == B - 1 ? '\n' : ' ');
    } else {
        return 2;
    }
    return 0;
}

static int print_taco_call(int argc, char** argv) {
    static float mel;                                                          // never read: the front end only tests the pointers
    static int32_t tokens;
    static uint64_t keys, offsets;
    const std::string kind = argv[2];
    std::map<std::string, int> v{{"B", -1}, {"len", 1}, {"Tin", 8}, {"enc", 512}, {"model_enc", 512}, {"precision", 0},
                                 {"mem", TTS_HIP_MEM_HOST}, {"ready", 1}, {"spk_dim", 0}, {"masks", 0}};
    std::string nulls;
    std::vector<int32_t> lens;
    for (int i = 3; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            lens.push_back((int32_t)atoi(argv[i]));
            continue;
        }
        std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "T" || key == "max_len") key = "len";
        if (key == "null") nulls = eq + 1;
        else if (v.count(key)) v[key] = atoi(eq + 1);
        else return 2;
    }
    const auto null = [&](const char* name) { return nulls.find(name) != std::string::npos; };
    const int B = lens.empty() ? v["B"] : (int)lens.size();
    if (lens.empty() && B > 0 && B <= (1 << 20)) lens.assign((size_t)B, (int32_t)v["len"]);
    char why[256] = "";
    int rc = TTS_HIP_OK;
    if (kind == "encode" || kind == "infer") {
        const TacoEncode c{"who", v["ready"] != 0, v["spk_dim"], null("tokens") ? nullptr : &tokens, B, v["Tin"],
                           null("speaker") ? nullptr : &mel, v["mem"], nullptr};
        rc = taco_encode_check(c, why, sizeof why);
    }
    TacoRun c{};
    if (kind != "encode" && !rc) {
        c.who = "who", c.kind = kind == "forward" ? TACO_FORWARD : TACO_DECODE, c.model_ready = v["ready"] != 0;
        c.has_encoded = kind == "infer" || !null("encoded"), c.B = B, c.Tin = v["Tin"], c.model_enc = v["model_enc"];
        c.enc = kind == "infer" ? c.model_enc : v["enc"], c.len = v["len"], c.precision = v["precision"], c.mem = v["mem"];
        c.masks = (TacoMasks)v["masks"], c.prenet_masks = &mel, c.keys = null("keys") ? nullptr : &keys;
        c.offsets = null("offsets") ? nullptr : &offsets, c.mel_input = null("mel") ? nullptr : &mel;
        c.mel_lengths = null("lens") || lens.empty() ? nullptr : lens.data();
        if (kind != "decode" && kind != "forward" && kind != "infer") return 2;
        rc = taco_run_check(c, why, sizeof why);
    }
    printf("%d %s\n", rc, why);
    if (rc || kind != "forward") return 0;
    const TacoForwardSizes z = taco_forward_sizes(c.B, c.len, c.enc);
    printf("%lld %zu %zu %zu %zu %zu\n", z.frames, z.mel_in, z.prenet, z.gates, z.history, z.proj);
    return 0;
}

static int print_taco_loss(int argc, char** argv) {
    // never read: the check only tests the pointers' values
    const auto at = [](unsigned long long a) { return (const float*)(uintptr_t)a; };
    std::map<std::string, double> v{{"B", 1}, {"T", 1}, {"mem", TTS_HIP_MEM_HOST}, {"mask", 1}, {"logits", 0},
                                    {"fw", 1}, {"nfw", 1}};
    std::string nulls, odd;
    std::vector<int32_t> kinds;
    int n_kinds = 0;
    bool n_given = false;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            kinds.push_back((int32_t)atoi(argv[i]));
            continue;
        }
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "null") nulls = eq + 1;
        else if (key == "odd") odd = eq + 1;
        else if (key == "n_kinds") n_kinds = atoi(eq + 1), n_given = true;
        else if (v.count(key)) v[key] = atof(eq + 1);
        else return 2;
    }
    if (!n_given) n_kinds = (int)kinds.size();
    kinds.resize(std::max<size_t>(kinds.size(), kLossMaxKinds), 0);
    const auto ptr = [&](const char* name, unsigned long long a) {
        if (nulls.find(name) != std::string::npos) return (const float*)nullptr;
        return at(odd.find(name) != std::string::npos ? a + 4 : a);
    };
    const TacoLossCall c{"who", ptr("target", 0x100000000ull), ptr("gate", 0x200000000ull), ptr("dec", 0x300000000ull),
                         ptr("mel", 0x400000000ull), ptr("stop", 0x500000000ull), (int)v["B"], (int)v["T"],
                         nulls.find("kinds") != std::string::npos ? nullptr : kinds.data(), n_kinds, v["mask"] != 0,
                         v["logits"] != 0, v["fw"], v["nfw"], const_cast<float*>(ptr("out", 0x600000000ull)), (int)v["mem"], nullptr};
    char why[256] = "";
    const int rc = taco_loss_check(c, why, sizeof why);
    printf("%d %s\n", rc, why);
    if (rc) return 0;
    const TacoLossLayout l = taco_loss_layout(c);
    printf("%d %d %d %zu\n", l.K, l.chunks, (int)l.weighted, l.bytes);
    return 0;
}

static int print_mel_dtw(int argc, char** argv) {
    std::map<std::string, int> v{{"B", 1}, {"Ta", 1}, {"Tb", 1}, {"n_mel", 80}, {"n_cep", 13}, {"flags", TTS_HIP_DTW_ALIGN},
                                 {"mem", TTS_HIP_MEM_HOST}, {"probe", 0}, {"what", -1}, {"path", 0}, {"dct", 0}};
    std::string nulls;
    std::vector<int32_t> la, lb;
    bool has_la = false, has_lb = false;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "null") nulls = eq + 1;
        else if (key == "la" || key == "lb") {
            std::vector<int32_t>& t = key == "la" ? la : lb;
            (key == "la" ? has_la : has_lb) = true;
            for (const char* p = eq + 1; *p;) {
                char* end = nullptr;
                t.push_back((int32_t)strtol(p, &end, 10));
                if (end == p) return 2;
                p = *end == ',' ? end + 1 : end;
            }
        } else if (v.count(key)) v[key] = atoi(eq + 1);
        else return 2;
    }
    // a table shorter than B would be read past its end by the check: that is the caller's contract, not the check's
    if ((has_la && (long long)la.size() < v["B"]) || (has_lb && (long long)lb.size() < v["B"])) return 2;
    // never read: the check only tests the pointers' values
    const auto ptr = [&](const char* name, unsigned long long a) {      // (whole names: "stats" holds an "a")
        return ("," + nulls + ",").find(std::string(",") + name + ",") != std::string::npos ? nullptr : (void*)(uintptr_t)a;
    };
    const MelDtwCall c{"who", (const float*)ptr("a", 0x100000000ull), (const float*)ptr("b", 0x200000000ull), v["B"], v["Ta"], v["Tb"],
                       v["n_mel"], has_la ? la.data() : nullptr, has_lb ? lb.data() : nullptr, v["n_cep"], v["flags"],
                       (float*)ptr("stats", 0x300000000ull), v["path"] ? (int32_t*)(uintptr_t)0x400000000ull : nullptr, v["probe"] != 0,
                       v["what"], (float*)ptr("out", 0x500000000ull), v["mem"], nullptr};
    char why[256] = "";
    const int rc = mel_dtw_check(c, why, sizeof why);
    printf("%d %s\n", rc, why);
    if (rc) return 0;
    const MelDtwLayout l = mel_dtw_layout(c);
    printf("%d %d %d %d %d\n", l.R, l.W, l.K, (int)l.skew_i, (int)l.aligned);
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.in_a, l.in_b, l.lens, l.cep_a, l.cep_b, l.dist, l.step, l.cost,
           l.final_cost, l.stats, l.path, l.out, l.out_elems, l.bytes);
    if (v["dct"]) {
        const std::vector<float> D = mel_dtw_dct(c.n_mel, c.n_cep, (c.flags & TTS_HIP_DTW_C0) != 0);
        if (D.size() != (size_t)l.R * c.n_mel) return 2;
        for (float x : D) printf("%.9g\n", x);
    }
    return 0;
}

static int print_pitch(int argc, char** argv) {
    std::map<std::string, long long> v{{"B", 1}, {"N", 4096}, {"rate", 22050}, {"hop", 256}, {"win", 1024}, {"tau_min", 45},
                                       {"tau_max", 367}, {"mem", TTS_HIP_MEM_HOST}, {"probe", 0}, {"what", -1}, {"f0", 0}, {"Fa", 1},
                                       {"Fb", 1}, {"P", 1}, {"path", 0}};
    std::map<std::string, double> f{{"threshold", 0.1}, {"gross", 315.64}};
    std::map<std::string, std::vector<int32_t>> tables;
    std::string nulls;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "null") nulls = eq + 1;
        else if (key == "len" || key == "la" || key == "lb") {
            std::vector<int32_t>& t = tables[key];
            for (const char* p = eq + 1; *p;) {
                char* end = nullptr;
                t.push_back((int32_t)strtol(p, &end, 10));
                if (end == p) return 2;
                p = *end == ',' ? end + 1 : end;
            }
        } else if (f.count(key)) f[key] = strtod(eq + 1, nullptr);
        else if (v.count(key)) v[key] = atoll(eq + 1);
        else return 2;
    }
    // a table shorter than B would be read past its end by the check: that is the caller's contract, not the check's
    for (const auto& kv : tables)
        if ((long long)kv.second.size() < v["B"]) return 2;
    const auto table = [&](const char* name) { return tables.count(name) ? tables[name].data() : (const int32_t*)nullptr; };
    // never read: the checks only test the pointers' values
    const auto ptr = [&](const char* name, unsigned long long a) {
        return ("," + nulls + ",").find(std::string(",") + name + ",") != std::string::npos ? nullptr : (void*)(uintptr_t)a;
    };
    char why[256] = "";
    if (v["f0"]) {
        const F0ErrorCall c{"who", (const float*)ptr("f0_a", 0x100000000ull), (const float*)ptr("f0_b", 0x200000000ull), (int)v["B"],
                            (int)v["Fa"], (int)v["Fb"], table("la"), table("lb"),
                            v["path"] ? (const int32_t*)(uintptr_t)0x400000000ull : nullptr, (int)v["P"], (float)f["gross"],
                            (float*)ptr("stats", 0x300000000ull), (int)v["mem"], nullptr};
        const int rc = f0_error_check(c, why, sizeof why);
        printf("%d %s\n", rc, why);
        if (rc) return 0;
        const F0ErrorLayout l = f0_error_layout(c);
        printf("%zu %zu %zu %zu %zu %zu\n", l.lens, l.in_a, l.in_b, l.path, l.stats, l.bytes);
        return 0;
    }
    const PitchCall c{"who", (const float*)ptr("audio", 0x100000000ull), (int)v["B"], (int)v["N"], table("len"), (int)v["rate"],
                      (int)v["hop"], (int)v["win"], (int)v["tau_min"], (int)v["tau_max"], (float)f["threshold"], v["probe"] != 0,
                      (int)v["what"], (float*)ptr("out", 0x500000000ull), (int)v["mem"], nullptr};
    const int rc = pitch_check(c, why, sizeof why);
    printf("%d %s\n", rc, why);
    if (rc) return 0;
    const PitchLayout l = pitch_layout(c);
    printf("%d %d %zu %zu %zu %zu %zu\n", l.F, l.threads, l.lens, l.in, l.out, l.out_elems, l.bytes);
    return 0;
}

static int print_pyin(int argc, char** argv) {
    std::map<std::string, long long> v{{"B", 1}, {"N", 4096}, {"rate", 22050}, {"hop", 256}, {"win", 1024}, {"tau_min", 45},
                                       {"tau_max", 367}, {"mem", TTS_HIP_MEM_HOST}, {"probe", 0}, {"what", -1}, {"n_bins", 368},
                                       {"bps", 10}, {"max_step", 51}, {"n_thresh", 4}, {"tables", 0}};
    std::map<std::string, double> f{{"switch", 0.01}, {"no_trough", 0.01}, {"fmin", 60.0}};
    std::vector<int32_t> len;
    std::vector<float> prior;
    bool have_prior = false;
    std::string nulls;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "null") nulls = eq + 1;
        else if (key == "len" || key == "prior") {
            have_prior |= key == "prior";
            for (const char* p = eq + 1; *p;) {
                char* end = nullptr;
                if (key == "len") len.push_back((int32_t)strtol(p, &end, 10));
                else prior.push_back((float)strtod(p, &end));
                if (end == p) return 2;
                p = *end == ',' ? end + 1 : end;
            }
        } else if (f.count(key)) f[key] = strtod(eq + 1, nullptr);
        else if (v.count(key)) v[key] = atoll(eq + 1);
        else return 2;
    }
    const auto null = [&](const char* name) { return ("," + nulls + ",").find(std::string(",") + name + ",") != std::string::npos; };
    // tables shorter than the check reads would be read past their end: that is the caller's contract, not the check's
    if (!len.empty() && (long long)len.size() < v["B"]) return 2;
    const long long n_thresh = v["n_thresh"];
    if (!have_prior && n_thresh >= 1 && n_thresh <= kPyinMaxThresh) prior.assign((size_t)n_thresh, 1.f / (float)n_thresh);
    if (!null("prior") && n_thresh >= 1 && n_thresh <= kPyinMaxThresh && (long long)prior.size() < n_thresh) return 2;
    // audio and out are never read: the checks only test the pointers' values
    const PyinCall c{PitchCall{"who", null("audio") ? nullptr : (const float*)(uintptr_t)0x100000000ull, (int)v["B"], (int)v["N"],
                               len.empty() ? nullptr : len.data(), (int)v["rate"], (int)v["hop"], (int)v["win"], (int)v["tau_min"],
                               (int)v["tau_max"], 0.5f, false, -1, null("out") ? nullptr : (float*)(uintptr_t)0x500000000ull, (int)v["mem"],
                               nullptr},
                     null("prior") ? nullptr : prior.data(), (int)n_thresh, (float)f["no_trough"], f["fmin"], (int)v["bps"], (int)v["n_bins"],
                     (int)v["max_step"], (float)f["switch"], v["probe"] != 0, (int)v["what"]};
    char why[256] = "";
    const int rc = pyin_check(c, why, sizeof why);
    printf("%d %s\n", rc, why);
    if (rc) return 0;
    const PyinLayout l = pyin_layout(c);
    printf("%d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.F, l.threads, l.vit_threads, l.lens, l.in, l.out, l.cum, l.tables,
           l.obs, l.cand, l.vprob, l.back, l.path, l.out_elems, l.bytes);
    if (v["tables"]) {                                          // the host tables, one value a line: cum, then the transition tables
        std::vector<float> cum((size_t)c.n_thresh + 1), tab((size_t)c.max_step + 1 + c.n_bins + 2);
        pyin_tables(c, cum.data(), tab.data());
        for (float x : cum) printf("%.9g\n", x);
        for (float x : tab) printf("%.9g\n", x);
    }
    return 0;
}

static int print_time_stretch(int argc, char** argv) {
    // never read: the check only tests the pointers' values
    const float* audio = (const float*)(uintptr_t)0x100000000ull;
    float* out = (float*)(uintptr_t)0x200000000ull;
    std::map<std::string, double> v{{"B", -1}, {"N", 0}, {"M", 0}, {"mem", TTS_HIP_MEM_DEVICE}, {"what", -1}, {"mel_kind", 0},
                                    {"filter_length", 1024}, {"hop_length", 256}, {"win_length", 1024}, {"pre_emph", 0},
                                    {"helpers", 0}};
    std::string nulls;
    std::vector<int32_t> lengths;
    std::vector<double> rates;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            lengths.push_back((int32_t)atoi(argv[i]));
            continue;
        }
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "null") nulls = eq + 1;
        else if (key == "rates") {
            for (const char* p = eq + 1; *p;) {
                char* end = nullptr;
                rates.push_back(strtod(p, &end));
                if (end == p) return 2;
                p = *end == ',' ? end + 1 : end;
            }
        } else if (v.count(key)) v[key] = atof(eq + 1);
        else return 2;
    }
    const auto null = [&](const char* name) { return ("," + nulls + ",").find(std::string(",") + name + ",") != std::string::npos; };
    const int B = lengths.empty() ? (int)v["B"] : (int)lengths.size(), N = (int)v["N"];
    // a table shorter than B would be read past its end by the check: that is the caller's contract, not the check's
    if (rates.size() == 1 && B > 1 && B <= (1 << 20)) rates.assign((size_t)B, rates[0]);
    if (!null("rates") && B > 0 && (long long)rates.size() < B) return 2;
    const tts_hip_mel_config cfg{(int)v["mel_kind"], 22050, 1, (int)v["filter_length"], (int)v["hop_length"], (int)v["win_length"], 0, 0.0,
                                 11025.0, v["pre_emph"]};
    char why[256] = "";
    MelPlan p{};
    int rc = mel_cfg_check("who", &cfg, nullptr, true, &p, why, sizeof why);
    if (!rc && v["helpers"] != 0) {                             // the two host-only helpers, one line "frames samples" per row
        if (rates.size() < lengths.size()) return 2;
        printf("0 \n");
        for (size_t b = 0; b < lengths.size(); ++b)
            printf("%d %lld\n", ts_row_frames(p, lengths[b], rates[b]), ts_row_samples(p, lengths[b], rates[b]));
        return 0;
    }
    TsGeom g;
    if (!rc)
        rc = time_stretch_check("who", null("fn") ? nullptr : &p, null("audio") ? nullptr : audio, B, N,
                                lengths.empty() ? nullptr : lengths.data(), null("rates") ? nullptr : rates.data(),
                                null("out") ? nullptr : out, (int)v["M"], (int)v["mem"], (int)v["what"], &g, why, sizeof why);
    printf("%d %s\n", rc, why);
    if (rc) return 0;
    if ((int)g.fwd.lens.size() != B || (int)g.fwd.fout.size() != B || (int)g.inv.frames.size() != B || (int)g.S.size() != B ||
        (int)g.keep.size() != B || (int)g.rates.size() != B)
        return 2;
    printf("%d %d %d\n", g.fwd.Fr, g.inv.F, g.M);
    printf("%zu %zu %zu %zu %zu %zu\n", g.off_rowinfo, g.off_mag, g.off_owner, g.off_adv, g.off_rel, g.inv.total);
    for (int b = 0; b < B; ++b) printf("%d%c", g.fwd.fout[b], b == B - 1 ? '\n' : ' ');
    for (int b = 0; b < B; ++b) printf("%d%c", g.inv.frames[b], b == B - 1 ? '\n' : ' ');
    for (int b = 0; b < B; ++b) printf("%d%c", g.S[b], b == B - 1 ? '\n' : ' ');
    for (int b = 0; b < B; ++b) printf("%d%c", g.keep[b], b == B - 1 ? '\n' : ' ');
    return 0;
}

static int print_formant_match(int argc, char** argv) {
    // never read: the check only tests the pointers' values
    const float* audio = (const float*)(uintptr_t)0x100000000ull;
    float* out = (float*)(uintptr_t)0x200000000ull;
    std::map<std::string, double> v{{"B", -1}, {"N", 0}, {"Q", 33}, {"max_gain_db", 24}, {"mem", TTS_HIP_MEM_DEVICE}, {"what", -1},
                                    {"mel_kind", 0}, {"filter_length", 1024}, {"hop_length", 256}, {"win_length", 1024},
                                    {"pre_emph", 0}, {"table", 0}};
    std::string nulls;
    std::vector<int32_t> lengths;
    std::vector<double> warps;
    bool have_warps = false;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            lengths.push_back((int32_t)atoi(argv[i]));
            continue;
        }
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        if (key == "null") nulls = eq + 1;
        else if (key == "warps") {
            have_warps = true;
            for (const char* p = eq + 1; *p;) {
                char* end = nullptr;
                warps.push_back(strtod(p, &end));
                if (end == p) return 2;
                p = *end == ',' ? end + 1 : end;
            }
        } else if (v.count(key)) v[key] = atof(eq + 1);
        else return 2;
    }
    const auto null = [&](const char* name) { return ("," + nulls + ",").find(std::string(",") + name + ",") != std::string::npos; };
    const int B = lengths.empty() ? (int)v["B"] : (int)lengths.size(), N = (int)v["N"];
    // a table shorter than B would be read past its end by the check: that is the caller's contract, not the check's
    if (warps.size() == 1 && B > 1 && B <= (1 << 20)) warps.assign((size_t)B, warps[0]);
    if (have_warps && B > 0 && (long long)warps.size() < B) return 2;
    const tts_hip_mel_config cfg{(int)v["mel_kind"], 22050, 1, (int)v["filter_length"], (int)v["hop_length"], (int)v["win_length"], 0, 0.0,
                                 11025.0, v["pre_emph"]};
    char why[256] = "";
    MelPlan p{};
    int rc = mel_cfg_check("who", &cfg, nullptr, true, &p, why, sizeof why);
    if (!rc && v["table"] != 0) {                               // the liftering table alone, one value a line
        const int Q = (int)v["Q"];
        if (Q < 0 || Q > p.fl) return 2;
        std::vector<double> L;
        fm_lifter_table(p.fl, Q, L);
        printf("0 \n");
        for (double x : L) printf("%.17g\n", x);
        return 0;
    }
    FmGeom g;
    if (!rc)
        rc = formant_match_check("who", null("fn") ? nullptr : &p, null("audio") ? nullptr : audio, B, N,
                                 lengths.empty() ? nullptr : lengths.data(), have_warps ? warps.data() : nullptr, (int)v["Q"],
                                 v["max_gain_db"], null("out") ? nullptr : out, (int)v["mem"], (int)v["what"], &g, why, sizeof why);
    printf("%d %s\n", rc, why);
    if (rc) return 0;
    if ((int)g.fwd.lens.size() != B || (int)g.fwd.fout.size() != B || (int)g.inv.frames.size() != B || (int)g.keep.size() != B ||
        (int)g.warps.size() != B)
        return 2;
    uint32_t gbits;
    memcpy(&gbits, &g.G, 4);
    printf("%d %d %u\n", g.fwd.Fr, g.Q, gbits);
    printf("%zu %zu %zu %zu %zu\n", g.off_warps, g.off_logmag, g.off_env, g.off_gain, g.inv.total);
    for (int b = 0; b < B; ++b) printf("%d%c", g.inv.frames[b], b == B - 1 ? '\n' : ' ');
    for (int b = 0; b < B; ++b) printf("%d%c", g.keep[b], b == B - 1 ? '\n' : ' ');
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--formant-match")) return print_formant_match(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "--time-stretch")) return print_time_stretch(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "--pitch")) return print_pitch(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "--pyin")) return print_pyin(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "--mel-dtw")) return print_mel_dtw(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "--taco-loss")) return print_taco_loss(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "--taco-call")) return print_taco_call(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "--audio-call")) return print_audio_call(argc, argv);
    if (argc >= 5 && !strcmp(argv[1], "--wg-call")) return print_wg_call(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "--wg-encode")) return print_wg_encode(argc, argv);
    if (argc >= 5 && !strcmp(argv[1], "--wn-taps")) {
        std::vector<int> lens;
        for (int i = 4; i < argc; ++i) lens.push_back(atoi(argv[i]));
        return print_wn_taps(atoi(argv[2]), atoi(argv[3]), lens);
    }
    if ((argc == 4 || argc == 5) && !strcmp(argv[1], "--wg-plan")) {
        const int step = argc == 5 ? atoi(argv[4]) : 1;
        return step > 0 ? print_wg_plans(atoi(argv[2]), atoi(argv[3]), step) : 2;
    }
    bool load = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--load")) {
            load = true;
            continue;
        }
        std::map<std::string, HostTensor> tensors;
        std::string err;
        const int rc = parse_ttsw(argv[i], load ? &tensors : nullptr, &err);
        size_t floats = 0;
        for (auto& kv : tensors) {
            floats += kv.second.data.size();
            if (kv.second.numel() != kv.second.data.size()) return 2;          // dims and payload must agree after a load
        }
        printf("%d %zu %zu %s\n", rc, tensors.size(), floats, err.c_str());
    }
    return 0;
}
