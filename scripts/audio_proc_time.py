"""Timing of the waveform clean-up (csrc/audio_proc.hip) at batch 8 x 204 800 samples (800 mel frames) and 22 050 Hz.

  python scripts/audio_proc_time.py [--calls 20] [--no-tts]

Device tensors in and out (no PCIe in the figures); warm-up, synchronize, median of --calls timed calls (wall clock
around one call + synchronize).  Prints ms per call for reduce_noise and trim_silence (full and ragged batch), the GEMM
FLOP of the two DFT products and the share of the fp32 MFMA peak (157.3 TFLOP/s), the fp64 FLOP of the trim
convolution, and the batch-8 text -> audio time of TTSPipeline.synthesize_tokens with the clean-up keywords off and on.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/audio_proc_time.py --no-tts`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATE, B, N, PEAK_F32 = 22050, 8, 204800, 157.3e12


def median_ms(fn, calls, sync):
    for _ in range(3):
        fn()
    sync()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--no-tts', action='store_true')
    args = ap.parse_args()
    import torch
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    t = np.arange(N) / RATE
    host = (0.5 * np.sin(2 * np.pi * 220 * t)[None] * (t[None] > 0.5) + 0.02 * rng.standard_normal((B, N))).astype(np.float32)
    a = torch.as_tensor(host, device='cuda:0')
    ragged = np.array([N, N - 7000, N // 2 + 123, N // 3, 150000, 99999, 180000, 60000], np.int32)
    res = {}
    for name, lens in (('full', None), ('ragged', ragged)):
        res[f'reduce_noise_ms_{name}'] = median_ms(lambda: eng.reduce_noise(a, RATE, lengths=lens), args.calls, sync)
        res[f'trim_silence_ms_{name}'] = median_ms(lambda: eng.trim_silence(a, RATE, lengths=lens), args.calls, sync)
    Fr = (N + 2560 + 511) // 512                      # frame rows per batch row (the GEMM M), K = 2048, N = 2080
    gemm_flop = 2 * (2.0 * B * Fr * 2080 * 2048)
    W = 2 * (int(0.2 * RATE) // 2)
    trim_flop = 2.0 * B * (N - W + 1) * W
    res['dft_gemm_gflop'] = gemm_flop / 1e9
    res['dft_gemm_ms_at_peak'] = gemm_flop / PEAK_F32 * 1e3
    res['reduce_noise_share_of_f32_peak'] = gemm_flop / PEAK_F32 * 1e3 / res['reduce_noise_ms_full']
    res['trim_fp64_gflop'] = trim_flop / 1e9
    res['trim_fp64_tflops'] = trim_flop / (res['trim_silence_ms_full'] * 1e-3) / 1e12
    if not args.no_tts:
        from text_to_speech_amd import weights
        from text_to_speech_amd.config import Tacotron2Config, WaveGlowConfig
        from text_to_speech_amd.pipeline import TTSPipeline
        eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=1234))
        eng.load_state(weights.synth_tacotron2(Tacotron2Config(), seed=1234))
        eng.finalize()
        tok = rng.integers(1, 148, (B, 100)).astype(np.int32)
        p = TTSPipeline(eng, seed=0)
        kw = dict(deterministic=True, max_length=800, early_stopping=False)
        calls = max(3, args.calls // 4)
        res['tts_b8_800f_ms_off'] = median_ms(lambda: p.synthesize_tokens(tok, **kw), calls, sync)
        res['tts_b8_800f_ms_on'] = median_ms(lambda: p.synthesize_tokens(tok, reduce_noise=True, trim_silence=True, **kw),
                                             calls, sync)
    eng.close()
    print(json.dumps({k: round(v, 4) for k, v in res.items()}))


if __name__ == '__main__':
    main()
