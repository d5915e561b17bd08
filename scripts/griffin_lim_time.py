"""Timing: Griffin-Lim on the GPU (`TacotronSTFT.mel_to_audio`, csrc/stft_inv.hip) -- 60 iterations on an 80 x 800 log-mel at
batch 1 and 8, device tensors, the default plan (1024 / 256 / 1024).  Every timed window ends in a synchronise.

  python scripts/griffin_lim_time.py [--reps N] [--iters N]

Prints one JSON line per batch size: the call's median time, then from a separate pass with the engine's launch timing
(tts_hip_kernel_timing: the event pairs serialise the launches) the average time of the four parts of an iteration
(inverse-frames GEMM, gather overlap-add, forward DFT GEMM, phase update) and the share of the fp32 MFMA peak the two GEMMs
reach against 2 * 2 * F * 2 * bins * filter_length FLOP per row and iteration, the peak being what tts_hip_probe_mfma_f32
measures on this device in the same run."""
import argparse, json, time
import os, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--iters', type=int, default=60)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_to_speech_amd.engine import HipEngine
from text_to_speech_amd.stft import TacotronSTFT

F, NMEL, FL, BINS = 800, 80, 1024, 513
PARTS = ('inverse_gemm', 'overlap_add', 'forward_gemm', 'phase_update')
eng = HipEngine(0)
fn = TacotronSTFT(engine=eng)
rng = np.random.default_rng(7)
peak_tflops, clock = eng.probe_mfma_f32()
for B in (1, 8):
    audio = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, (F - 1) * 256)).astype(np.float32)).cuda()
    mel = fn(audio)                                                     # a mel a real signal has
    assert tuple(mel.shape) == (B, F, NMEL)
    call = lambda: fn.mel_to_audio(mel, n_iters=args.iters, momentum=0.99)
    call()                                                              # warm-up: tables, workspace
    ms = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    out = {'B': B, 'F': F, 'iters': args.iters, 'call_ms_median': float(np.median(ms)), 'call_ms_min_max': [min(ms), max(ms)]}
    eng.kernel_timing(True)
    call()
    us = [eng.kernel_time_us(kind) for kind in range(4)]
    eng.kernel_timing(False)
    out['part_us_avg_n'] = {name: [float(u), int(n)] for name, (u, n) in zip(PARTS, us)}
    flop = 2.0 * B * F * 2 * BINS * FL                                  # one GEMM of one iteration
    gemm_us = us[0][0] + us[2][0]
    out['gemm_tflops'] = 2 * flop / (gemm_us * 1e-6) / 1e12 if gemm_us else 0.0
    out['mfma_f32_peak_tflops'] = peak_tflops
    out['gemm_share_of_peak'] = out['gemm_tflops'] / peak_tflops if peak_tflops else 0.0
    print(json.dumps(out))
eng.close()
