"""Timing: the WaveGlow denoiser on the GPU (`HipEngine.denoise`, csrc/stft_inv.hip) on the benchmark's audio, [8, 204 800]
samples under the default plan (1024 / 256 / 1024), device tensors, and its share of the vocoder step it follows.

  python scripts/denoise_time.py [--reps N] [--step-reps N]

Prints one JSON line: the whole call between HIP events (warm, `--reps` calls per window, median of 5 windows); from a separate
pass with the engine's launch timing (tts_hip_kernel_timing: the event pairs serialise the launches) the average time of the
four parts (forward DFT with its padding, gate, inverse-frames GEMM, overlap-add); and, in the same run, `HipRuntime.
waveglow_infer` fp32 at batch 8 x 800 frames with `denoiser_strength` None and 0.01 (host clock around calls that end in a
synchronise, alternating, median of `--step-reps`), with the denoiser's cost as a share of that step."""
import argparse, json, time
import os, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--step-reps', type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_to_speech_amd.runtime import HipRuntime

B, T = 8, 800
PARTS = ('inverse_gemm', 'overlap_add', 'forward_dft', 'gate')          # the timing kinds 0 .. 3
rt = HipRuntime('synthetic', model='waveglow', seed=1)
eng = rt.engine
den = rt.denoiser('f32')
rng = np.random.default_rng(7)
audio = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, T * 256)).astype(np.float32)).cuda()
bias = den.bias
plan = den._plan()
call = lambda: eng.denoise(plan, audio, bias, 0.01)
for _ in range(3):
    call()                                                              # warm-up: tables, workspaces
windows = []
for _ in range(5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.reps):
        call()
    b.record()
    torch.cuda.synchronize()
    windows.append(a.elapsed_time(b) / args.reps)
out = {'B': B, 'samples': T * 256, 'call_ms_median': float(np.median(windows)), 'call_ms_min_max': [min(windows), max(windows)]}
eng.kernel_timing(True)
for _ in range(10):
    call()
us = [eng.kernel_time_us(kind) for kind in range(4)]
eng.kernel_timing(False)
out['part_us_avg_n'] = {name: [float(u), int(n)] for name, (u, n) in zip(PARTS, us)}
out['parts_ms_sum'] = sum(u for u, _ in us) / 1e3
flop = 2.0 * B * (T + 1) * 1024 * 1026                                  # one of the two GEMMs
out['gemm_tflops'] = {'forward_dft': flop / (us[2][0] * 1e-6) / 1e12 if us[2][0] else 0.0,
                      'inverse_gemm': flop / (us[0][0] * 1e-6) / 1e12 if us[0][0] else 0.0}

mel = torch.from_numpy(rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)).cuda()
step = {None: [], 0.01: []}
for s in step:
    rt.waveglow_infer(mel, seed=3, denoiser_strength=s)                 # warm-up of both paths
    torch.cuda.synchronize()
for _ in range(args.step_reps):
    for s in step:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.waveglow_infer(mel, seed=3, denoiser_strength=s)
        torch.cuda.synchronize()
        step[s].append((time.perf_counter() - t0) * 1e3)
plain, clean = float(np.median(step[None])), float(np.median(step[0.01]))
out['waveglow_f32_step_ms'] = {'plain': plain, 'denoised': clean, 'plain_min_max': [min(step[None]), max(step[None])],
                               'denoised_min_max': [min(step[0.01]), max(step[0.01])]}
out['denoise_share_of_step'] = out['call_ms_median'] / plain
print(json.dumps(out))
eng.close()
