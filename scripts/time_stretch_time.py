"""Timing: time stretching on the GPU (`HipEngine.time_stretch`, csrc/stft_inv.hip) on the benchmark's audio, [8, 204 800]
samples under the default plan (1024 / 256 / 1024), device tensors, at the rates 0.5, 1.25 and 2, and its share of the vocoder
step it follows.

  python scripts/time_stretch_time.py [--reps N] [--step-reps N]

Prints one JSON line.  Per rate: the whole call between HIP events (warm, `--reps` calls per window, median of 5 windows); from
a separate pass with the engine's launch timing (tts_hip_kernel_timing: the event pairs serialise the launches) the average
time of the five parts (forward DFT with its padding, the vocoder's parallel pass, its chain over the frames, inverse-frames
GEMM, overlap-add) and the chain's time per output frame.  Then, in the same run, `HipRuntime.waveglow_infer` fp32 at batch
8 x 800 frames (host clock around calls that end in a synchronise, median of `--step-reps`), with each rate's call as a share
of that step."""
import argparse, json, time
import os, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--step-reps', type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_to_speech_amd import effects
from text_to_speech_amd.runtime import HipRuntime

B, T = 8, 800
RATES = (0.5, 1.25, 2.0)
PARTS = ('inverse_gemm', 'overlap_add', 'forward_dft', 'parallel_pass', 'chain')    # the timing kinds 0 .. 4
rt = HipRuntime('synthetic', model='waveglow', seed=1)
eng = rt.engine
plan = effects.default_plan(eng)
rng = np.random.default_rng(7)
t = np.arange(T * 256) / 22050.0
tone = 0.4 * np.sin(2 * np.pi * 220.3 * t) + 0.1 * np.sin(2 * np.pi * 683.0 * t)
audio = torch.from_numpy((tone[None] + rng.uniform(-0.05, 0.05, (B, T * 256))).astype(np.float32)).cuda()
out = {'B': B, 'samples': T * 256, 'rates': {}}
for rate in RATES:
    call = lambda: eng.time_stretch(plan, audio, rate)
    for _ in range(3):
        call()                                                          # warm-up: tables, workspaces
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
    frames = eng._lib.tts_hip_time_stretch_frames(plan.handle, T * 256, float(rate))
    row = {'out_frames': int(frames), 'call_ms_median': float(np.median(windows)), 'call_ms_min_max': [min(windows), max(windows)]}
    eng.kernel_timing(True)
    for _ in range(10):
        call()
    us = [eng.kernel_time_us(kind) for kind in range(5)]
    eng.kernel_timing(False)
    row['part_us_avg_n'] = {name: [float(u), int(n)] for name, (u, n) in zip(PARTS, us)}
    row['parts_ms_sum'] = sum(u for u, _ in us) / 1e3
    row['chain_us_per_frame'] = us[4][0] / frames
    out['rates'][str(rate)] = row

mel = torch.from_numpy(rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)).cuda()
rt.waveglow_infer(mel, seed=3)                                          # warm-up
torch.cuda.synchronize()
step = []
for _ in range(args.step_reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rt.waveglow_infer(mel, seed=3)
    torch.cuda.synchronize()
    step.append((time.perf_counter() - t0) * 1e3)
plain = float(np.median(step))
out['waveglow_f32_step_ms'] = {'plain': plain, 'min_max': [min(step), max(step)]}
out['share_of_step'] = {r: row['call_ms_median'] / plain for r, row in out['rates'].items()}
print(json.dumps(out))
eng.close()
