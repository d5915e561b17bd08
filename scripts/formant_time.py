"""Timing: cepstral envelope matching on the GPU (`HipEngine.formant_match`, csrc/stft_inv.hip) on the benchmark's audio, [8, 204 800]
samples under the default plan (1024 / 256 / 1024, lifter cut 33), device tensors, and its share of the pitch shift it follows.

  python scripts/formant_time.py [--reps N] [--steps S]

Prints one JSON line: the whole call between HIP events with a source (two transforms) and against the audio itself (one), warm,
`--reps` calls per window, median of 5 windows; from a separate pass with the engine's launch timing (tts_hip_kernel_timing: the
event pairs serialise the launches) the average time and the launch count of the five parts (inverse-frames GEMM, overlap-add,
forward DFT with its padding, log-magnitudes with the envelope GEMM, gain); and, in the same run, `effects.pitch_shift` by
`--steps` semitones without and with `preserve_formants` (HIP events, alternating, median), with the matching's cost as a share
of the plain shift.  No target is set."""
import argparse, json
import os, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--steps', type=float, default=4.0)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_to_speech_amd import effects
from text_to_speech_amd.engine import HipEngine

B, T = 8, 800
PARTS = ('inverse_gemm', 'overlap_add', 'forward_dft', 'logmag_envelope_gemm', 'gain')     # the timing kinds 0 .. 4
eng = HipEngine(0)
plan = effects.default_plan(eng)
rng = np.random.default_rng(7)
audio = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, T * 256)).astype(np.float32)).cuda()
source = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, T * 256)).astype(np.float32)).cuda()


def windows(call, reps):
    for _ in range(3):
        call()                                                          # warm-up: tables, workspaces
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


with_source = windows(lambda: eng.formant_match(plan, audio, source, warp=1.0), args.reps)
on_itself = windows(lambda: eng.formant_match(plan, audio, None, warp=1.19), args.reps)
out = {'B': B, 'samples': T * 256, 'lifter': eng.default_lifter(plan),
       'call_ms_median': float(np.median(with_source)), 'call_ms_min_max': [min(with_source), max(with_source)],
       'self_call_ms_median': float(np.median(on_itself)), 'self_call_ms_min_max': [min(on_itself), max(on_itself)]}
eng.kernel_timing(True)
for _ in range(10):
    eng.formant_match(plan, audio, source)
us = [eng.kernel_time_us(kind) for kind in range(5)]
eng.kernel_timing(False)
out['part_us_avg_n'] = {name: [float(u), int(n)] for name, (u, n) in zip(PARTS, us)}
out['parts_ms_per_call'] = sum(u * n for u, n in us) / 10 / 1e3
rows = B * (T + 1)
# the envelope GEMM's flop over its kind's whole time (the two log-magnitude kernels included); the inverse GEMM alone
out['gemm_tflops'] = {'logmag_envelope_gemm': 2.0 * 2 * rows * 544 * 513 * 10 / (us[3][0] * us[3][1] * 1e-6) / 1e12 if us[3][0] else 0.0,
                      'inverse_gemm': 2.0 * rows * 1024 * 1056 / (us[0][0] * 1e-6) / 1e12 if us[0][0] else 0.0}

plain = windows(lambda: effects.pitch_shift(audio, args.steps, engine=eng), max(1, args.reps // 4))
kept = windows(lambda: effects.pitch_shift(audio, args.steps, engine=eng, preserve_formants=True), max(1, args.reps // 4))
out['pitch_shift_ms'] = {'steps': args.steps, 'plain': float(np.median(plain)), 'preserve_formants': float(np.median(kept)),
                         'plain_min_max': [min(plain), max(plain)], 'preserve_formants_min_max': [min(kept), max(kept)]}
out['formant_match_share_of_pitch_shift'] = out['call_ms_median'] / out['pitch_shift_ms']['plain']
print(json.dumps(out))
eng.close()
