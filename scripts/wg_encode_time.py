"""Timing: WaveGlow's forward flow (`waveglow_encode`: audio -> z and its statistics) beside `waveglow_infer` on the same shape
in the same run.  B = 8, T = 800 (6 400 frames: the Winograd form), fp32, device tensors; both calls warmed, every timed
window ends in a synchronise, the calls alternate.

  python scripts/wg_encode_time.py [--reps N] [--kernels]

Prints one JSON line.  --kernels: also the engine's own launch timing of each direction (kernel_timing: [average us,
launches] of the kinds the driver times -- 1 is the residual GEMM, 84 launches a call), for saying where a difference between
the two directions lies."""
import argparse, json, time
import os, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--kernels', action='store_true')
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_to_speech_amd import weights
from text_to_speech_amd.config import WaveGlowConfig
from text_to_speech_amd.engine import HipEngine

B, T = 8, 800
eng = HipEngine(0)
eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=1234))
eng.finalize()
rng = np.random.default_rng(7)
mel = torch.from_numpy(rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)).cuda()
z = torch.from_numpy(rng.standard_normal((B, T * 32, 8)).astype(np.float32)).cuda()
audio = eng.waveglow_infer(mel, z=z)                                 # the model's own audio for z: encode returns z (warm-up too)
calls = {'infer': lambda: eng.waveglow_infer(mel, z=z), 'encode': lambda: eng.waveglow_encode(audio, mel)}
out = {'B': B, 'T': T}
for name, call in calls.items():
    res = call()                                                     # warm-up (returns after the engine's stream drained)
    out[f'{name}_form_tiles'] = [eng.last_waveglow_form, eng.last_waveglow_tiles]
z_back = res[0]
out['encode_of_infer_z_rms_err'] = float((z_back - z).double().pow(2).mean().sqrt())
ms = {name: [] for name in calls}
for _ in range(args.reps):
    for name, call in calls.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms[name].append((time.perf_counter() - t0) * 1e3)
for name in calls:
    out[f'{name}_ms_median'] = float(np.median(ms[name]))
    out[f'{name}_ms_min_max'] = [float(min(ms[name])), float(max(ms[name]))]
out['encode_over_infer_time'] = out['encode_ms_median'] / out['infer_ms_median']
if args.kernels:                                                     # kind 1: the residual GEMMs (plain in `encode`, with the
    for name, call in calls.items():                                 # end sums in `infer`); kinds 0 / 3: the direct form's in-layer GEMMs
        eng.kernel_timing(True)
        call()
        out[f'{name}_kernel_us_avg_n'] = [list(eng.kernel_time_us(kind)) for kind in range(4)]
        eng.kernel_timing(False)
eng.close()
print(json.dumps(out))
