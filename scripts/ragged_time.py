"""Timing: WaveGlow on a batch of unequal rows -- the ragged call (`waveglow_infer(..., lengths=...)`: every row's audio is that
of its own frames) against the padded call on the same shape (tails filled with -11; what a batch cost before per-row lengths).
B = 8, T = 800, config-3-like lengths; each precision; device tensors; every shape warmed, every timed window ends in a
synchronise, the two calls alternate.

  python scripts/ragged_time.py [--root DIR] [--mode both|padded|ragged] [--reps N]

--root: the tree whose `text_to_speech_amd` is imported (default: this one) -- `--root <checkout of an older commit> --mode
padded` times that commit's padded call for comparison.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--mode', default='both', choices=('both', 'padded', 'ragged'))
ap.add_argument('--reps', type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch
from text_to_speech_amd import weights
from text_to_speech_amd.config import WaveGlowConfig
from text_to_speech_amd.engine import HipEngine

B, T = 8, 800
LENGTHS = [800, 523, 77, 1, 640, 799, 300, 0]
eng = HipEngine(0)
eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=1234))
eng.finalize()
rng = np.random.default_rng(7)
mel = rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
for b, n in enumerate(LENGTHS):
    mel[b, n:] = -11.0
mel = torch.from_numpy(mel).cuda()
z = torch.from_numpy(rng.standard_normal((B, T * 32, 8)).astype(np.float32)).cuda()
calls = {'padded': lambda p: eng.waveglow_infer(mel, z=z, precision=p),
         'ragged': lambda p: eng.waveglow_infer(mel, z=z, precision=p, lengths=LENGTHS)}
modes = ('padded', 'ragged') if args.mode == 'both' else (args.mode,)
out = {'root': os.path.abspath(args.root), 'B': B, 'T': T, 'lengths': LENGTHS, 'tail_frames': B * T - sum(LENGTHS)}
for prec in ('f32', 'f16x3', 'f16'):
    for m in modes:
        calls[m](prec)                                   # warm-up (returns after the engine's stream drained)
    ms = {m: [] for m in modes}
    for _ in range(args.reps):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[m](prec)
            ms[m].append((time.perf_counter() - t0) * 1e3)
    for m in modes:
        out[f'{prec}_{m}_ms_median'] = float(np.median(ms[m]))
        out[f'{prec}_{m}_ms_min_max'] = [float(min(ms[m])), float(max(ms[m]))]
    out[f'{prec}_form_tiles'] = [eng.last_waveglow_form, eng.last_waveglow_tiles]
eng.close()
print(json.dumps(out))
