"""Timing: WaveGlow on a batch of unequal rows -- the packed call (`waveglow_infer(..., lengths=..., packed=True)`: the real
frames of all rows in ONE row, 4 gap frames between two rows) against the ragged call on the same shape (every row padded
to the longest).  B = 8, T = 800, config-3-like lengths (F = 3 164 packed frames against 6 400); each precision; device
tensors; every shape warmed, every timed window ends in a synchronise, the calls alternate.

  python scripts/packed_time.py [--root DIR] [--mode both|packed|ragged] [--reps N]

--root: the tree whose `text_to_speech_amd` is imported (default: this one) -- `--root <checkout of an older commit> --mode
ragged` times that commit's ragged call; run the two trees in turn within one visit to the GPU to compare them.  Prints one
JSON line; `rows_run` are the GEMM rows per phase the call ran (its frames rounded up to the tile it chose)."""
import argparse, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--mode', default='both', choices=('both', 'packed', 'ragged'))
ap.add_argument('--reps', type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch
from text_to_speech_amd import weights
from text_to_speech_amd.config import WaveGlowConfig
from text_to_speech_amd.engine import HipEngine

B, T, GAP = 8, 800, 4
LENGTHS = [800, 523, 77, 1, 640, 799, 300, 0]
F = sum(LENGTHS) + GAP * (sum(n > 0 for n in LENGTHS) - 1)
TILE_ROWS = {'256-row': 256, '128-row': 128, '128x64': 128, '64-row': 64}
eng = HipEngine(0)
eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=1234))
eng.finalize()
rng = np.random.default_rng(7)
mel = rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
mel = torch.from_numpy(mel).cuda()
z = torch.from_numpy(rng.standard_normal((B, T * 32, 8)).astype(np.float32)).cuda()
calls = {'ragged': lambda p: eng.waveglow_infer(mel, z=z, precision=p, lengths=LENGTHS),
         'packed': lambda p: eng.waveglow_infer(mel, z=z, precision=p, lengths=LENGTHS, packed=True)}
frames = {'ragged': B * T, 'packed': F}
modes = ('ragged', 'packed') if args.mode == 'both' else (args.mode,)
out = {'root': os.path.abspath(args.root), 'B': B, 'T': T, 'lengths': LENGTHS, 'real_frames': sum(LENGTHS), 'packed_frames': F}
for prec in ('f32', 'f16x3', 'f16'):
    rows = {}
    for m in modes:
        calls[m](prec)                                   # warm-up (returns after the engine's stream drained)
        tile = TILE_ROWS[eng.last_waveglow_tiles]
        rows[m] = -(-frames[m] // tile) * tile
        out[f'{prec}_{m}_form_tiles_rows_run'] = [eng.last_waveglow_form, eng.last_waveglow_tiles, rows[m]]
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
    if len(modes) == 2:
        out[f'{prec}_packed_over_ragged_time'] = out[f'{prec}_packed_ms_median'] / out[f'{prec}_ragged_ms_median']
        out[f'{prec}_packed_over_ragged_rows'] = rows['packed'] / rows['ragged']
eng.close()
print(json.dumps(out))
