"""Time of the MCD-DTW call (HipEngine.mel_dtw) on 8 pairs of 800 x 900 frames, per kernel and in total, beside the free-running
decode it follows in `Tacotron2.evaluate_synthesis` (HipEngine.tacotron2_infer: 8 rows of 128 tokens, 800 frames each, no early
stop, synthetic weights; uses TTS_HIP_LIBRARY if set).  Everything is on the device: CUDA tensors in, CUDA tensors out.

One process; a warm-up round (code objects, workspaces, the decoder's graphs), then ROUNDS rounds in which the calls alternate.
A figure is the wall time of one call (it ends in a stream synchronise: what a caller pays), median over the rounds.  The
per-kernel figures come from the engine's event timing (tts_hip_kernel_timing: a mel_dtw call files its cepstra, distance, sweep
and path launches under kinds 0 .. 3), taken in rounds of their own so that the events do not sit in the wall times.
`a` is the decoder's own mel, `b` a seeded log-mel-like target; also timed: the same call without the path, and without
alignment.  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from text_to_speech_amd import config, weights  # noqa: E402
from text_to_speech_amd.engine import HipEngine  # noqa: E402

B, TIN, TA, TB, ROUNDS = 8, 128, 800, 900, 7


def log_mel(rng, T, n_mel=80):
    """[T, n_mel] float32, log-mel-like: a spectral tilt plus noise smoothed over nine frames, clipped to [ln 1e-5, 2]"""
    x = rng.standard_normal((T + 8, n_mel))
    x = sum(x[s:s + T] for s in range(9)) / 3.0
    return np.clip(-4.0 - 4.0 * np.arange(n_mel) / n_mel + 2.5 * x, np.log(1e-5), 2.0).astype(np.float32)


eng = HipEngine(0)
eng.load_state(weights.synth_tacotron2(config.Tacotron2Config(), seed=1234))
eng.finalize()
rng = np.random.default_rng(0)
tok = torch.from_numpy(rng.integers(1, 148, (B, TIN)).astype(np.int32)).cuda()
target = torch.from_numpy(np.stack([log_mel(rng, TB) for _ in range(B)])).cuda()
calls = {
    'infer': lambda: eng.tacotron2_infer(tok, max_len=TA, early_stopping=False, want_attention=False),
    'dtw_path': lambda: eng.mel_dtw(mel, target, return_path=True),
    'dtw': lambda: eng.mel_dtw(mel, target),
    'unaligned': lambda: eng.mel_dtw(mel, target, align=False),
}
times = {k: [] for k in calls}
mel = None
for r in range(ROUNDS + 1):
    for name, call in calls.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        dt = time.perf_counter() - t0
        if name == 'infer':
            mel = out.mel
        if r > 0:
            times[name].append(dt)
stats = eng.mel_dtw(mel, target).cpu().numpy()
kernels = {}
eng.kernel_timing(True)
for _ in range(ROUNDS):
    eng.mel_dtw(mel, target, return_path=True)
for kind, name in enumerate(('cepstra', 'distance', 'sweep', 'path')):
    kernels[name + '_us'] = round(eng.kernel_time_us(kind)[0], 1)
eng.kernel_timing(False)
eng.close()
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps({'B': B, 'Ta': TA, 'Tb': TB, 'Tin': TIN, 'n_cep': 13, 'infer_ms': round(med['infer'] * 1e3, 2),
                  'dtw_path_ms': round(med['dtw_path'] * 1e3, 3), 'dtw_ms': round(med['dtw'] * 1e3, 3),
                  'unaligned_ms': round(med['unaligned'] * 1e3, 3), **kernels,
                  'dtw_share_of_infer': round(med['dtw'] / med['infer'], 5),
                  'sweep_steps': sum(-(-(TA + min(256, TB - j0) - 1) // 8) * 8 for j0 in range(0, TB, 256)),      # strips of 256 columns, rounds of 8
                  'mean_mcd_db': round(float(stats[2].mean()), 2), 'mean_path_len': round(float(stats[1].mean()), 1),
                  'rounds_ms': {k: [round(v * 1e3, 3) for v in times[k]] for k in ('dtw_path', 'dtw', 'unaligned')}}), flush=True)
