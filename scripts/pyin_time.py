"""Time of the probabilistic-YIN call (HipEngine.pyin) at the defaults on 8 rows x 800 frames of device-resident audio, beside the
YIN call (HipEngine.pitch) on the same audio and the vocoder step that produces such audio (HipEngine.waveglow_infer: 8 rows of
800 frames, synthetic weights).  Uses TTS_HIP_LIBRARY if set.  Everything is on the device.

One process; a warm-up round, then ROUNDS rounds in which the calls alternate.  A figure is the time between two events on the
caller's stream around one call, median over the rounds.  The kernels alone come from the engine's event timing
(tts_hip_kernel_timing: a pitch call files its launch under kind 0, a pyin call its observation kernel under kind 2 and its
decode under kind 3; other calls file launches under the same kinds, so no other call runs while timing is on -- keep it so when
changing this script).

`decode_lds_reads`: the LDS reads one thread of the decode issues per frame (two sources and the triangle per bin of the window).
Prints one JSON line.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from text_to_speech_amd import config, weights  # noqa: E402
from text_to_speech_amd.engine import HipEngine  # noqa: E402
from text_to_speech_amd.pitch import pyin_geometry  # noqa: E402

B, FRAMES, ROUNDS = 8, 800, 9
N = FRAMES * 256


def log_mel(rng, T, n_mel=80):
    x = rng.standard_normal((T + 8, n_mel))
    x = sum(x[s:s + T] for s in range(9)) / 3.0
    return np.clip(-4.0 - 4.0 * np.arange(n_mel) / n_mel + 2.5 * x, np.log(1e-5), 2.0).astype(np.float32)


eng = HipEngine(0)
eng.load_state(weights.synth_waveglow(config.WaveGlowConfig(), seed=1234))
eng.finalize()
rng = np.random.default_rng(0)
mel = torch.from_numpy(np.stack([log_mel(rng, FRAMES) for _ in range(B)])).cuda()
z = torch.from_numpy(rng.standard_normal((B, FRAMES * 32, 8)).astype(np.float32)).cuda()
# speech-like audio to track: a gliding tone per row in noise, with a stretch of noise alone
t = np.arange(N) / 22050.0
rows = []
for b in range(B):
    f = 110.0 * (1 + 0.2 * b) * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))
    x = 0.4 * np.sin(2 * np.pi * np.cumsum(f) / 22050.0) + 0.1 * rng.standard_normal(N)
    x[N // 3:N // 3 + 20000] = 0.1 * rng.standard_normal(20000)
    rows.append(x)
audio = torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()
stream = torch.cuda.Stream()

calls = {
    'waveglow': lambda: eng.waveglow_infer(mel, z=z),
    'pitch': lambda: eng.pitch(audio, stream=stream),
    'pyin': lambda: eng.pyin(audio, stream=stream),
    'pyin_one_row': lambda: eng.pyin(audio[:1], stream=stream),
}
times = {k: [] for k in calls}
for r in range(ROUNDS + 1):
    for name, call in calls.items():
        torch.cuda.synchronize()
        on = torch.cuda.current_stream() if name == 'waveglow' else stream
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(on)
        call()
        b.record(on)
        torch.cuda.synchronize()
        if r > 0:
            times[name].append(a.elapsed_time(b))
kernels = {}
eng.kernel_timing(True)                 # from here to kernel_timing(False): pitch calls, then pyin calls, nothing else
for _ in range(ROUNDS):
    eng.pitch(audio)
kernels['pitch_kernel_us'] = round(eng.kernel_time_us(0)[0], 1)
for _ in range(ROUNDS):
    eng.pyin(audio)
kernels['pyin_obs_kernel_us'] = round(eng.kernel_time_us(2)[0], 1)
kernels['pyin_decode_kernel_us'] = round(eng.kernel_time_us(3)[0], 1)
eng.kernel_timing(False)
yin, pyin = eng.pitch(audio)[0], eng.pyin(audio)[0]
voiced = {'yin': float((yin > 0).float().mean()), 'pyin': float((pyin > 0).float().mean())}
eng.close()

med = {k: float(np.median(v)) for k, v in times.items()}
n_bins, max_step = pyin_geometry(22050, 256, 60., 500.)
frames = 1 + N // 256
print(json.dumps({'B': B, 'N': N, 'frames': frames, 'n_bins': n_bins, 'max_step': max_step, 'waveglow_ms': round(med['waveglow'], 3),
                  'pitch_ms': round(med['pitch'], 4), 'pyin_ms': round(med['pyin'], 4), 'pyin_one_row_ms': round(med['pyin_one_row'], 4),
                  **kernels, 'decode_us_per_frame': round(kernels['pyin_decode_kernel_us'] / frames, 3),
                  'decode_lds_reads': 3 * (2 * max_step + 1), 'decode_over_pitch_kernel': round(kernels['pyin_decode_kernel_us'] / kernels['pitch_kernel_us'], 2),
                  'pyin_share_of_waveglow': round(med['pyin'] / med['waveglow'], 5), 'voiced_share': {k: round(v, 3) for k, v in voiced.items()},
                  'rounds_ms': {k: [round(v, 4) for v in times[k]] for k in ('pitch', 'pyin', 'pyin_one_row')}}), flush=True)
