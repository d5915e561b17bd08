"""Time of the pitch call (HipEngine.pitch) at the defaults on 8 x 204 800 device-resident samples (the benchmark's audio shape) and
on one row, beside the vocoder step that produces such audio (HipEngine.waveglow_infer: 8 rows of 800 frames, synthetic weights),
the mel analysis of the same audio (HipEngine.mel_stft) and the F0 comparison (HipEngine.f0_error) of two 8 x 801-frame tracks
along the 800 x 800-frame warping paths of a mel_dtw call.  Uses TTS_HIP_LIBRARY if set.  Everything is on the device.

One process; a warm-up round, then ROUNDS rounds in which the calls alternate.  A figure is the time between two events on the
caller's stream around one call, median over the rounds; `pitch_kernel_us` is the kernel alone from the engine's event timing
(tts_hip_kernel_timing: a pitch call files its launch under kind 0, an f0_error call under kind 1).  Other calls file
launches under the same kinds (the vocoder, mel_dtw, the STFT family): the two figures are these kernels' only because no
other call runs while timing is on -- keep it so when changing this script.

`lds_bound_us`: what the kernel's own LDS reads cost at the array's 256 bytes a clock and CU -- per frame, every wave of the
workgroup issues two 16-byte reads (1 KiB a wave each) per four samples of the window -- and `lds_share` = that over the kernel
time.  Prints one JSON line.
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

B, FRAMES, ROUNDS = 8, 800, 9
N = FRAMES * 256
WIN, TAU_MAX = 1024, 367
CUS, CLOCK_GHZ, LDS_BYTES_PER_CLK = 256, 2.4, 256


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
# speech-like audio to track: a gliding tone per row with an unvoiced stretch (the vocoder's output on synthetic weights is noise)
t = np.arange(N) / 22050.0
rows = []
for b in range(B):
    f = 110.0 * (1 + 0.2 * b) * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))
    x = 0.4 * np.sin(2 * np.pi * np.cumsum(f) / 22050.0)
    x[N // 3:N // 3 + 20000] = 0.05 * rng.standard_normal(20000)
    rows.append(x)
audio = torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()
stream = torch.cuda.Stream()
_, path = eng.mel_dtw(mel, torch.roll(mel, 3, 1), return_path=True)
tracks = eng.pitch(audio)
f0_a, f0_b = tracks[0], torch.roll(tracks[0], 5, 1) * 1.01

calls = {
    'waveglow': lambda: eng.waveglow_infer(mel, z=z),
    'pitch': lambda: eng.pitch(audio, stream=stream),
    'pitch_one_row': lambda: eng.pitch(audio[:1], stream=stream),
    'mel_stft': lambda: eng.mel_stft(audio),
    'f0_error': lambda: eng.f0_error(f0_a[:, :FRAMES], f0_b[:, :FRAMES], path=path, stream=stream),
}
times = {k: [] for k in calls}
for r in range(ROUNDS + 1):
    for name, call in calls.items():
        torch.cuda.synchronize()
        on = stream if name in ('pitch', 'pitch_one_row', 'f0_error') else torch.cuda.current_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(on)
        call()
        b.record(on)
        torch.cuda.synchronize()
        if r > 0:
            times[name].append(a.elapsed_time(b))
kernels = {}
eng.kernel_timing(True)                 # from here to kernel_timing(False): pitch calls, then f0_error calls, nothing else
for _ in range(ROUNDS):
    eng.pitch(audio)
kernels['pitch_kernel_us'] = round(eng.kernel_time_us(0)[0], 1)
for _ in range(ROUNDS):
    eng.f0_error(f0_a[:, :FRAMES], f0_b[:, :FRAMES], path=path)
kernels['f0_error_kernel_us'] = round(eng.kernel_time_us(1)[0], 1)
eng.kernel_timing(False)
stats = eng.f0_error(f0_a[:, :FRAMES], f0_b[:, :FRAMES], path=path).cpu().numpy()
voiced = float((tracks[0] > 0).float().mean())
eng.close()

med = {k: float(np.median(v)) for k, v in times.items()}
frames = B * (1 + N // 256)
waves = -(-(-(-(TAU_MAX + 1) // 4)) // 64)
lds_bytes = frames * waves * (WIN // 4) * 2 * 1024
lds_bound_us = lds_bytes / (CUS * LDS_BYTES_PER_CLK * CLOCK_GHZ * 1e3)
print(json.dumps({'B': B, 'N': N, 'frames': frames, 'lags': TAU_MAX + 1, 'waveglow_ms': round(med['waveglow'], 3),
                  'pitch_ms': round(med['pitch'], 4), 'pitch_one_row_ms': round(med['pitch_one_row'], 4),
                  'mel_stft_ms': round(med['mel_stft'], 4), 'f0_error_ms': round(med['f0_error'], 4), **kernels,
                  'pitch_share_of_waveglow': round(med['pitch'] / med['waveglow'], 5),
                  'lds_bytes': lds_bytes, 'lds_bound_us': round(lds_bound_us, 1),
                  'lds_share': round(lds_bound_us / kernels['pitch_kernel_us'], 4),
                  'gflop': round(frames * WIN * (TAU_MAX + 1) * 3 / 1e9, 2), 'voiced_share': round(voiced, 3),
                  'mean_pairs': float(stats[0].mean()), 'mean_rmse_cents': round(float(stats[2].mean()), 2),
                  'rounds_ms': {k: [round(v, 4) for v in times[k]] for k in ('pitch', 'pitch_one_row', 'f0_error')}}), flush=True)
