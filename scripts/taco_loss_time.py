"""Time of the TacotronLoss pass (HipEngine.tacotron2_loss) at B = 8, T = 800 -- 'mse', then the four-kind list -- beside the
teacher-forced pass whose outputs feed it (HipEngine.tacotron2_forward on a kept EncodedBatch, Tin = 128; uses TTS_HIP_LIBRARY
if set).  Everything is on the device: CUDA tensors in, a CUDA tensor out.  One process; a warm-up round (code objects, graph
capture, workspaces), then ROUNDS rounds in which the three calls alternate.  A loss call is a few microseconds of GPU work, so
each loss figure is the wall time of CALLS back-to-back calls (each ends in a stream synchronise) divided by CALLS: it includes
the launches and the synchronise, which is what a caller pays.  The figure reported is the median over the rounds.
Bytes = what the pass must read: 3 x [B, T, 80] + 2 x [B, T] floats (mel_target once more for the weighted kinds' row extrema).
The loss alone is then timed the same way at the call's frame limit, B = 8, T = 8192, on random tensors: the size at which the
pass streams long enough to show its rate.  Under `rocprofv3 --kernel-trace` the kernels' own durations come out per dispatch
(the two shapes differ in their grid sizes).
Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from text_to_speech_amd import config, weights  # noqa: E402
from text_to_speech_amd.engine import HipEngine  # noqa: E402

B, TIN, T, ROUNDS, CALLS = 8, 128, 800, 5, 200
ALL = ['mse', 'mae', 'weighted_mse', 'weighted_mae']
eng = HipEngine(0)
eng.load_state(weights.synth_tacotron2(config.Tacotron2Config(), seed=1234))
eng.finalize()
rng = np.random.default_rng(0)
tok = torch.from_numpy(rng.integers(1, 148, (B, TIN)).astype(np.int32)).cuda()
target = torch.from_numpy(rng.uniform(-8.0, 1.0, (B, T, 80)).astype(np.float32)).cuda()
x = torch.cat([torch.zeros_like(target[:, :1]), target[:, :-1]], dim=1).contiguous()
gate = torch.zeros((B, T), dtype=torch.float32, device='cuda')
gate[:, -1] = 1
lengths = np.full((B,), T, np.int32)
enc = eng.tacotron2_encode(tok)
times = {'forward': [], 'mse': [], 'all': []}
out = None
for r in range(ROUNDS + 1):
    for name in ('forward', 'mse', 'all'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == 'forward':
            out = eng.tacotron2_forward(enc, x, lengths)
            dt = time.perf_counter() - t0
        else:
            for _ in range(CALLS):
                eng.tacotron2_loss(target, gate, out.decoder_output, out.mel, out.stop_tokens, mel_loss='mse' if name == 'mse' else ALL)
            dt = (time.perf_counter() - t0) / CALLS
        if r > 0:
            times[name].append(dt)
enc.close()
TL, CALLS_L = 8192, 50
big = [torch.from_numpy(rng.uniform(-8.0, 1.0, (B, TL, 80)).astype(np.float32)).cuda() for _ in range(3)]
gate_l = torch.zeros((B, TL), dtype=torch.float32, device='cuda')
gate_l[:, -1] = 1
stop_l = torch.full((B, TL), 0.3, dtype=torch.float32, device='cuda')
times.update(limit_mse=[], limit_all=[])
for r in range(ROUNDS + 1):
    for name in ('limit_mse', 'limit_all'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS_L):
            eng.tacotron2_loss(big[0], gate_l, big[1], big[2], stop_l, mel_loss='mse' if name == 'limit_mse' else ALL)
        if r > 0:
            times[name].append((time.perf_counter() - t0) / CALLS_L)
eng.close()
med = {k: float(np.median(v)) for k, v in times.items()}
bytes_l = (3 * B * TL * 80 + 2 * B * TL) * 4
bytes_mse = (3 * B * T * 80 + 2 * B * T) * 4
bytes_all = bytes_mse + B * T * 80 * 4
print(json.dumps({'B': B, 'T': T, 'Tin': TIN, 'forward_ms': round(med['forward'] * 1e3, 3),
                  'loss_mse_us': round(med['mse'] * 1e6, 2), 'loss_all_us': round(med['all'] * 1e6, 2),
                  'bytes_mse': bytes_mse, 'bytes_all': bytes_all,
                  'gbps_mse': round(bytes_mse / med['mse'] / 1e9, 1), 'gbps_all': round(bytes_all / med['all'] / 1e9, 1),
                  'loss_share_of_forward_mse': round(med['mse'] / med['forward'], 6),
                  'loss_share_of_forward_all': round(med['all'] / med['forward'], 6),
                  'limit_T': TL, 'limit_bytes_mse': bytes_l, 'limit_mse_us': round(med['limit_mse'] * 1e6, 2),
                  'limit_all_us': round(med['limit_all'] * 1e6, 2), 'limit_gbps_mse': round(bytes_l / med['limit_mse'] / 1e9, 1),
                  'limit_gbps_all': round((bytes_l + B * TL * 80 * 4) / med['limit_all'] / 1e9, 1),
                  'rounds_us': {k: [round(v * 1e6, 2) for v in times[k]] for k in ('mse', 'all')}}), flush=True)
