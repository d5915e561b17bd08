"""Timing of FFT resampling (csrc/resample.hip) on three shapes, with scipy's host time beside it as context only.

  python scripts/resample_time.py [--calls 20]

Shapes: one 64 880-sample file 16 -> 22.05 kHz; 8 x 10 s at 44.1 -> 22.05 kHz; one 60 s file at 48 -> 22.05 kHz.  Device
tensors in and out (no PCIe in the figures).  Each shape is warmed up, then timed with device events around each call on
torch's current stream; the median of --calls calls is printed in ms, with the Bluestein lengths and an estimate of the
bytes the FFT passes move.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/resample_time.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [('one 64880-sample file 16->22.05 kHz', 1, 64880, 16000, 22050),
          ('8 x 10 s 44.1->22.05 kHz', 8, 441000, 44100, 22050),
          ('one 60 s file 48->22.05 kHz', 1, 2880000, 48000, 22050)]


def lengths(n, m):
    lf = max(64, 1 << int(np.ceil(np.log2(n + n // 2))))
    li = max(64, 1 << int(np.ceil(np.log2(2 * m - 1))))
    return lf, li


def pass_bytes(L, lines_fwd, lines_inv):
    # one pass in LDS reads and writes each line once; the four-step form reads and writes it twice
    per = 16 if L <= 8192 else 32
    return per * L * (lines_fwd + lines_inv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    import torch
    from scipy import signal
    from text_to_speech_amd.audio import resampled_length
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    rng = np.random.default_rng(0)
    res = []
    for name, B, N, r, t in SHAPES:
        host = rng.standard_normal((B, N)).astype(np.float32)
        a = torch.as_tensor(host, device='cuda:0')
        M = resampled_length(N, r, t)
        for _ in range(3):
            eng.resample(a, r, t)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.resample(a, r, t)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        gpu_ms = float(np.median(ts))
        t0 = time.perf_counter()
        signal.resample(host[0].astype(np.float64), M)
        scipy_ms = (time.perf_counter() - t0) * 1e3 * B
        lf, li = lengths(N, M)
        traffic = B * (pass_bytes(lf, 2, 1) + pass_bytes(li, 2, 1)) + B * (N + M) * 4
        row = dict(shape=name, B=B, N=N, M=M, L_fwd=lf, L_inv=li, gpu_ms=round(gpu_ms, 4),
                   est_MB=round(traffic / 1e6, 1), est_GBps=round(traffic / gpu_ms / 1e6, 1),
                   scipy_host_ms=round(scipy_ms, 2))
        res.append(row)
        print(json.dumps(row), flush=True)
    eng.close()


if __name__ == '__main__':
    main()
