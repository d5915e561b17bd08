"""Timing of the silence removal (csrc/silence.hip) at batch 8 x 220 500 samples (10 s at 22 050 Hz).

  python scripts/silence_time.py [--calls 20]

Device tensors in and out (no PCIe in the figures); warm-up, synchronize, median of --calls timed calls (wall clock around
one call + synchronize; `_ms_of_100` is the mean over 100 calls back to back as a cross-check).  Prints, per method, ms per
call, the kept share of the samples and the effective GB/s: the bytes a call has to move at the least (the input read once,
the output written once, B * N * 8) over its time.  The rows are voice and pauses from the test builders
(tests/silence_ref.py), so every method removes something.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/silence_time.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

RATE, B, N = 22050, 8, 220500


def median_ms(fn, calls, sync):
    for _ in range(3):
        fn()
    sync()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    import torch
    import silence_ref as sr
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    sync = torch.cuda.synchronize
    host = np.stack([sr.build(RATE, [(0.3 + 0.05 * b, sr.Q)] + [(0.7, sr.LOUD), (0.35 + 0.02 * b, sr.Q)] * 12, 40 + b)[:N]
                     for b in range(B)])
    assert host.shape == (B, N)
    a = torch.as_tensor(host, device='cuda:0')
    res = {}
    for name, kw in (('rms', {'method': 'rms', 'mode': 'remove', 'replace_by': 0.1}),
                     ('rms_start_end', {'method': 'rms', 'mode': 'start_end'}),
                     ('threshold', {'method': 'threshold'}), ('mean_window', {'method': 'remove'})):
        ms = median_ms(lambda: eng.remove_silence(a, RATE, **kw), args.calls, sync)
        kept = eng.remove_silence(a, RATE, **kw)[1].cpu().numpy()
        res[f'{name}_ms'] = ms
        t0 = time.perf_counter()                # cross-check: 100 calls back to back, one synchronize at the end
        for _ in range(100):
            eng.remove_silence(a, RATE, **kw)
        sync()
        res[f'{name}_ms_of_100'] = (time.perf_counter() - t0) * 1e3 / 100
        res[f'{name}_kept'] = float(kept.sum()) / (B * N)
        res[f'{name}_gbps'] = B * N * 8 / (ms * 1e-3) / 1e9
    eng.close()
    print(json.dumps({k: round(v, 4) for k, v in res.items()}))


if __name__ == '__main__':
    main()
