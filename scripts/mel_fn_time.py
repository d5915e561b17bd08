"""Timing of the mel plans (csrc/mel_stft.hip): the default plan against the fixed call `mel_stft` at 8 x 204 800 samples
(bench.py's mel-STFT shape), and the Whisper plan at 8 x 30 s of 16 kHz audio (8 x 480 000 samples), whole rows and a ragged
batch.

  python scripts/mel_fn_time.py [--calls 20]

Device tensors in and out (no PCIe in the figures); warm-up, synchronize, median of --calls timed calls (wall clock around
one call + synchronize; `_ms_of_100` is the mean over 100 calls back to back as a cross-check).  Prints ms per call and the
multiple of real time (seconds of audio per second of computing).
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/mel_fn_time.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    from text_to_speech_amd.engine import HipEngine
    from text_to_speech_amd.stft import TacotronSTFT, WhisperSTFT
    eng = HipEngine(0)
    eng.finalize()                                  # no weights: only the fixed mel-STFT becomes ready
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    taco, whisper = TacotronSTFT(engine=eng), WhisperSTFT(engine=eng)
    a22 = torch.as_tensor(rng.uniform(-1, 1, (8, 204800)).astype(np.float32), device='cuda:0')
    a16 = torch.as_tensor(rng.uniform(-1, 1, (8, 480000)).astype(np.float32), device='cuda:0')
    lens = [480000 - 37000 * b for b in range(8)]
    runs = (('mel_stft', lambda: eng.mel_stft(a22), 8 * 204800 / 22050),
            ('default_plan', lambda: taco(a22), 8 * 204800 / 22050),
            ('whisper_8x30s', lambda: whisper(a16), 8 * 30.0),
            ('whisper_ragged', lambda: whisper(a16, lengths=lens), sum(lens) / 16000))
    res = {}
    for name, fn, seconds in runs:
        ms = median_ms(fn, args.calls, sync)
        res[f'{name}_ms'] = ms
        t0 = time.perf_counter()                    # cross-check: 100 calls back to back, one synchronize at the end
        for _ in range(100):
            fn()
        sync()
        res[f'{name}_ms_of_100'] = (time.perf_counter() - t0) * 1e3 / 100
        res[f'{name}_x_real_time'] = seconds / (ms * 1e-3)
    assert torch.equal(eng.mel_stft(a22), taco(a22))
    eng.close()
    print(json.dumps({k: round(v, 4) for k, v in res.items()}))


if __name__ == '__main__':
    main()
