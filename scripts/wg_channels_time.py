"""256- and 512-channel WaveGlow side by side on the headline call (batch 8 x 800 frames), one process.

Per width and precision (f32, f16, f16x3): samples/s of the whole call (host clock around calls on device tensors that end
in a synchronise; warm-up, then the median of --runs timed calls) and, from the engine's HIP-event hooks
(tts_hip_kernel_time_us) in a separate pass, the average in-layer (layers 1 .. 7) and residual GEMM time with their share
of the MFMA peak: the fp32 peak is what tts_hip_probe_mfma_f32 measures on this device now; the fp16 MFMA peak is taken as
16 x that (the per-clock ratio of the two instructions), and f16x3 issues three fp16 MFMAs per product.  The 512-channel
fp32 call is also timed in its direct form ('f32-direct'): that is the form a 256-channel model always takes.

    python scripts/wg_channels_time.py [--batch 8] [--frames 800] [--runs 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=800)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--json')
    args = ap.parse_args()
    if args.runs < 5:
        ap.error('--runs must be at least 5')
    import torch
    from text_to_speech_amd import weights
    from text_to_speech_amd.config import WaveGlowConfig
    from text_to_speech_amd.engine import HipEngine
    B, T = args.batch, args.frames
    mel = torch.from_numpy(np.random.default_rng(7).uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)).cuda()
    z = torch.from_numpy(np.random.default_rng(11).standard_normal((B, T * 32, 8)).astype(np.float32)).cuda()
    rows = []
    for C in (512, 256):
        eng = HipEngine(0)
        eng.load_state(weights.synth_waveglow(WaveGlowConfig(n_channels=C), seed=1234))
        eng.finalize()
        assert eng.waveglow_channels == C
        peak32, ghz = eng.probe_mfma_f32()
        pos = B * T * 32                                        # GEMM rows (positions) of the call
        for label in ('f32', 'f32-direct', 'f16', 'f16x3'):
            if label == 'f32-direct' and C != 512:
                continue
            prec = 'f32' if label.startswith('f32') else label
            eng.set_waveglow_form('direct' if label == 'f32-direct' else 'winograd')
            for _ in range(args.warmup):
                out = eng.waveglow_infer(mel, z=z, precision=prec)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                out = eng.waveglow_infer(mel, z=z, precision=prec)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            assert bool(torch.isfinite(out).all())
            form, tiles = eng.last_waveglow_form, eng.last_waveglow_tiles
            eng.kernel_timing(True)                             # separate pass: the event pairs serialise the launches
            eng.waveglow_infer(mel, z=z, precision=prec)
            torch.cuda.synchronize()
            in_us, in_n = eng.kernel_time_us(0)
            res_us, res_n = eng.kernel_time_us(1)
            if form == 'winograd':                              # its layers are not the K = 3 C + 320 GEMM counted below
                in_us, in_n = 0.0, 0
            eng.kernel_timing(False)
            mfma = {'f32': 1, 'f16': 1, 'f16x3': 3}[prec]      # MFMA products issued per useful product
            peak = peak32 * (1 if prec == 'f32' else 16)
            fl_in, fl_res = 2.0 * pos * (3 * C + 320) * 2 * C, 2.0 * pos * C * C
            med = statistics.median(times)
            rows.append({
                'channels': C, 'precision': label, 'form': form, 'tiles': tiles, 'median_ms': med * 1e3,
                'min_ms': min(times) * 1e3, 'max_ms': max(times) * 1e3, 'samples_per_s': B * T * 256 / med,
                'in_layer_us': in_us, 'in_layer_launches': in_n, 'residual_us': res_us, 'residual_launches': res_n,
                'in_layer_peak_share': (fl_in * mfma / (in_us * 1e-6) / 1e12 / peak) if in_n else None,
                'residual_peak_share': (fl_res * mfma / (res_us * 1e-6) / 1e12 / peak) if res_n else None,
                'mfma_f32_tflops': peak32, 'shader_clock_ghz': ghz})
        eng.close()
    print(f'batch {B} x {T} frames, {args.runs} timed runs after {args.warmup} warm-up calls')
    print('   C  precision   form      tiles     median ms  (min .. max)      Msamples/s   in-layer us (peak share)   residual us (peak share)')
    for r in rows:
        share = lambda v: '   n/a' if v is None else f'{100 * v:5.1f}%'
        print(f"{r['channels']:4d}  {r['precision']:10s}  {r['form']:8s}  {r['tiles']:8s}  {r['median_ms']:8.2f}  "
              f"({r['min_ms']:.2f} .. {r['max_ms']:.2f})  {r['samples_per_s'] / 1e6:10.2f}   "
              f"{r['in_layer_us']:9.1f} ({share(r['in_layer_peak_share'])})        {r['residual_us']:9.1f} ({share(r['residual_peak_share'])})")
    by = {(r['channels'], r['precision']): r for r in rows}
    for p in ('f32', 'f16', 'f16x3'):
        print(f"{p}: 256 / 512 channels = {by[256, p]['samples_per_s'] / by[512, p]['samples_per_s']:.2f} x samples/s")
    print(f"f32, both in the direct form: {by[256, 'f32']['samples_per_s'] / by[512, 'f32-direct']['samples_per_s']:.2f} x")
    print(f"fp32 MFMA probe: {rows[0]['mfma_f32_tflops']:.1f} TFLOP/s at {rows[0]['shader_clock_ghz']:.2f} GHz")
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
