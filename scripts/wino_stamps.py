"""Phase of the two co-resident blocks of a CU in wino4_fused2_kernel, from in-kernel clock stamps.

Needs the measurement build:  TTS_BUILD_TAG=stamps csrc/build.sh -DTTS_WINO_STAMPS, loaded through
TTS_HIP_LIBRARY=text_to_speech_amd/libtts_hip_stamps.so.  Runs one 8 x 800 call and reads the stamps of its last launch:
per block {entry, end of the K loop, end} on the shader clock plus HW_ID / XCC_ID.  Usage: python scripts/wino_stamps.py [out.json]
"""
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    from text_to_speech_amd import _lib, weights
    from text_to_speech_amd.config import WaveGlowConfig
    from text_to_speech_amd.engine import HipEngine
    lib = _lib.load_library()
    eng = HipEngine(0)
    eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=1234))
    eng.finalize()
    mel = np.random.default_rng(0).uniform(-11.5, 1.2, (8, 800, 80)).astype(np.float32)
    eng.waveglow_infer(mel, seed=1)
    eng.waveglow_infer(mel, seed=1)
    n = 6400
    buf = np.zeros((n, 4), np.uint64)
    lib.tts_hip_debug_wino_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.tts_hip_debug_wino_stamps(buf.ctypes.data_as(ctypes.c_void_p), n) == 0
    t0, t1, t2 = (buf[:, i].astype(np.int64) for i in range(3))
    hw = buf[:, 3]
    hwid, xcc = (hw & np.uint64(0xffffffff)).astype(np.int64), (hw >> np.uint64(32)).astype(np.int64) & 0xf
    cu = ((xcc << 8) | (((hwid >> 13) & 7) << 5) | (((hwid >> 12) & 1) << 4) | ((hwid >> 8) & 0xf))      # XCC | SE | SH | CU
    tile = float(np.median(t2 - t0))
    res = {'blocks': n, 'cus': int(len(np.unique(cu))),
           'tile_clocks_median': tile, 'epilogue_over_tile_median': float(np.median((t2 - t1) / (t2 - t0))),
           'kloop_clocks_median': float(np.median(t1 - t0)), 'epilogue_clocks_median': float(np.median(t2 - t1))}
    # blocks of the first round, by CU: which block indices are the second of their CU
    first = np.arange(n) < 512
    second = []
    for c in np.unique(cu):
        ids = np.flatnonzero((cu == c) & first)
        second += list(ids[np.argsort(t0[ids])][1:])
    res['first_round_second_blocks_min_max'] = [int(min(second)), int(max(second))] if second else None
    res['first_round_second_blocks_in_256_511'] = float(np.mean([256 <= b < 512 for b in second])) if second else None
    # phase: on every CU, the K-loop ends in time order; distance of each to the nearest K-loop end of ANOTHER block of that CU,
    # as a fraction of a tile (0 = the two resident blocks reach their epilogues together, 0.5 = half a tile apart)
    for name, lo, hi in (('all', 0.0, 1.0), ('first_third', 0.0, 1 / 3), ('last_third', 2 / 3, 1.0)):
        fr = []
        for c in np.unique(cu):
            ids = np.flatnonzero(cu == c)
            ke = np.sort(t1[ids])
            span = ke[-1] - ke[0]
            sel = ke[(ke >= ke[0] + lo * span) & (ke <= ke[0] + hi * span)]
            if len(sel) < 3:
                continue
            d = np.diff(sel)
            near = np.minimum(np.r_[d, d[-1]], np.r_[d[0], d])
            fr += list(near / tile)
        fr = np.asarray(fr)
        res[f'phase_{name}'] = {'median': float(np.median(fr)), 'p10': float(np.percentile(fr, 10)), 'p90': float(np.percentile(fr, 90)),
                                'hist_0_to_0.6_by_0.1': [int(x) for x in np.histogram(fr, bins=np.arange(0, 0.7001, 0.1))[0]]}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(line + '\n')
        np.save(os.path.splitext(sys.argv[1])[0] + '_raw.npy', buf)        # the stamps themselves, for another look
    eng.close()


if __name__ == '__main__':
    main()
