"""Per-step time of the teacher-forced pass (HipEngine.tacotron2_forward) against the free-running decoder in 'graph' mode
(tacotron2_infer, early_stopping=False) at the same B, Tin, T (uses TTS_HIP_LIBRARY if set).

Both calls take device tensors and start from the tokens, so each is the encoder, its loop, what surrounds the loop on the GPU
(forward: bulk prenet, gate term, projection and postnet; infer: postnet) and its synchronisations.  Neither pays for a graph
capture in the timed rounds: the forward call re-encodes INTO one kept EncodedBatch (`tacotron2_encode(into=)`), as
HipRuntime does, and `tacotron2_infer` into the handle's own, so no buffer is allocated and the handle's cached chunk graphs
stay (a forward call made from tokens would encode into a fresh buffer, which empties the cache for both).  The two alternate
in one process, one warm-up round (graph capture) and three timed rounds; the figure is the median of the three wall times,
divided by T.
Prints one JSON line per shape.
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

TIN, T, ROUNDS = 128, 800, 3
precision = sys.argv[1] if len(sys.argv) > 1 else 'f32'
eng = HipEngine(0)
eng.load_state(weights.synth_tacotron2(config.Tacotron2Config(), seed=1234))
eng.finalize()
eng.set_decoder_mode('graph')
rng = np.random.default_rng(0)
for B in (8, 1):
    tok = torch.from_numpy(rng.integers(1, 148, (B, TIN)).astype(np.int32)).cuda()
    x = torch.from_numpy(rng.uniform(-8.0, 1.0, (B, T, 80)).astype(np.float32)).cuda()
    x[:, 0] = 0
    lengths = np.full((B,), T, np.int32)
    enc = eng.tacotron2_encode(tok)
    times = {'forward': [], 'graph': []}
    for r in range(ROUNDS + 1):
        for name in ('forward', 'graph'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == 'forward':
                eng.tacotron2_forward(eng.tacotron2_encode(tok, into=enc), x, lengths, precision=precision)
            else:
                eng.tacotron2_infer(tok, max_len=T, early_stopping=False, precision=precision)
            dt = time.perf_counter() - t0
            if r > 0:
                times[name].append(dt)
    enc.close()
    print(json.dumps({'B': B, 'Tin': TIN, 'T': T, 'precision': precision,
                      'forward_us_per_step': round(float(np.median(times['forward'])) / T * 1e6, 2),
                      'graph_us_per_step': round(float(np.median(times['graph'])) / T * 1e6, 2),
                      'forward_ms': [round(v * 1e3, 2) for v in times['forward']],
                      'graph_ms': [round(v * 1e3, 2) for v in times['graph']]}), flush=True)
eng.close()
