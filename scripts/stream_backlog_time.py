"""Timing: `predict()` over a backlog of sentences -- sequential (every sentence alone at batch 1) against `batch_backlog=8`
(waiting sentences decoded as one token batch on the fused step and vocoded in one ragged WaveGlow call) and against the same
with `pack_vocoder=True` (that one vocoder call computed as one packed row; mode `packed`, with `--mode all`).  The workload of
bench.py's config 5: 64 sentences, token counts cycling 50 .. 200, fp16 modes of both models, max_length=4., deterministic.
Reports x real time (audio seconds per wall second) and the time to the first sentence's audio for each mode; the modes
alternate, each run ends with its last callback (host arrays: every device call has finished).

  python scripts/stream_backlog_time.py [--root DIR] [--mode both|all|sequential|backlog|packed] [--k 8] [--reps 3]

--root: the tree whose `text_to_speech_amd` is imported (default: this one) -- `--root <checkout of an older commit> --mode
sequential` times that commit's stream for comparison.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--mode', default='both', choices=('both', 'all', 'sequential', 'backlog', 'packed'))
ap.add_argument('--k', type=int, default=8)
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from text_to_speech_amd import weights
from text_to_speech_amd.config import Tacotron2Config, WaveGlowConfig
from text_to_speech_amd.engine import HipEngine
from text_to_speech_amd.runtime import HipRuntime
from text_to_speech_amd.tacotron2 import Tacotron2
from text_to_speech_amd.waveglow import WaveGlow

eng = HipEngine(0)
eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=1234))
eng.load_state(weights.synth_tacotron2(Tacotron2Config(), seed=1234))
eng.finalize()
model = Tacotron2(HipRuntime('t', model='tacotron2', engine=eng, seed=0, synthesizer_precision='f16'))
voc = WaveGlow(HipRuntime('w', model='waveglow', engine=eng, seed=0, vocoder_precision='f16'))
rng = np.random.default_rng(0)
letters = np.array(list('abcdefghijklmnopqrstuvwxyz     '))
lens = [50, 70, 90, 110, 130, 150, 170, 200]
texts = [''.join(rng.choice(letters, lens[i % 8])).strip() + f' {i}.' for i in range(64)]
kw = dict(vocoder=voc, max_length=4., deterministic=True, save=False, return_results=False)
extra = {'sequential': {}, 'backlog': {'batch_backlog': args.k}, 'packed': {'batch_backlog': args.k, 'pack_vocoder': True}}
modes = {'both': ('sequential', 'backlog'), 'all': ('sequential', 'backlog', 'packed')}.get(args.mode, (args.mode,))


def run(mode, items):
    secs, first = [], []
    t0 = time.perf_counter()

    def cb(**entry):
        if not secs:
            first.append(time.perf_counter() - t0)
        secs.append(entry['time'])

    model.predict(items, callbacks=[cb], **kw, **extra[mode])
    dt = time.perf_counter() - t0
    return dt, sum(secs), first[0], eng.last_decoder_mode


for m in modes:                                          # warm every shape of the timed runs
    run(m, texts)
res = {m: [] for m in modes}
for _ in range(args.reps):
    for m in modes:
        res[m].append(run(m, texts))
out = {'root': os.path.abspath(args.root), 'sentences': len(texts), 'k': args.k}
for m in modes:
    dts = [r[0] for r in res[m]]
    out[f'{m}_ms_median'] = float(np.median(dts)) * 1e3
    out[f'{m}_ms_min_max'] = [min(dts) * 1e3, max(dts) * 1e3]
    out[f'{m}_x_realtime'] = res[m][0][1] / float(np.median(dts))
    out[f'{m}_first_audio_ms_median'] = float(np.median([r[2] for r in res[m]])) * 1e3
    out[f'{m}_decoder_path'] = res[m][-1][3]
out['audio_seconds'] = res[modes[0]][0][1]
if 'sequential' in modes and 'backlog' in modes:
    out['backlog_over_sequential'] = out['backlog_x_realtime'] / out['sequential_x_realtime']
if 'packed' in modes and 'backlog' in modes:
    out['packed_over_backlog'] = out['packed_x_realtime'] / out['backlog_x_realtime']
eng.close()
print(json.dumps(out))
