"""Which kernels each kind of WaveGlow call launches, in order: one call of each kind -- plain, seeded, ragged, packed, rows-seeded
ragged, rows-seeded packed; each on the engine's stream and on a caller's -- at B = 3, T = 6, lengths (6, 0, 3), fp32, device
tensors.  A mel-STFT call stands between two of them as a marker (its kernels occur in no WaveGlow call), and the list runs
twice: the first pass takes the one-time work.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o wg -- python3 scripts/wg_call_launches.py [--root TREE]
  python3 scripts/wg_call_launches.py --summarize DIR

--root: the tree whose `text_to_speech_amd` is imported (default: this one), e.g. a checkout of the parent commit.  --summarize
reads the kernel trace under DIR and prints one line per call of the second pass, `kind: kernel xN | kernel ...`; two trees
launch the same when `diff` finds the two outputs equal."""
import argparse, csv, glob, itertools, os, sys

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--summarize', metavar='DIR')
args = ap.parse_args()

LENGTHS = (6, 0, 3)
ROWS = ([11, 12, 13], [0, 5, 9])
KINDS = {'plain': dict(z=True), 'seeded': dict(seed=5), 'ragged': dict(z=True, lengths=LENGTHS),
         'packed': dict(z=True, lengths=LENGTHS, packed=True), 'rows-seeded ragged': dict(row_seeds=ROWS, lengths=LENGTHS),
         'rows-seeded packed': dict(row_seeds=ROWS, lengths=LENGTHS, packed=True)}
LABELS = [f'{kind} {how}' for kind in KINDS for how in ('sync', 'async')]

if args.summarize:
    rows = []
    for path in glob.glob(os.path.join(args.summarize, '**', '*kernel_trace.csv'), recursive=True):
        with open(path, newline='') as f:
            rows += [(int(r['Start_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(f)]
    names = [n for _, n in sorted(rows)]
    # a marker runs from its reflect_pad_kernel to its log_clamp_kernel; a call is what lies between two markers
    calls, cur, in_marker = [], None, False
    for n in names:
        if n.startswith('reflect_pad_kernel'):
            if cur is not None:
                calls.append(cur)
            in_marker = True
        elif in_marker and n.startswith('log_clamp_kernel'):
            in_marker, cur = False, []
        elif not in_marker and cur is not None:
            cur.append(n)
    assert len(calls) == 2 * len(LABELS), f'{len(calls)} calls between markers, expected {2 * len(LABELS)}'
    for label, call in zip(LABELS, calls[len(LABELS):]):
        print(f'{label}: ' + ' | '.join(f'{n} x{len(list(g))}' for n, g in itertools.groupby(call)))
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch
from text_to_speech_amd import weights
from text_to_speech_amd.config import WaveGlowConfig
from text_to_speech_amd.engine import HipEngine

eng = HipEngine(0)
eng.load_state(weights.synth_waveglow(WaveGlowConfig(), seed=1234))
eng.finalize()
rng = np.random.default_rng(3)
mel = torch.from_numpy(rng.uniform(-11.5, 1.2, (3, 6, 80)).astype(np.float32)).cuda()
z = torch.from_numpy(rng.standard_normal((3, 6 * 32, 8)).astype(np.float32)).cuda()
wav = torch.zeros((1, 1024), device='cuda')
stream = torch.cuda.Stream()
torch.cuda.synchronize()
for _ in range(2):
    for kw in KINDS.values():
        kw = dict(kw, z=z) if kw.get('z') else kw
        for st in (None, stream):
            eng.mel_stft(wav)
            eng.waveglow_infer(mel, stream=st, **kw)
            torch.cuda.synchronize()
eng.mel_stft(wav)
eng.close()
