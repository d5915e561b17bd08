"""Copy the reference's waveform clean-up goldens into a small committed fixture.

Run where the reference checkout exists:  python scripts/make_audio_fixture.py <reference root>
Inputs (data files held by the reference's own tests, tests/test_utils_audio.py:60-82):
  tests/data/audio_test.wav                        16 kHz int16, 64 880 samples
  tests/__reproduction/audio_reduce_noise.npy      float32 (64880,) = load_audio(wav, rate=None, reduce_noise=True)
  tests/__reproduction/audio_trim_silence.npy      float32 (55675,) = load_audio(wav, rate=None, trim_silence=True,
                                                                                 method='window')
Outputs:
  tests/golden/audio_test_16k.wav                  the input wav, byte for byte
  tests/golden/audio_processing_fixture.npz        the reduce_noise golden, the trim indices (the trim golden is the slice
                                                   [start, end) of the normalized input) and the sha256 of the three files
                                                   and of the trim golden's float32 bytes (so the slice is checked bitwise
                                                   without a second copy of the signal)
"""
import hashlib
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 2:
    sys.exit('usage: python scripts/make_audio_fixture.py <reference root>')
REF = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import audio_ref  # noqa: E402


def sha(p):
    return hashlib.sha256(open(p, 'rb').read()).hexdigest()


wav = os.path.join(REF, 'tests', 'data', 'audio_test.wav')
rn_p = os.path.join(REF, 'tests', '__reproduction', 'audio_reduce_noise.npy')
tr_p = os.path.join(REF, 'tests', '__reproduction', 'audio_trim_silence.npy')
rn, tr = np.load(rn_p), np.load(tr_p)
assert rn.dtype == np.float32 and rn.shape == (64880,) and tr.dtype == np.float32, (rn.shape, tr.shape)

rate, raw = audio_ref.read_wav(wav)
x = audio_ref.normalize_audio(raw)
start, end = audio_ref.trim_window(x, rate)
assert np.array_equal(x[start:end], tr), 'the trim golden is not a slice of the normalized input'

golden = os.path.join(ROOT, 'tests', 'golden')
shutil.copyfile(wav, os.path.join(golden, 'audio_test_16k.wav'))
out = os.path.join(golden, 'audio_processing_fixture.npz')
np.savez_compressed(out, reduce_noise=rn, trim_start=np.int64(start), trim_end=np.int64(end),
                    wav_sha256=sha(wav), reduce_noise_sha256=sha(rn_p), trim_silence_sha256=sha(tr_p),
                    trim_silence_f32_sha256=hashlib.sha256(tr.tobytes()).hexdigest())
print('wrote', out, os.path.getsize(out), 'bytes; trim', start, end)
