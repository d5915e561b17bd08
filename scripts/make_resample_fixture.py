"""Copy the reference's resampling and mel goldens into a small committed fixture.

Run where the reference checkout exists:  python scripts/make_resample_fixture.py <reference root>
Inputs (data files held by the reference's own tests, tests/test_utils_audio.py:60-110):
  tests/data/audio_test.wav                        16 kHz int16, 64 880 samples (committed as tests/golden/audio_test_16k.wav)
  tests/__reproduction/audio_resample.npy          float32 (89412,) = load_audio(wav, rate=22050)
  tests/__reproduction/stft-TacotronSTFT.npy       float32 (350, 80) = load_mel(wav, TacotronSTFT())
Output:
  tests/golden/resample_fixture.npz                the whole mel golden, every 8th sample of the resampled golden and its
                                                   length, and the sha256 of both source files and of the resampled
                                                   golden's float32 bytes (scipy in float64 rebuilds it bitwise from the
                                                   wav, so a test checks the full copy against that hash)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 2:
    sys.exit('usage: python scripts/make_resample_fixture.py <reference root>')
REF = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import audio_ref  # noqa: E402
import resample_ref  # noqa: E402


def sha(p):
    return hashlib.sha256(open(p, 'rb').read()).hexdigest()


wav = os.path.join(ROOT, 'tests', 'golden', 'audio_test_16k.wav')
assert sha(wav) == sha(os.path.join(REF, 'tests', 'data', 'audio_test.wav'))
rs_p = os.path.join(REF, 'tests', '__reproduction', 'audio_resample.npy')
mel_p = os.path.join(REF, 'tests', '__reproduction', 'stft-TacotronSTFT.npy')
rs, mel = np.load(rs_p), np.load(mel_p)
assert rs.dtype == np.float32 and rs.shape == (89412,) and mel.dtype == np.float32 and mel.shape == (350, 80)

rate, raw = audio_ref.read_wav(wav)
rebuilt = audio_ref.normalize_audio(resample_ref.resample(raw, resample_ref.resampled_length(raw.size, rate, 22050)))
assert np.array_equal(rebuilt, rs), 'scipy in float64 does not rebuild the resampled golden'

out = os.path.join(ROOT, 'tests', 'golden', 'resample_fixture.npz')
np.savez_compressed(out, mel=mel, resample_every8=rs[::8].copy(), resample_len=np.int64(rs.size),
                    resample_sha256=sha(rs_p), mel_sha256=sha(mel_p),
                    resample_f32_sha256=hashlib.sha256(rs.tobytes()).hexdigest())
print('wrote', out, os.path.getsize(out), 'bytes')
