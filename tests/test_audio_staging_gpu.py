"""GPU: the one staging buffer every synchronous audio call of a handle shares (tts_hip_engine::audio_io, AudioStage in
csrc/engine.h).  A sequence of host-array calls of different sizes on one engine -- so that the buffer is carved differently
from call to call and grows after others have used it -- must give, call for call, the bytes a fresh engine gives."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 22050


def _fresh():
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.finalize()                      # no weights: the mel-STFT bases only
    return eng


def _rows(rng, B, N, quiet=()):
    """B rows of N samples of noise, the spans in `quiet` (start, stop) 40 dB down: something to gate, trim and remove."""
    x = (0.5 * rng.standard_normal((B, N))).astype(np.float32)
    for a, z in quiet:
        x[:, a:z] *= 0.01
    return x


# the smallest shapes that hit a tail tile (3 x 2048 -> 9 frames, 2 x 4100 -> three scan tiles of 2048), a one-sample row and a
# row shorter than the trim window
def _calls():
    rng = np.random.default_rng(5)
    mel_small, mel_big = _rows(rng, 1, 1024), _rows(rng, 3, 2048)
    rs, rn, trim = _rows(rng, 2, 300), _rows(rng, 2, 3000, [(0, 600)]), _rows(rng, 1, 100, [(0, 30)])
    sil = _rows(rng, 2, 4100, [(0, 1000), (2000, 3200)])
    calls = [('mel_stft 1 x 1024', lambda e: e.mel_stft(mel_small)),
             ('resample 2 x 300', lambda e: e.resample(rs, 16000, 22050)),
             ('reduce_noise 2 x 3000, lengths [3000, 1]', lambda e: e.reduce_noise(rn, lengths=[3000, 1], noise_length=500)),
             ('trim_silence 1 x 100, window 200', lambda e: e.trim_silence(trim, window_length=200, threshold=0.01))]
    for method, kw in (('rms', {}), ('threshold', {}), ('remove', {'min_silence': 0.05})):
        calls.append((f'remove_silence 2 x 4100, {method}', lambda e, m=method, k=kw: e.remove_silence(sil, R, method=m, **k)))
    calls += [('mel_stft 3 x 2048', lambda e: e.mel_stft(mel_big)),
              ('mel_stft 1 x 1024 again', lambda e: e.mel_stft(mel_small)),
              ('reduce_noise_probe', lambda e: e.reduce_noise_probe(rn, lengths=[3000, 1], noise_length=500, what='gated')),
              ('mel_stft_probe', lambda e: e.mel_stft_probe(mel_big, what='mel_linear'))]
    return calls


def _bytes(result):
    parts = result if isinstance(result, tuple) else (result,)
    return [np.ascontiguousarray(p).tobytes() for p in parts]


def test_calls_that_share_the_staging_buffer_equal_a_fresh_engine():
    calls = _calls()
    used = _fresh()
    try:
        got = [_bytes(fn(used)) for _, fn in calls]
    finally:
        used.close()
    assert got[0] == got[8] and got[0] != got[7]            # the repeated call, and that the sequence is not trivially constant
    for (name, fn), mine in zip(calls, got):
        fresh = _fresh()
        try:
            want = _bytes(fn(fresh))
        finally:
            fresh.close()
        assert len(mine) == len(want) and all(len(m) for m in mine), name
        assert mine == want, name
