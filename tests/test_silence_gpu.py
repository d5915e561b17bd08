"""GPU parity: silence removal (csrc/silence.hip) against what the reference returned (tests/golden/silence_fixture.json)
and the numpy restatement; batches, device tensors, streams, the dispatcher and the facade."""
import ctypes
import hashlib
import json

import numpy as np
import pytest

import silence_ref as sr

pytestmark = pytest.mark.gpu

R = 22050
# shorter than a block; one sample; shorter than the mean-window's 3307 taps for the other methods, several scan tiles, a
# tile multiple (2048 * 10), a plain length; the mean-window method runs the rows that hold its window
LENGTHS = [1500, 1, 4410 + 300, 2048 * 10, 26460, 40001]


def _sha(y):
    return hashlib.sha256(np.ascontiguousarray(y, np.float32).tobytes()).hexdigest()


@pytest.fixture(scope='module')
def fixture():
    return json.load(open(sr.FIXTURE))['cases']


@pytest.fixture(scope='module')
def ragged():
    """Six rows at 22 050 Hz: voice and pauses cut to LENGTHS, one sample, and an all-silent row (it comes out empty in
    mode start_end); NaN beyond each row's length."""
    N = max(LENGTHS)
    base = sr.build(R, [(0.2, sr.Q), (0.3, sr.LOUD), (0.35, sr.Q), (0.12, sr.LOUD), (0.3, sr.Q), (0.4, sr.LOUD), (0.2, sr.Q)], 31)
    assert len(base) >= N
    a = np.full((len(LENGTHS), N), np.nan, np.float32)
    for b, L in enumerate(LENGTHS):
        a[b, :L] = sr.make_input('all_silent')[1][:L] if L == 26460 else base[b * 37:b * 37 + L]
    a.setflags(write=False)
    return a


def test_every_fixture_case_is_bit_equal(gpu_engine, fixture):
    for name, inp, method, kw in sr.CASES:
        rate, x = sr.make_input(inp)
        y = gpu_engine.remove_silence(x, rate, method=method, **kw)
        rec = fixture[name]
        assert y.dtype == np.float32 and y.ndim == 1
        if 'raises' in rec:                 # no silence in a slice mode: the row comes back unchanged
            assert np.array_equal(y, x), name
        else:
            assert (len(y), _sha(y)) == (rec['len'], rec['sha256']), name


BATCH = [('rms', {'mode': m, 'replace_by': 0.1}) for m in sr.RMS_MODES] + \
    [('rms', {'mode': 'remove', 'replace_by': 0.1, 'min_voice_time': 0, 'block_size': 100}),
     ('threshold', {'mode': 'start_end', 'threshold': 0.46}), ('threshold', {'mode': 'end', 'threshold': 0.3}), ('remove', {}),
     ('remove', {'min_silence': 0.05, 'threshold': 0.04})]


@pytest.mark.parametrize('method,kw', BATCH, ids=[f'{m}-{"-".join(str(v) for v in kw.values())}' for m, kw in BATCH])
def test_ragged_batch_equals_one_row_calls(gpu_engine, ragged, method, kw):
    rows = [b for b, L in enumerate(LENGTHS) if method != 'remove' or L >= int(kw.get('min_silence', 0.15) * R)]
    a, lens = np.ascontiguousarray(ragged[rows]), [LENGTHS[b] for b in rows]
    assert np.isnan(a[0, lens[0]:]).all()
    out, n = gpu_engine.remove_silence(a, R, lengths=lens, method=method, **kw)
    assert out.shape == a.shape and n.dtype == np.int32 and n.shape == (len(rows),)
    for i, L in enumerate(lens):
        assert sr.margin(method, a[i, :L], R, **kw) >= sr.MARGINS[method]        # a condition on the input, as on the CPU
        ref = sr.run(method, a[i, :L], R, **kw)
        one = gpu_engine.remove_silence(a[i, :L].copy(), R, method=method, **kw)
        assert int(n[i]) == len(one) == len(ref), (i, L)
        assert np.array_equal(out[i, :n[i]], one) and np.array_equal(one, ref), (i, L)
        assert not out[i, n[i]:].any() and not np.isnan(out[i]).any()
    if method == 'rms' and kw['mode'] == 'start_end':
        assert 0 in n and 1 in n and 1 in lens          # the all-silent row comes out empty, the one-sample row whole


def test_device_tensors_and_stream(gpu_engine, ragged):
    import torch
    a_d = torch.as_tensor(ragged.copy(), device='cuda:0')
    s = torch.cuda.Stream(device=0)
    for method, kw in (('rms', {'mode': 'remove', 'replace_by': 0.1}), ('threshold', {'threshold': 0.46}),
                       ('remove', {'min_silence': 0.05})):
        rows = slice(2, None) if method == 'remove' else slice(None)
        lens = LENGTHS[rows]
        host, n = gpu_engine.remove_silence(np.ascontiguousarray(ragged[rows]), R, lengths=lens, method=method, **kw)
        dev, n_d = gpu_engine.remove_silence(a_d[rows], R, lengths=lens, method=method, **kw)
        assert dev.is_cuda and n_d.is_cuda and n_d.dtype == torch.int32
        assert np.array_equal(dev.cpu().numpy(), host) and np.array_equal(n_d.cpu().numpy(), n)
        asy, n_a = gpu_engine.remove_silence(a_d[rows], R, lengths=lens, method=method, stream=s, **kw)
        s.synchronize()
        assert np.array_equal(asy.cpu().numpy(), host) and np.array_equal(n_a.cpu().numpy(), n)
    row, n1 = gpu_engine.remove_silence(a_d[5], R, mode='remove', replace_by=0.1)
    assert row.shape == (LENGTHS[5],) and n1.shape == ()
    assert np.array_equal(row.cpu().numpy()[:int(n1)], gpu_engine.remove_silence(ragged[5], R, mode='remove', replace_by=0.1))


def test_window_method_through_the_dispatcher(gpu_engine):
    from text_to_speech_amd.audio import load_audio, trim_silence
    f = np.load(sr.WAV.replace('audio_test_16k.wav', 'audio_processing_fixture.npz'))
    x = load_audio(sr.WAV, rate=None, engine=gpu_engine)
    y = trim_silence(x, engine=gpu_engine, rate=16000, method='window')
    assert y.dtype == np.float32 and _sha(y) == str(f['trim_silence_f32_sha256'])
    assert np.array_equal(y, load_audio(sr.WAV, rate=None, engine=gpu_engine, trim_silence=True, method='window'))
    # the reference's audio models: rms / remove / -25 dB / 0.1 s / 0.4 s on the same recording
    z = trim_silence(x, engine=gpu_engine, rate=16000, method='rms', mode='remove', threshold=-25, min_silence=0.1,
                     replace_by=0.4)
    assert len(z) == 63360


def test_infer_with_a_trim_dict(gpu_engine):
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    model = Tacotron2(HipRuntime('ts', model='tacotron2', engine=gpu_engine, seed=0))
    voc = WaveGlow(HipRuntime('ws', model='waveglow', engine=gpu_engine, seed=0))

    class Tap:                              # the vocoder, keeping the untrimmed audio of the call
        compiled_infer = voc.compiled_infer

        def __call__(self, mel, **kw):
            a = voc(mel, **kw)
            self.audio = np.array(a.detach().cpu().numpy() if hasattr(a, 'detach') else a, np.float32).reshape(-1)
            return self.audio

    tap = Tap()
    plain = model.infer('Hello there, general test.', vocoder=tap, max_length=3., seed=5)['audio']
    assert np.array_equal(plain, tap.audio)
    # a level that splits the blocks of this audio, so that something is removed
    level = 20 * np.log10(float(np.median(sr.rms_block_peaks(plain, 220))))
    trim = {'method': 'rms', 'mode': 'remove', 'threshold': level, 'min_silence': 0.02, 'replace_by': 0.01,
            'min_voice_time': 0}
    out = model.infer('Hello there, general test.', vocoder=tap, max_length=3., seed=5, trim_silence=trim)
    want = gpu_engine.remove_silence(tap.audio, R, **{k: v for k, v in trim.items() if k != 'method'})
    print(f'infer: {len(tap.audio)} samples vocoded, {len(out["audio"])} kept at {level:.1f} dB')
    assert np.array_equal(out['audio'], want) and out['time'] == len(want) / R
    assert len(want) <= len(tap.audio)


def test_refused_calls_launch_nothing(gpu_engine):
    lib, h = gpu_engine._lib, gpu_engine._h
    a = np.zeros((2, 4096), np.float32)
    out, n = np.full_like(a, 7.), np.full(2, -5, np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    ok = dict(method=0, mode=0, rate=R, threshold=-25., min_silence=0.1, block_size=220, replace_by=100, min_voice_time=0.2)

    def call(fn='tts_hip_remove_silence', audio=a, B=2, N=4096, lengths=None, o=out, last=0, **kw):
        k = {**ok, **kw}
        return getattr(lib, fn)(h, p(audio), B, N, lengths, k['method'], k['mode'], k['rate'], k['threshold'], k['min_silence'],
                                k['block_size'], k['replace_by'], k['min_voice_time'], p(o), p(n), last)

    bad_len = np.array([4097, 10], np.int32)
    bad = [dict(method=3), dict(method=-1), dict(mode=4), dict(mode=3, method=1), dict(mode=3, method=2, threshold=0.025),
           dict(rate=0), dict(block_size=0), dict(replace_by=-1), dict(threshold=float('nan')), dict(min_silence=-0.1),
           dict(min_voice_time=float('inf')), dict(method=1, threshold=-0.1), dict(method=2, threshold=0.),
           dict(method=2, threshold=0.025, min_silence=0.), dict(method=2, threshold=0.025, min_silence=0.2),
           dict(o=a), dict(o=a[1:]), dict(B=1, N=(1 << 24) + 1), dict(B=1 << 10, N=1 << 19),
           dict(B=65536, N=16),
           dict(lengths=p(bad_len)), dict(last=7)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.tts_hip_last_error(h).startswith(b'remove_silence:'), (kw, lib.tts_hip_last_error(h))
    assert call(method=2, threshold=0.025, min_silence=0.2) == -1
    msg = lib.tts_hip_last_error(h)
    assert b'L = 4096' in msg and b'w = 4410' in msg
    assert call(fn='tts_hip_remove_silence_async', rate=-1, last=None) == -1
    assert lib.tts_hip_last_error(h).startswith(b'remove_silence_async:')
    assert (out == 7.).all() and (n == -5).all()
    # the engine still works after the refused calls
    assert np.array_equal(gpu_engine.remove_silence(np.ones(5000, np.float32), 16000), np.ones(5000, np.float32))
