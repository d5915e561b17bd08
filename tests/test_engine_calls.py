"""CPU: every library call `HipEngine` makes for host arrays, symbol by symbol and argument by argument, against a recording.

The engine is built without a handle of its own (`HipEngine.__new__`) on a stand-in for the C library that records
(symbol, normalized arguments) and returns 0.  tests/golden/engine_calls.json holds what each case below recorded when the fixture
was made (`python tests/test_engine_calls.py` rewrites it); the test asserts that the same calls, in the same order, with the same
arguments are made now -- so a binding change that adds or drops a `synchronize`, a `random_fill` or a width query, converts an
input differently or passes another mem kind shows up here without a GPU.

How an argument is recorded: ints, floats and None as they are; a ctypes scalar by its value; a pointer to an array (found
through a registry filled by wrapping `HipEngine._ptr`, or through the array numpy hangs on the pointer it makes) as dtype and
shape, plus a short hash of the bytes where the header declares the parameter `const` (an input); the opaque handles the stand-in
gave out by name; `byref` of a scalar as the scalar's type (an output), of a struct as a hash of its bytes.

Not here, because they need a CUDA tensor even for host input: `random_normal`, `random_prenet_masks`, `random_*_rows`,
`waveglow_infer(seed=, lengths=)` and `tacotron2_forward(seed=)`; tests/test_engine_calls_gpu.py runs those.
"""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'engine_calls.json')

ENGINE, PLAN, ENCODED = 0x7700, 0x1000, 0x2000
HANDLES = {ENGINE: 'engine', PLAN: 'plan', ENCODED: 'encoded'}
FRAMES, SAMPLES, CHANNELS, WIDTH = 12, 2816, 512, 37          # the stand-in's fixed answers


def _outputs():
    """symbol -> per parameter, True where the header declares a pointer that is not `const` (something the call writes)."""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tts_hip.h')).read(), flags=re.S)
    table = {}
    for name, params in re.findall(r'\b(tts_hip_\w+)\s*\(([^)]*)\)\s*;', src):
        table[name] = ['*' in p and not p.strip().startswith('const') for p in params.split(',')]
    return table


OUTPUTS = _outputs()


class Recorder:
    """Stands for the C library: every tts_hip_* attribute records its call and returns 0 (or the fixed answer above)."""

    def __init__(self):
        self.calls, self.arrays = [], {}

    def __getattr__(self, name):
        if not name.startswith('tts_hip_'):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def register(self, pointer, array):
        if pointer is not None:
            self.arrays[pointer.value] = array             # kept alive: its address is not handed out again

    def _call(self, name, args):
        assert len(args) == len(OUTPUTS[name]), f'{name}: {len(args)} arguments, the header declares {len(OUTPUTS[name])}'
        self.calls.append([name[len('tts_hip_'):], [self._norm(a, out) for a, out in zip(args, OUTPUTS[name])]])
        if name == 'tts_hip_last_error':
            return b''
        if name == 'tts_hip_mel_fn_create':
            args[3]._obj.value = PLAN
        if name == 'tts_hip_tacotron2_encode':
            args[-1]._obj.value = ENCODED
        if name == 'tts_hip_remove_silence_probe':
            args[-2]._obj.value = WIDTH
        return {'tts_hip_mel_fn_frames': FRAMES, 'tts_hip_mel_fn_samples': SAMPLES, 'tts_hip_waveglow_channels': CHANNELS}.get(name, 0)

    def _norm(self, a, is_output):
        if a is None or isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, np.integer):
            return int(a)
        if isinstance(a, np.floating):
            return float(a)
        if isinstance(a, bytes):
            return a.decode()
        if isinstance(a, ctypes.Array):
            return list(a)
        if type(a).__name__ == 'CArgObject':               # ctypes.byref
            obj = a._obj
            if isinstance(obj, ctypes.Structure):
                return {'struct': hashlib.sha1(bytes(obj)).hexdigest()[:12]}
            return {'byref': type(obj).__name__}
        if isinstance(a, ctypes.c_void_p):
            if a.value is None:
                return None
            array = self.arrays.get(a.value, getattr(a, '_arr', None))
            if array is not None:
                d = {'dtype': str(array.dtype), 'shape': list(array.shape)}
                if not is_output:
                    assert array.flags.c_contiguous
                    d['sha'] = hashlib.sha1(array.tobytes()).hexdigest()[:12]
                return d
            return HANDLES.get(a.value, 'opaque')
        if isinstance(a, ctypes._SimpleCData):
            return a.value
        raise TypeError(f'unrecorded argument type {type(a)}')


def run(case):
    """The calls `case(engine)` makes, as JSON gives them back."""
    from text_to_speech_amd.engine import HipEngine
    lib = Recorder()
    real = HipEngine.__dict__['_ptr']

    def ptr(x):
        p = real.__func__(x)
        if x is not None and not isinstance(x, ctypes.c_void_p):
            lib.register(p, x)
        return p

    HipEngine._ptr = staticmethod(ptr)
    try:
        eng = HipEngine.__new__(HipEngine)
        eng._lib, eng._h, eng.device = lib, ctypes.c_void_p(ENGINE), 0
        try:
            case(eng)
        finally:
            eng._h = None                                  # nothing to destroy
    finally:
        HipEngine._ptr = real
    return json.loads(json.dumps(lib.calls))


# ---------------------------------------------------------------------------------------------------------------- inputs
def ramp(*shape, k=0):
    """float64 in [-0.5, 0.5), from integer arithmetic and one correctly rounded division: the same bits everywhere."""
    n = int(np.prod(shape))
    return (((np.arange(n, dtype=np.int64) * 7919 + k * 104729) % 10007) / 10007.0 - 0.5).reshape(shape)


B, T, TIN, N = 2, 4, 5, 3000
MEL = ramp(B, T, 80, k=1) * 10 - 5                                         # float64
Z = ramp(B, 8, T * 32, k=2).transpose(0, 2, 1)                             # float64, not contiguous
WAV = ramp(B, T * 256, k=3).astype(np.float32)
TOKENS = ((np.arange(B * TIN * 2).reshape(B, TIN * 2) * 7) % 30 + 1)[:, ::2]      # int64, not contiguous
SPEAKER = ramp(B, 16, k=4)
FRAMES_IN = ramp(B, 6, 80, k=5)                                            # teacher-forced T = 6
AUDIO = ramp(B, 2 * N, k=6)[:, ::2]                                        # float64, not contiguous
ROW = ramp(N, k=7).astype(np.float32)                                      # one 1-D row
LENS = [N, N // 2]
CFG = dict(sampling_rate=22050, n_mel_channels=80, filter_length=1024, hop_length=256, win_length=1024, mel_fmin=0.0,
           mel_fmax=8000.0)
BINS = 513
KEYS = ([3, 2 ** 64 - 1], [0, 2 ** 33])


def masks(t, k):
    return (ramp(B, t, 2, 256, k=k) > 0) * 2.0


def _encode_decode(eng, **kw):
    enc = eng.tacotron2_encode(TOKENS)
    eng.tacotron2_decode(enc, max_len=8, **kw)
    enc.close()


def _reencode(eng):
    enc = eng.tacotron2_encode(TOKENS, speaker=SPEAKER)
    assert eng.tacotron2_encode(TOKENS[:, :3], into=enc) is enc and enc.Tin == 3
    enc.close()


def _forward_encoded(eng):
    enc = eng.tacotron2_encode(TOKENS)
    eng.tacotron2_forward(enc, FRAMES_IN, mel_lengths=[6, 3], prenet_masks=masks(6, 9), precision='f16')
    enc.close()


def _loss_inputs():
    return [ramp(B, 6, 80, k=11), (ramp(B, 6, k=12) > 0).astype(np.float64), ramp(B, 6, 80, k=13).astype(np.float32),
            ramp(B, 80, 6, k=14).transpose(0, 2, 1), ramp(B, 6, k=15) + 0.5]


def _misc(eng):
    eng.set_tensor('waveglow.start.bias', ramp(2, 3, k=16))
    eng.load_weights('weights.bin')
    eng.finalize()
    eng.has_model('waveglow')
    eng.set_decoder_mode('fused')
    eng.set_waveglow_form('direct')
    assert (eng.last_decoder_mode, eng.last_waveglow_form, eng.last_waveglow_tiles) == ('graph', 'direct', '256-row')
    assert eng.last_conv_paths == 0 and eng.waveglow_channels == CHANNELS
    eng.kernel_timing(True)
    eng.kernel_time_us(1)
    eng.probe_mfma_f32()
    eng.synchronize()
    eng.close()


def _plans(eng):
    a = eng.mel_fn(CFG)
    assert eng.mel_fn(dict(CFG)) is a                                       # cached by value: one create
    b = eng.mel_fn(dict(CFG, kind='whisper', normalize_mode='per_feature', pre_emph=0.97), window=np.hanning(1024))
    assert b is not a
    assert eng.mel_fn_frames(a, N) == FRAMES and eng.mel_fn_samples(a, 8) == SAMPLES


CASES = {
    'misc': _misc,
    # ---- WaveGlow
    'waveglow_infer': lambda e: e.waveglow_infer(MEL),
    'waveglow_infer_z_f16': lambda e: e.waveglow_infer(MEL, z=Z, sigma=0.7, precision='f16'),
    'waveglow_infer_z_f16x3': lambda e: e.waveglow_infer(MEL.astype(np.float32), z=Z, precision='f16x3'),
    'waveglow_infer_seed': lambda e: e.waveglow_infer(MEL, seed=2 ** 64 + 5, offset=9, precision='f16x3'),
    'waveglow_infer_lengths': lambda e: e.waveglow_infer(MEL, z=Z, lengths=[4, 2]),
    'waveglow_infer_lengths_no_z': lambda e: e.waveglow_infer(MEL, lengths=np.asarray([4, 0])),
    'waveglow_infer_packed': lambda e: e.waveglow_infer(MEL, z=Z, lengths=[4, 2], packed=True, precision='f16'),
    'waveglow_infer_row_seeds': lambda e: e.waveglow_infer(MEL, row_seeds=KEYS),
    'waveglow_infer_row_seeds_packed': lambda e: e.waveglow_infer(MEL, row_seeds=([1, 2], None), lengths=[4, 2], packed=True),
    'waveglow_encode': lambda e: e.waveglow_encode(WAV.astype(np.float64), MEL),
    'waveglow_encode_lengths': lambda e: e.waveglow_encode(WAV, MEL, lengths=[4, 2]),
    'waveglow_encode_probe': lambda e: e.waveglow_encode_probe(WAV, MEL, flow=5),
    'waveglow_encode_probe_slog': lambda e: e.waveglow_encode_probe(WAV, MEL, lengths=[4, 2], flow=-1, what='slog'),
    'waveglow_probe': lambda e: e.waveglow_probe(MEL, flow=3, layer=2),
    'waveglow_probe_state_z': lambda e: e.waveglow_probe(MEL, z=Z, precision='f16x3', flow=4, what='state'),
    'waveglow_probe_cond': lambda e: e.waveglow_probe(MEL, z=Z, what='cond', layer=1),
    'waveglow_probe_lengths': lambda e: e.waveglow_probe(MEL, z=Z, precision='f16', flow=8, what='state', lengths=[4, 2]),
    'waveglow_probe_packed': lambda e: e.waveglow_probe(MEL, lengths=np.asarray([3, 2]), packed=True, layer=5),
    'waveglow_probe_acts': lambda e: e.waveglow_probe_acts(MEL),
    'waveglow_probe_acts_z': lambda e: e.waveglow_probe_acts(MEL, z=Z, sigma=0.5, flow=2, layer=3),
    # ---- Tacotron2
    'tacotron2_infer': lambda e: e.tacotron2_infer(TOKENS, max_len=8),
    'tacotron2_infer_all': lambda e: e.tacotron2_infer(TOKENS.tolist(), speaker=SPEAKER, max_len=8, early_stopping=False,
                                                       prenet_masks=masks(8, 8), attn_mask_win_len=3, attn_mask_offset=1,
                                                       want_attention=False, precision='f16'),
    'tacotron2_infer_row_mask_seeds': lambda e: e.tacotron2_infer(TOKENS, speaker=SPEAKER, max_len=8, row_mask_seeds=KEYS),
    'tacotron2_encode_into': _reencode,
    'tacotron2_decode': lambda e: _encode_decode(e),
    'tacotron2_decode_masks': lambda e: _encode_decode(e, prenet_masks=masks(8, 8), early_stopping=False, attn_mask_win_len=4,
                                                       want_attention=False, precision='f16'),
    'tacotron2_decode_mask_seed': lambda e: _encode_decode(e, mask_seed=(7, 2 ** 40)),
    'tacotron2_decode_row_mask_seeds': lambda e: _encode_decode(e, row_mask_seeds=([5, 6], 512)),
    'tacotron2_forward': lambda e: e.tacotron2_forward(TOKENS, FRAMES_IN),
    'tacotron2_forward_all': lambda e: e.tacotron2_forward(TOKENS, FRAMES_IN.astype(np.float32), mel_lengths=np.asarray([6, 3]),
                                                           speaker=SPEAKER, prenet_masks=masks(6, 9)),
    'tacotron2_forward_encoded': _forward_encoded,
    'tacotron2_loss': lambda e: e.tacotron2_loss(*_loss_inputs()),
    'tacotron2_loss_all': lambda e: e.tacotron2_loss(*_loss_inputs(), mel_loss=['mae', 'weighted_mse'], mask_mel_padding=False,
                                                     from_logits=True, finish_weight=2.0, not_finish_weight=0.5),
    'tacotron2_probe_encoder': lambda e: e.tacotron2_probe_encoder(TOKENS, what='conv2'),
    'tacotron2_probe_encoder_speaker': lambda e: e.tacotron2_probe_encoder(TOKENS, speaker=SPEAKER),
    'tacotron2_probe_postnet': lambda e: e.tacotron2_probe_postnet(FRAMES_IN, [5, 2], what='conv4'),
    'tacotron2_postnet': lambda e: e.tacotron2_postnet(FRAMES_IN, np.asarray([5, 2], np.int64)),
    # ---- mel-STFT and mel plans
    'mel_stft': lambda e: e.mel_stft(AUDIO),
    'mel_stft_row': lambda e: e.mel_stft(ROW),
    'mel_stft_short': lambda e: e.mel_stft(ROW[:700]),
    'mel_stft_probe': lambda e: e.mel_stft_probe(ROW, what='magnitude'),
    'mel_fn': _plans,
    'mel_fn_run': lambda e: e.mel_fn_run(e.mel_fn(CFG), AUDIO),
    'mel_fn_run_lengths': lambda e: e.mel_fn_run(e.mel_fn(CFG), AUDIO, lengths=LENS),
    'mel_fn_run_row': lambda e: e.mel_fn_run(e.mel_fn(CFG), ROW, lengths=[N - 1]),
    'mel_fn_probe': lambda e: e.mel_fn_probe(e.mel_fn(CFG), AUDIO, what='mel_log', lengths=LENS),
    'mel_fn_probe_row': lambda e: e.mel_fn_probe(e.mel_fn(CFG), ROW, what='padded'),
    # ---- STFT with phase, Griffin-Lim, denoiser
    'stft_transform': lambda e: e.stft_transform(e.mel_fn(CFG), AUDIO),
    'stft_transform_lengths': lambda e: e.stft_transform(e.mel_fn(CFG), ROW, lengths=[N - 1], polar=False),
    'stft_inverse': lambda e: e.stft_inverse(e.mel_fn(CFG), ramp(8, BINS, k=20), ramp(8, BINS, k=21)),
    'stft_inverse_frames': lambda e: e.stft_inverse(e.mel_fn(CFG), ramp(B, BINS, 8, k=20).transpose(0, 2, 1),
                                                    ramp(B, 8, BINS, k=21).astype(np.float32), frames=[8, 3], polar=False),
    'griffin_lim': lambda e: e.griffin_lim(e.mel_fn(CFG), ramp(8, BINS, k=22) + 0.5, n_iters=2),
    'griffin_lim_all': lambda e: e.griffin_lim(e.mel_fn(CFG), ramp(B, 8, 80, k=23), frames=[8, 3], kind='log_mel', n_iters=2,
                                               momentum=0.5, init=ramp(B, 8, BINS, 2, k=24), mel_inverse=ramp(80, BINS, k=25)),
    'griffin_lim_probe': lambda e: e.griffin_lim_probe(e.mel_fn(CFG), ramp(8, BINS, k=22) + 0.5, 1, 'signal'),
    'griffin_lim_probe_all': lambda e: e.griffin_lim_probe(e.mel_fn(CFG), ramp(B, 8, 80, k=23), 0, 'phasor', frames=[8, 3],
                                                           kind='log_mel', init=ramp(B, 8, BINS, 2, k=24),
                                                           mel_inverse=ramp(80, BINS, k=25)),
    'denoise': lambda e: e.denoise(e.mel_fn(CFG), AUDIO, ramp(BINS, k=26) + 0.5),
    'denoise_lengths': lambda e: e.denoise(e.mel_fn(CFG), ROW, ramp(BINS, k=26).astype(np.float32) + 0.5, strength=0.3,
                                           lengths=[N - 1]),
    'denoise_probe': lambda e: e.denoise_probe(e.mel_fn(CFG), AUDIO, ramp(BINS, k=26) + 0.5, 0.1, 'frames', lengths=LENS),
    # ---- waveform clean-up, resampling, silence removal
    'reduce_noise': lambda e: e.reduce_noise(AUDIO, rate=22050),
    'reduce_noise_all': lambda e: e.reduce_noise(AUDIO, lengths=LENS, noise=ramp(B, 800, k=27)[:, ::2], renormalize=True),
    'reduce_noise_row': lambda e: e.reduce_noise(ROW, noise=ramp(300, k=28), noise_length=100),
    'reduce_noise_probe': lambda e: e.reduce_noise_probe(AUDIO, lengths=LENS, noise_length=500, what='mask'),
    'reduce_noise_probe_noise': lambda e: e.reduce_noise_probe(ROW, noise=ramp(300, k=28), what='threshold'),
    'trim_silence': lambda e: e.trim_silence(AUDIO, rate=22050),
    'trim_silence_all': lambda e: e.trim_silence(ROW, lengths=[N - 1], threshold=0.2, window_length=100, add_start=1, add_end=0.5,
                                                 mode='end'),
    'trim_silence_probe': lambda e: e.trim_silence_probe(AUDIO, lengths=LENS, window_length=101),
    'resample': lambda e: e.resample(AUDIO, 22050, 16000),
    'resample_lengths': lambda e: e.resample(ROW, 22050, 16000, lengths=[N // 2]),
    'resample_same_rate': lambda e: e.resample(AUDIO, 16000, 16000),
    'resample_same_rate_lengths': lambda e: e.resample(AUDIO, 16000, 16000, lengths=LENS),
    'resample_probe': lambda e: e.resample_probe(AUDIO, 22050, 16000, lengths=LENS),
    'resample_fft_probe': lambda e: e.resample_fft_probe(ramp(3, 64, k=29) + 1j * ramp(3, 64, k=30), inverse=True),
    'remove_silence': lambda e: e.remove_silence(AUDIO, 22050),
    'remove_silence_all': lambda e: e.remove_silence(AUDIO, 22050, lengths=LENS, method='remove', threshold=0.05, min_silence=0.05),
    'remove_silence_row': lambda e: e.remove_silence(ROW, 16000, method='threshold', mode='end'),
    'remove_silence_probe': lambda e: e.remove_silence_probe(AUDIO, 22050, 'flags', lengths=LENS, mode='remove', replace_by=0.1),
}


def test_the_fixture_holds_exactly_these_cases():
    assert sorted(json.load(open(GOLDEN))) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_library_calls_are_the_recorded_ones(name):
    want = json.load(open(GOLDEN))[name]
    got = run(CASES[name])
    assert [c[0] for c in got] == [c[0] for c in want]                         # the symbols, in order
    for g, w in zip(got, want):
        assert g == w


# ------------------------------------------------------------------------------------------------------------ refusals
STREAM = object()                                     # never looked at: host arrays refuse any stream
PLANE = ramp(B, 8, BINS, k=20)
REFUSALS = {
    # a stream with host arrays, for every call that takes one and runs on host arrays
    'waveglow_infer_stream': (lambda e: e.waveglow_infer(MEL, stream=STREAM), 'stream= needs device tensors'),
    'waveglow_encode_stream': (lambda e: e.waveglow_encode(WAV, MEL, stream=STREAM), 'stream= needs device tensors'),
    'tacotron2_encode_stream': (lambda e: e.tacotron2_encode(TOKENS, stream=STREAM), 'stream= needs device tensors'),
    'tacotron2_forward_stream': (lambda e: e.tacotron2_forward(TOKENS, FRAMES_IN, stream=STREAM), 'stream= needs device tensors'),
    'tacotron2_loss_stream': (lambda e: e.tacotron2_loss(*_loss_inputs(), stream=STREAM), 'stream= needs device tensors'),
    'mel_stft_stream': (lambda e: e.mel_stft(AUDIO, stream=STREAM), 'stream= needs device tensors'),
    'griffin_lim_stream': (lambda e: e.griffin_lim(_plan(e), PLANE, stream=STREAM), 'stream= needs device tensors'),
    'denoise_stream': (lambda e: e.denoise(_plan(e), AUDIO, ramp(BINS), stream=STREAM), 'stream= needs device tensors'),
    'reduce_noise_stream': (lambda e: e.reduce_noise(AUDIO, rate=22050, stream=STREAM), 'stream= needs device tensors'),
    'resample_stream': (lambda e: e.resample(AUDIO, 22050, 16000, stream=STREAM), 'stream= needs device tensors'),
    'resample_same_rate_stream': (lambda e: e.resample(AUDIO, 16000, 16000, stream=STREAM), 'stream= needs device tensors'),
    'remove_silence_stream': (lambda e: e.remove_silence(AUDIO, 22050, stream=STREAM), 'stream= needs device tensors'),
    # shapes
    'waveglow_infer_mel': (lambda e: e.waveglow_infer(MEL[..., :79]), r'mel must be \[B, T, 80\]'),
    'waveglow_infer_z': (lambda e: e.waveglow_infer(MEL, z=Z[:, :-1]), r'z must be \[B, T\*32, 8\]'),
    'waveglow_encode_audio': (lambda e: e.waveglow_encode(WAV[:, :-1], MEL), r'audio must be \[B, T\*256\]'),
    'waveglow_encode_probe_mel': (lambda e: e.waveglow_encode_probe(WAV, MEL[0]), r'mel must be \[B, T, 80\]'),
    'waveglow_probe_z': (lambda e: e.waveglow_probe(MEL, z=Z[:1]), r'z must be \[B, T\*32, 8\]'),
    'waveglow_probe_packed_alone': (lambda e: e.waveglow_probe(MEL, packed=True), 'packed=True needs lengths'),
    'waveglow_probe_lengths_range': (lambda e: e.waveglow_probe(MEL, lengths=[5, 2]), r'lengths must lie in \[0, '),
    'waveglow_probe_acts_mel': (lambda e: e.waveglow_probe_acts(MEL[0]), r'mel must be \[B, T, 80\]'),
    'tacotron2_infer_tokens': (lambda e: e.tacotron2_infer(TOKENS[0]), r'tokens must be \[B, Tin\]'),
    'tacotron2_infer_masks': (lambda e: e.tacotron2_infer(TOKENS, max_len=8, prenet_masks=masks(7, 8)),
                              r'prenet_masks must be \[B, max_len, 2, 256\]'),
    'tacotron2_infer_max_len': (lambda e: e.tacotron2_infer(TOKENS, max_len=0), 'max_len must be positive'),
    'tacotron2_probe_postnet_frames': (lambda e: e.tacotron2_probe_postnet(FRAMES_IN[0], [5]), r'frames must be \[B, T, 80\]'),
    'tacotron2_probe_postnet_lengths': (lambda e: e.tacotron2_probe_postnet(FRAMES_IN, [5, 2, 1]), 'lengths must '),
    'tacotron2_loss_gate': (lambda e: e.tacotron2_loss(MEL, MEL[..., 0], MEL, MEL, MEL), 'stop_tokens must be'),
    'stft_inverse_planes': (lambda e: e.stft_inverse(_plan(e), PLANE, PLANE[:, :7]), r'planes must both be \[F, C\] or \[B, F, C\]'),
    'stft_inverse_bins': (lambda e: e.stft_inverse(_plan(e), PLANE[..., :512], PLANE[..., :512]), '512 bins, the plan has 513'),
    'griffin_lim_spec': (lambda e: e.griffin_lim(_plan(e), PLANE[0, 0]), r'spec must be \[F, C\] or \[B, F, C\]'),
    'griffin_lim_mel_inverse': (lambda e: e.griffin_lim(_plan(e), PLANE, mel_inverse=ramp(80, BINS)), "goes with kind='log_mel'"),
    'denoise_bias': (lambda e: e.denoise(_plan(e), AUDIO, ramp(BINS - 1)), r'bias must be \[513\]'),
    'mel_fn_run_audio': (lambda e: e.mel_fn_run(_plan(e), AUDIO[None]), r'audio must be \[N\] or \[B, N\]'),
    'reduce_noise_noise': (lambda e: e.reduce_noise(AUDIO, noise=ramp(3, 100)), r'noise must be \[noise_len\]'),
    # row tables: shape, dtype and range
    'waveglow_infer_lengths_shape': (lambda e: e.waveglow_infer(MEL, lengths=[4]), r'lengths must hold one .* per row, shape \(2,\)'),
    'waveglow_infer_lengths_float': (lambda e: e.waveglow_infer(MEL, lengths=[4.0, 2.0]), 'lengths must be integers'),
    'waveglow_infer_lengths_range': (lambda e: e.waveglow_infer(MEL, lengths=[5, 2]), r'lengths must lie in \[0, '),
    'waveglow_encode_lengths_range': (lambda e: e.waveglow_encode(WAV, MEL, lengths=[-1, 2]), r'lengths must lie in \[0, '),
    'waveglow_encode_probe_lengths': (lambda e: e.waveglow_encode_probe(WAV, MEL, lengths=[[4, 2]]), 'lengths must hold one '),
    'waveglow_infer_row_seeds': (lambda e: e.waveglow_infer(MEL, row_seeds=([1, 2, 3], None)), 'row_seeds: need one key and one offset per row'),
    'tacotron2_forward_mel_lengths': (lambda e: _forward_refused(e), 'mel_lengths must '),
    'stft_inverse_frames_shape': (lambda e: e.stft_inverse(_plan(e), PLANE, PLANE, frames=[8]), r'stft_inverse: frames must .*shape \(2,\)'),
    'stft_inverse_frames_range': (lambda e: e.stft_inverse(_plan(e), PLANE, PLANE, frames=[8, 0]), r'stft_inverse: frames must lie in \[1, 8\]'),
    'griffin_lim_frames_range': (lambda e: e.griffin_lim(_plan(e), PLANE, frames=[9, 1]), r'griffin_lim: frames must lie in \[1, 8\]'),
    'mel_fn_run_lengths_shape': (lambda e: e.mel_fn_run(_plan(e), AUDIO, lengths=[N]), r'mel_fn_run: lengths must .*shape \(2,\)'),
    'denoise_lengths_range': (lambda e: e.denoise(_plan(e), AUDIO, ramp(BINS), lengths=[N, 0]), r'denoise: lengths must lie in \[1, 3000\]'),
    'resample_lengths_range': (lambda e: e.resample(AUDIO, 22050, 16000, lengths=[N + 1, 1]), r'resample: lengths must lie in \[1, 3000\]'),
    'trim_silence_lengths_shape': (lambda e: e.trim_silence(AUDIO, rate=22050, lengths=[N, N, N]), r'trim_silence: lengths must .*shape \(2,\)'),
}


def _plan(eng):
    """A plan that cost no library call: the refusals below must leave the recorder empty."""
    from text_to_speech_amd.engine import MelFn
    from text_to_speech_amd._lib import MelConfigC
    return MelFn(ctypes.c_void_p(PLAN), MelConfigC(0, 22050, 80, 1024, 256, 1024, 0, 0.0, 8000.0, 0.0))


def _forward_refused(eng):
    """`tacotron2_forward` on an encoded batch that cost no library call."""
    from text_to_speech_amd.engine import EncodedBatch
    enc = EncodedBatch(eng, ctypes.c_void_p(ENCODED), B, TIN)
    try:
        eng.tacotron2_forward(enc, FRAMES_IN, mel_lengths=[6, 3, 1])
    finally:
        enc.handle = None


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_a_bad_argument_raises_before_any_library_call(name):
    case, match = REFUSALS[name]
    calls = None

    def guarded(eng):
        nonlocal calls
        calls = eng._lib.calls
        with pytest.raises(ValueError, match=match):
            case(eng)

    run(guarded)
    assert calls == []


if __name__ == '__main__':
    with open(GOLDEN, 'w') as f:
        json.dump({name: run(case) for name, case in sorted(CASES.items())}, f, indent=0, separators=(',', ':'))
        f.write('\n')
    print(f'wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(CASES)} cases')
