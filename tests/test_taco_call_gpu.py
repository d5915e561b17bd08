"""GPU: every tts_hip_tacotron2_* entry point goes through one front end (csrc/taco_call.h; taco_encode, taco_run and taco_infer
in csrc/tacotron2.hip; the `HipEngine` methods are one staging path in front of them).  So every refusal reads the same through
every symbol that can give it and touches nothing, and every route to one result gives the same bits.

The shape is the session's smallest with a full, a partial and a nearly empty row: B = 3 rows of 12 / 7 / 3 tokens padded to 12,
max_len = T = 33 (one step into the second 32-step chunk), the fused step in `auto` mode.  Other tests assert some of these
equalities on other inputs and in f32 only (tests/test_boundary_gpu.py: infer against encode + decode, mask_seed against the
restated stream; tests/test_row_streams_gpu.py: row_mask_seeds against explicit masks, mel only; tests/test_teacher_forced_gpu.py:
CUDA against numpy input of the forward pass); none on these, in f16, on a caller's stream or on all five outputs."""
import ctypes

import numpy as np
import pytest

from taco_call_cases import B, LEN, REFUSALS, TIN

pytestmark = pytest.mark.gpu

LENS = (12, 7, 3)
KEYS, OFFS = (11, 2 ** 63 + 5, 77), (0, 9, 4)
SEED, OFFSET = 5, 3
SENTINEL = 7.0
OUTPUTS = ('decoder_output', 'mel', 'stop_tokens', 'attention_weights', 'lengths')

p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr()) if hasattr(a, 'data_ptr') else a.ctypes.data_as(ctypes.c_void_p)
u64 = lambda v: ctypes.c_uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope='module')
def case(taco_weights, taco_cfg):
    """Tokens, masks and a shifted target, and the oracle's free-running result: computed once, shared, never modified."""
    from oracle import tacotron2_ref
    rng = np.random.default_rng(31)
    tok = np.zeros((B, TIN), np.int32)
    for b, n in enumerate(LENS):
        tok[b, :n] = rng.integers(1, 148, n)
    masks = (rng.random((B, LEN, 2, 256)) >= 0.5).astype(np.float32) * 2.0
    x = rng.uniform(-8.0, 1.0, (B, LEN, 80)).astype(np.float32)
    x[:, 0] = 0.0                                                               # the go-frame
    ref = tacotron2_ref.infer(tok, taco_weights, taco_cfg, max_length=LEN, early_stopping=False)
    return dict(tok=tok, masks=masks, x=x, mel_lengths=np.asarray((33, 17, 1), np.int32), ref=ref)


def _host(out):
    return [None if v is None else v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v) for v in out]


def _assert_same(a, b, what):
    a, b = _host(a), _host(b)
    assert len(a) == len(b)
    for name, u, v in zip(OUTPUTS, a, b):
        assert u.shape == v.shape and np.array_equal(u, v), f'{what}: {name} differs'
    assert np.isfinite(a[1]).all() and a[1].any()


# ---- every route to one result gives the same bits ---------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['f32', 'f16'])
def test_infer_is_encode_plus_decode_from_every_kind_of_input(gpu_engine, case, prec):
    import torch
    eng, kw = gpu_engine, dict(max_len=LEN, early_stopping=False, precision=prec)
    dtok, st = torch.as_tensor(case['tok']).cuda(), torch.cuda.Stream()
    for what, m in (('deterministic', None), ('masks', case['masks'])):
        dm = None if m is None else torch.as_tensor(m).cuda()
        whole = eng.tacotron2_infer(case['tok'], prenet_masks=m, **kw)
        assert eng.last_steps == LEN and isinstance(whole.mel, np.ndarray)
        enc = eng.tacotron2_encode(case['tok'])
        _assert_same(eng.tacotron2_decode(enc, prenet_masks=m, **kw), whole, f'{prec} {what}: encode + decode')
        enc.close()
        on_device = eng.tacotron2_infer(dtok, prenet_masks=dm, **kw)
        assert on_device.mel.is_cuda and on_device.lengths.is_cuda
        _assert_same(on_device, whole, f'{prec} {what}: infer on CUDA tensors')
        for stream in (None, st):
            enc = eng.tacotron2_encode(dtok, stream=stream)
            parts = eng.tacotron2_decode(enc, prenet_masks=dm, stream=stream, **kw)
            assert parts.mel.is_cuda
            _assert_same(parts, whole, f'{prec} {what}: encode + decode on CUDA tensors, stream={stream is not None}')
            enc.close()
    plain = eng.tacotron2_infer(case['tok'], **kw)
    assert not np.array_equal(plain.mel, whole.mel)                              # the masks were applied


@pytest.mark.parametrize('prec', ['f32', 'f16'])
def test_drawn_masks_are_their_tensors(gpu_engine, case, prec):
    eng, kw = gpu_engine, dict(max_len=LEN, early_stopping=False, precision=prec)
    enc = eng.tacotron2_encode(case['tok'])
    try:
        drawn = eng.random_prenet_masks(B, LEN, SEED, OFFSET).cpu().numpy()
        seeded = eng.tacotron2_decode(enc, mask_seed=(SEED, OFFSET), **kw)
        _assert_same(seeded, eng.tacotron2_decode(enc, prenet_masks=drawn, **kw), f'{prec}: mask_seed')
        rows = eng.random_prenet_masks_rows(LEN * 512, KEYS, OFFS).view(B, LEN, 2, 256).cpu().numpy()
        by_row = eng.tacotron2_decode(enc, row_mask_seeds=(KEYS, OFFS), **kw)
        _assert_same(by_row, eng.tacotron2_decode(enc, prenet_masks=rows, **kw), f'{prec}: row_mask_seeds')
        assert not np.array_equal(seeded.mel, by_row.mel)
    finally:
        enc.close()


@pytest.mark.parametrize('prec', ['f32', 'f16'])
def test_forward_from_every_kind_of_input(gpu_engine, case, prec):
    import torch
    eng = gpu_engine
    dtok, dx, st = torch.as_tensor(case['tok']).cuda(), torch.as_tensor(case['x']).cuda(), torch.cuda.Stream()
    for what, m in (('deterministic', None), ('masks', case['masks'])):
        dm = None if m is None else torch.as_tensor(m).cuda()
        host = eng.tacotron2_forward(case['tok'], case['x'], case['mel_lengths'], prenet_masks=m, precision=prec)
        assert isinstance(host.mel, np.ndarray) and host.mel.shape == (B, LEN, 80)
        for stream in (None, st):
            dev = eng.tacotron2_forward(dtok, dx, case['mel_lengths'], prenet_masks=dm, precision=prec, stream=stream)
            assert dev.mel.is_cuda
            _assert_same(dev, host, f'{prec} {what}: forward on CUDA tensors, stream={stream is not None}')


# ---- refusals -------------------------------------------------------------------------------------------------------------------
ENCODES = ['tts_hip_tacotron2_encode', 'tts_hip_tacotron2_reencode', 'tts_hip_tacotron2_infer', 'tts_hip_tacotron2_infer_f16',
           'tts_hip_tacotron2_probe_encoder']
DECODES = ['tts_hip_tacotron2_decode', 'tts_hip_tacotron2_decode_seeded', 'tts_hip_tacotron2_decode_rows_seeded']
INFERS = ENCODES[2:4]
SYMBOLS = ENCODES + DECODES + ['tts_hip_tacotron2_forward']


def _applies(sym, kind, reason):
    """Can `sym` give this row of tests/taco_call_cases.py?  infer gives what encode gives, and of decode's reasons only a bad
    max_len (its precision, mask source and encoded batch are its own)."""
    if kind == 'encode':
        return sym in ENCODES
    if kind == 'forward':
        return sym.endswith('forward')
    if sym in INFERS:
        return reason == 'max_len = 0'
    return sym in DECODES and (not reason.endswith(' NULL') or reason == 'encoded NULL' or sym.endswith('rows_seeded'))


def _c_args(sym, c):
    outs = (p(c['mel']), p(c['dec']), p(c['stop']), p(c['attn']))
    tail = (p(c['lengths']), ctypes.cast(ctypes.byref(c['steps']), ctypes.c_void_p))
    tokens = (p(c['tokens']), c['B'], c['Tin'], p(c['speaker']))
    if sym in INFERS:
        return tokens + (c['max_len'], 0, None, 0, 0) + outs + tail + (c['mem'],)
    if sym.endswith('reencode'):
        return (c['into'],) + tokens + (c['mem'], None)
    if sym.endswith('encode'):
        return tokens + (c['mem'], None, ctypes.byref(c['new']))
    if sym.endswith('probe_encoder'):
        return tokens + (3, p(c['dec']), c['mem'])
    if sym.endswith('forward'):
        return (c['encoded'], p(c['mel_input']), c['T'], p(c['mel_lengths']), None, c['precision']) + outs + (c['mem'], None)
    mid = (p(c['keys']), p(c['offsets'])) if sym.endswith('rows_seeded') else (u64(SEED), u64(OFFSET)) if sym.endswith('seeded') else (None,)
    return (c['encoded'], c['max_len'], 0) + mid + (0, 0, c['precision']) + outs + tail + (c['mem'], None)


@pytest.fixture(scope='module')
def other_engines(gpu_engine):
    """A handle without weights, and one whose 768-wide model needs a speaker, with a batch it encoded."""
    from text_to_speech_amd import weights
    from text_to_speech_amd.config import Tacotron2Config
    from text_to_speech_amd.engine import HipEngine
    bare, wide = HipEngine(0), HipEngine(0)
    wide.load_state(weights.synth_tacotron2(Tacotron2Config(speaker_embedding_dim=256), seed=1234))
    wide.finalize()
    enc768 = wide.tacotron2_encode(np.ones((B, TIN), np.int32), speaker=np.zeros((B, 256), np.float32))
    yield bare, wide, enc768
    enc768.close()
    wide.close()
    bare.close()


@pytest.mark.parametrize('sym', SYMBOLS)
def test_refusals_through_every_entry_point(gpu_engine, other_engines, case, sym):
    """Each row of tests/taco_call_cases.py the symbol can give: its status, and the symbol's name and the exact reason as the
    handle's last error; nothing was copied or launched (the outputs keep their bytes).  Then the handle still infers right."""
    bare, wide, enc768 = other_engines
    lib = gpu_engine._lib
    enc, into = gpu_engine.tacotron2_encode(case['tok']), gpu_engine.tacotron2_encode(case['tok'])
    outs = dict(mel=np.full((B, LEN, 80), SENTINEL, np.float32), dec=np.full((B, LEN, 80), SENTINEL, np.float32),
                stop=np.full((B, LEN), SENTINEL, np.float32), attn=np.full((B, LEN, TIN), SENTINEL, np.float32),
                lengths=np.full((B,), 7, np.int32), steps=ctypes.c_int32(-7), new=ctypes.c_void_p())
    good = dict(outs, tokens=case['tok'], B=B, Tin=TIN, speaker=None, encoded=enc.handle, into=into.handle, max_len=LEN, T=LEN,
                precision=0, mem=0, keys=np.asarray(KEYS, np.uint64), offsets=np.asarray(OFFS, np.uint64), mel_input=case['x'],
                mel_lengths=case['mel_lengths'])
    ran = 0
    try:
        for kind, reason, wrong, code, text in REFUSALS:
            if not _applies(sym, kind, reason):
                continue
            eng, c = gpu_engine, dict(good)
            for k, v in wrong.items():
                if k == 'ready':
                    eng = bare
                elif k == 'spk_dim':
                    eng = wide
                elif k == 'enc':
                    c['encoded'] = enc768.handle
                elif k == 'null':
                    c[{'tokens': 'tokens', 'speaker': 'speaker', 'encoded': 'encoded', 'keys': 'keys', 'offsets': 'offsets',
                       'mel': 'mel_input', 'lens': 'mel_lengths'}[v]] = None
                elif k == 'lens':
                    c['mel_lengths'] = np.asarray(v, np.int32)
                elif k != 'masks':                                                # (the symbol is the mask source)
                    c[k] = v
            rc = getattr(lib, sym)(eng._h, *_c_args(sym, c))
            msg = lib.tts_hip_last_error(eng._h).decode()
            assert (rc, msg) == (code, f'{sym[len("tts_hip_"):]}: {text}'), (reason, rc, msg)
            ran += 1
        assert ran >= 6
        gpu_engine.synchronize()
        for name in ('mel', 'dec', 'stop', 'attn'):
            assert np.all(outs[name] == SENTINEL), name
        assert np.all(outs['lengths'] == 7) and outs['steps'].value == -7 and not outs['new'].value
        out = gpu_engine.tacotron2_infer(case['tok'], max_len=LEN, early_stopping=False)          # and the handle is as good as ever
        assert gpu_engine.last_steps == LEN and np.abs(out.mel - case['ref'].mel).max() <= 1e-3
    finally:
        enc.close()
        into.close()
