"""GPU: HipEngine.tacotron2_loss (tts_hip_tacotron2_loss, csrc/taco_loss.hip), HipRuntime / TacotronLoss on top of it and
Tacotron2.evaluate against the float64 restatement of the reference's TacotronLoss (tests/taco_loss_ref.py).

Every output of every case is held to |got - ref| <= 2e-6 |ref| + 1e-12 (taco_loss_ref.RTOL / ATOL).  The bound: all partial
sums are float64 from the per-thread accumulator on, so what remains is the float32 rounding of one element's chain -- at most
about eight roundings for the weighted kinds (y - p, its square, y - ymin, + 1, ymax - ymin, + 1, the quotient, the product),
8 x 2^-24 = 4.8e-7 relative on sums of non-negative terms -- and the float32 rounding of the result, 6e-8; the gate term is
float64 throughout.  tests/test_taco_loss.py shows the bound is below a tenth of every planted mistake on these very cases.
The largest error seen on an MI355X is in DESIGN.md section 4.3e.

Inputs: seeded finite data (taco_loss_ref.make_inputs), padded frames -11, the prepare_data gate pattern unless the case says
otherwise; CHUNK = the kernel's frames per chunk.
"""
import ctypes
import os

import numpy as np
import pytest

import taco_loss_ref as lr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = ('mel_target', 'gate_target', 'decoder_output', 'mel', 'stop_tokens')


def _engine_kw(loss_kw):
    kw = dict(loss_kw)
    if 'mel_loss_kinds' in kw:
        kw['mel_loss'] = kw.pop('mel_loss_kinds')
    return kw


def _run(engine, inputs, loss_kw, **extra):
    return engine.tacotron2_loss(*(inputs[k] for k in NAMES), **_engine_kw(loss_kw), **extra)


def _check(got, ref, what):
    ok, ratio = lr.within(got, ref)
    print(f'{what}: largest |got - ref| / bound = {ratio:.3f}  (largest relative error {float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))):.2e})')
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    assert ok, (what, ratio, got, ref)


@pytest.fixture(scope='module')
def bare_engine():
    """A handle without weights: the loss needs none."""
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize('name', list(lr.CASES))
def test_loss_matches_the_float64_restatement(name, bare_engine):
    inputs, loss_kw = lr.case(name)
    got = _run(bare_engine, inputs, loss_kw)
    assert isinstance(got, np.ndarray) and np.isfinite(got).all()
    _check(got, lr.reference(inputs, loss_kw), name)
    if name == 'three_rows':                                     # the all-gate-1 row: divide_no_nan, exactly 0
        assert np.all(got[1:3, 2] == 0) and got[0, 2] == got[3, 2] > 0


def test_the_frame_limit(bare_engine):
    B, T = 8, 8192
    inputs = lr.make_inputs((T, T - 1, 4097, 4096, 33, 32, 2, 1), T, seed=8192)
    got = _run(bare_engine, inputs, {})
    _check(got, lr.reference(inputs, {}), f'B = {B}, T = {T}')
    with pytest.raises(Exception, match='B\\*T too large'):
        bare_engine.tacotron2_loss(*(np.zeros((9, T) + ((80,) if k in (0, 2, 3) else ()), np.float32) for k in range(5)))


def test_bit_for_bit_twice_alone_and_on_a_stream(bare_engine):
    import torch
    inputs, loss_kw = lr.case('two_chunks_plus_1')
    first = _run(bare_engine, inputs, loss_kw)
    assert np.array_equal(first, _run(bare_engine, inputs, loss_kw))                          # the same call twice
    wide = lr.make_inputs((65, 64, 33, 32, 31, 2, 1), 65, seed=77)                            # a row in a batch = that row alone, same T
    batch = _run(bare_engine, wide, loss_kw)
    for b in range(7):
        alone = _run(bare_engine, {k: wide[k][b:b + 1] for k in NAMES}, loss_kw)
        assert np.array_equal(alone[:, 0], batch[:, b]), b
    stream = torch.cuda.Stream()                                                              # numpy in = CUDA tensors in, on a stream
    dev = {k: torch.as_tensor(inputs[k]).cuda() for k in NAMES}
    torch.cuda.synchronize()
    got = _run(bare_engine, dev, loss_kw, stream=stream)
    assert got.is_cuda and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), first)
    mixed = _run(bare_engine, dict(dev, mel_target=inputs['mel_target'], gate_target=inputs['gate_target']), loss_kw)
    assert mixed.is_cuda and np.array_equal(mixed.cpu().numpy(), first)
    with pytest.raises(ValueError, match='stream= needs device tensors'):
        _run(bare_engine, inputs, loss_kw, stream=stream)


def test_forward_outputs_go_into_the_loss_on_the_device(gpu_engine):
    """The chain: tacotron2_forward on CUDA tensors, tacotron2_loss on its outputs where they are, on the caller's stream."""
    import torch
    from text_to_speech_amd.losses import TacotronLoss
    from text_to_speech_amd.tacotron2 import shift_mel_target
    g = np.load(os.path.join(GOLD, 'oracle_tacotron2_small.npz'))
    tok, lengths = g['tokens'], np.asarray([14, 9], np.int32)
    target = np.full((2, 14, 80), lr.PAD, np.float32)
    gate = np.ones((2, 14), np.float32)
    mel_input = np.full((2, 14, 80), lr.PAD, np.float32)
    for b, n in enumerate(lengths):
        target[b, :n], mel_input[b, :n], gate[b, :n - 1] = g['mel'][b, :n], shift_mel_target(g['mel'][b, :n]), 0.
    stream = torch.cuda.Stream()
    out = gpu_engine.tacotron2_forward(torch.as_tensor(tok).cuda(), torch.as_tensor(mel_input).cuda(), lengths, stream=stream)
    assert out.mel.is_cuda and out.stop_tokens.is_cuda
    loss = TacotronLoss(mel_loss=['mse', 'weighted_mae'], finish_weight=5.)
    got = loss([torch.as_tensor(target).cuda(), torch.as_tensor(gate).cuda()], out, engine=gpu_engine, stream=stream)
    assert got.is_cuda and tuple(got.shape) == (6, 2)
    ref = lr.tacotron_loss(target, gate, *(getattr(out, k).cpu().numpy() for k in ('decoder_output', 'mel', 'stop_tokens')),
                           mel_loss_kinds=['mse', 'weighted_mae'], finish_weight=5.)
    _check(got.cpu().numpy(), ref, 'forward -> loss')
    assert np.all(ref[1:5] > 0)                                  # an untrained model on a real target: a loss worth the name


def test_evaluate_equals_the_restatement_item_by_item(gpu_engine):
    """Four items, batch_size 3: every column of per_item is the restatement of its item's row in the batch it ran in."""
    from text_to_speech_amd.losses import TacotronLoss
    from text_to_speech_amd.runtime import HipRuntime
    from text_to_speech_amd.tacotron2 import Tacotron2, shift_mel_target
    rt = HipRuntime('synthetic', model='tacotron2', engine=gpu_engine, seed=3)
    model = Tacotron2(rt, lang='en')
    model.pad_mel_value = lr.PAD
    rng = np.random.default_rng(11)
    texts = ['Hello, World!', 'Hi there', 'The quick brown fox.', 'Bye']
    mels = [rng.uniform(-9, 1, (n, 80)).astype(np.float32) for n in (21, 34, 7, 12)]
    loss = TacotronLoss(mel_loss=['mse', 'mae'], not_finish_weight=0.5)
    res = model.evaluate(list(zip(texts, mels)), batch_size=3, loss=loss)
    assert res['names'] == loss.output_names and res['per_item'].shape == (6, 4)
    toks = [np.asarray(model.encode_text(model.clean_text(t), cleaned=True), np.int32) for t in texts]
    for rows in ((0, 1, 2), (3,)):                               # teacher_forced-style outputs of the same batches
        B, T, Tin = len(rows), max(len(mels[i]) for i in rows), max(len(toks[i]) for i in rows)
        tok = np.zeros((B, Tin), np.int32)
        target, mel_input = np.full((B, T, 80), lr.PAD, np.float32), np.full((B, T, 80), lr.PAD, np.float32)
        gate = np.ones((B, T), np.float32)
        for r, i in enumerate(rows):
            n = len(mels[i])
            tok[r, :len(toks[i])], target[r, :n], mel_input[r, :n], gate[r, :n - 1] = toks[i], mels[i], shift_mel_target(mels[i]), 0.
        out = rt.tacotron2_forward(tok, mel_input, np.asarray([len(mels[i]) for i in rows], np.int32), deterministic=True,
                                   on_device=True)
        ref = lr.tacotron_loss(target, gate, *(getattr(out, k).cpu().numpy() for k in ('decoder_output', 'mel', 'stop_tokens')),
                               mel_loss_kinds=['mse', 'mae'], not_finish_weight=0.5)
        _check(res['per_item'][:, rows[0]:rows[-1] + 1], ref, f'evaluate rows {rows}')
    for k, name in enumerate(res['names']):
        assert res['mean'][name] == pytest.approx(float(res['per_item'][k].astype(np.float64).mean()), rel=1e-12)


def test_symbol_is_exported_and_refuses_through_the_handle(bare_engine):
    from text_to_speech_amd import _lib
    lib = _lib.load_library()
    assert hasattr(lib, 'tts_hip_tacotron2_loss') and 'tts_hip_tacotron2_loss' in _lib.SIGNATURES
    assert lib.tts_hip_tacotron2_loss(None, None, None, None, None, None, 1, 1, None, 1, 1, 0, 1.0, 1.0, None, 0, None) == -1
    inputs, _ = lr.case('one_frame')
    with pytest.raises(Exception, match='tacotron2_loss: finish_weight = -1 must be finite and not negative'):
        _run(bare_engine, inputs, dict(finish_weight=-1.))
    kinds = np.asarray([0, 0], np.int32)
    out = np.zeros((6, 1), np.float32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.tts_hip_tacotron2_loss(bare_engine._h, *(ptr(inputs[k]) for k in NAMES), 1, 1, ptr(kinds), 2, 1, 0, 1.0, 1.0, ptr(out), 0, None)
    assert rc == -1 and lib.tts_hip_last_error(bare_engine._h) == b'tacotron2_loss: kinds[1] repeats kinds[0] = 0'
    with pytest.raises(ValueError, match='similarity'):
        _run(bare_engine, inputs, dict(mel_loss_kinds='similarity'))
