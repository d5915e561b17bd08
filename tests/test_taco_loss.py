"""CPU: the TacotronLoss evaluation path without a GPU.

1. tests/taco_loss_ref.py (the float64 restatement every GPU result is held to) against closed forms and against
   torch.nn.functional on the CPU.
2. `losses.TacotronLoss`: output_names and get_config keys as the reference's (custom_train_objects/losses/tacotron_loss.py:
   52-60, 169-179 on top of keras.losses.Loss.get_config: name, reduction), the kinds it refuses.
3. The front end of tts_hip_tacotron2_loss in C++ (csrc/taco_loss_call.h) against a Python restatement written here, refusal by
   refusal and on random calls.  The C++ side is csrc/host_check.cpp's --taco-loss mode, built with -fsanitize=address,undefined.
4. `Tacotron2.evaluate` on a recording fake runtime: what it prepares, pads, batches and returns.
5. The GPU bound (taco_loss_ref.RTOL / ATOL) lies at least a factor ten below the effect of every planted mistake on the GPU
   test's own cases.
"""
import os
import re
import shutil
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import taco_loss_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
EINVAL = -1
NAMES = ('mel_target', 'gate_target', 'decoder_output', 'mel', 'stop_tokens')


# ---- 1. the restatement --------------------------------------------------------------------------------------------------------
def test_restatement_closed_forms():
    B, T = 3, 7
    y = np.random.default_rng(0).uniform(-9, 1, (B, T, 80))
    g = np.zeros((B, T))
    g[:, -1] = 1
    half = np.full((B, T), 0.5)
    for c in (0.5, -2.0):                                        # a constant error c: mse c^2, mae |c|, whatever the mask keeps
        out = lr.tacotron_loss(y, g, y - c, y + c, half, mel_loss_kinds=['mse', 'mae'])
        assert np.allclose(out[1], c * c, rtol=1e-12) and np.allclose(out[3], c * c, rtol=1e-12)
        assert np.allclose(out[2], abs(c), rtol=1e-12) and np.allclose(out[4], abs(c), rtol=1e-12)
        assert np.allclose(out[5], np.log(2), rtol=1e-12)        # o = 0.5, weights 1
        assert np.allclose(out[0], out[1:].sum(axis=0), rtol=1e-12)
    # an all-gate-1 row: the mask is zero everywhere, divide_no_nan gives 0; the gate loss is still there
    g1 = g.copy()
    g1[1] = 1
    out = lr.tacotron_loss(y, g1, y - 3, y + 3, half, mel_loss_kinds=lr.ALL_KINDS)
    assert np.all(out[1:9, 1] == 0) and np.all(out[1:9, 0] > 0) and out[0, 1] == out[9, 1] > 0
    # gate loss at o = 0.5: ln 2 times the mean weight, over the padded length
    out = lr.tacotron_loss(y, g, y, y, half, finish_weight=5., not_finish_weight=0.5)
    assert np.allclose(out[3], np.log(2) * (5. + 0.5 * (T - 1)) / T, rtol=1e-12) and np.all(out[1:3] == 0)
    # the mask is 1 - gate: it drops the last real frame, and the mean runs over the kept spectrogram, not over frames
    d = y.copy()
    d[:, -1] += 100.0
    assert np.all(lr.tacotron_loss(y, g, d, y, half)[1] == 0)
    d = y.copy()
    d[:, 0, 0] += 4.0
    assert np.allclose(lr.tacotron_loss(y, g, d, y, half)[1], 16.0 / ((T - 1) * 80), rtol=1e-12)
    assert np.allclose(lr.tacotron_loss(y, g, d, y, half, mask_mel_padding=False)[1], 16.0 / (T * 80), rtol=1e-12)
    # a soft target weighs its frame: 0.25 -> mask 0.75
    gs = np.full((B, T), 0.25)
    assert np.allclose(lr.tacotron_loss(y, gs, y - 2, y, half)[1], 4.0, rtol=1e-12)
    # weighted kinds: w = (y - ymin + 1) / (ymax - ymin + 1), extrema over the padded row; at the row's maximum w = 1
    yw = np.zeros((1, 2, 80))
    yw[0, 1] = -11.0                                             # the padded frame holds the minimum
    gw = np.array([[0.0, 1.0]])
    out = lr.tacotron_loss(yw, gw, yw - 2, yw, np.full((1, 2), 0.5), mel_loss_kinds=['weighted_mse', 'weighted_mae'])
    assert np.allclose(out[1], 4.0, rtol=1e-12) and np.allclose(out[2], 2.0, rtol=1e-12)
    yw[0, 0, :40] = -5.0                                         # w = 7 / 12 on half of the kept frame
    out = lr.tacotron_loss(yw, gw, yw - 2, yw, np.full((1, 2), 0.5), mel_loss_kinds=['weighted_mse'])
    assert np.allclose(out[1], 4.0 * (1 + 7 / 12) / 2, rtol=1e-12)
    # the clip: probabilities of exactly 0 and 1 give finite values, -log(float32(1e-7)) where they are wrong
    x = np.array([[0.0, 1.0]])
    out = lr.tacotron_loss(yw, np.array([[1.0, 0.0]]), yw, yw, x)
    assert np.isfinite(out).all() and np.allclose(out[3], (-np.log(np.float64(np.float32(1e-7))) - np.log(1 - np.float64(lr.CLIP_HI))) / 2)
    assert lr.output_names('mse') == ['loss', 'mse_mel_loss', 'mse_mel_postnet_loss', 'gate_loss']


def test_restatement_against_torch_functional():
    import torch
    import torch.nn.functional as F
    inputs, _ = lr.case('three_rows')
    y, g, d, p, x = (torch.as_tensor(inputs[k], dtype=torch.float64) for k in NAMES)
    lengths = inputs['lengths']
    out = lr.tacotron_loss(*(inputs[k] for k in NAMES), mel_loss_kinds=['mse', 'mae'], mask_mel_padding=False)
    for row, (fn, pred) in enumerate(((F.mse_loss, d), (F.l1_loss, d), (F.mse_loss, p), (F.l1_loss, p)), start=1):
        want = torch.stack([fn(pred[b], y[b]) for b in range(len(lengths))]).numpy()
        assert np.allclose(out[row], want, rtol=1e-12, atol=0), row
    # masked: rows whose mask keeps frames 0 .. n - 2 are the unmasked loss of those frames
    out = lr.tacotron_loss(*(inputs[k] for k in NAMES), mel_loss_kinds=['mse', 'mae'])
    for b, n in enumerate(lengths):
        want = [float(fn(pred[b, :n - 1], y[b, :n - 1])) if n > 1 else 0.0
                for fn, pred in ((F.mse_loss, d), (F.l1_loss, d), (F.mse_loss, p), (F.l1_loss, p))]
        assert np.allclose(out[1:5, b], want, rtol=1e-12, atol=0), b
    # the gate loss: binary_cross_entropy on the clipped values with the per-frame weights, mean over the padded T
    w = g * 5.0 + (1 - g) * 0.5
    lo, hi = float(lr.CLIP_LO), float(lr.CLIP_HI)
    for probs in (x, torch.as_tensor(lr.case('stop_edges')[0]['stop_tokens'], dtype=torch.float64)):
        got = lr.tacotron_loss(y, g, d, p, probs, finish_weight=5., not_finish_weight=0.5)[3]
        want = (F.binary_cross_entropy(probs.clamp(lo, hi), g, reduction='none') * w).mean(dim=1).numpy()
        assert np.isfinite(got).all() and np.allclose(got, want, rtol=1e-12, atol=0)
    for logits in (torch.logit(x), torch.as_tensor(lr.case('logits')[0]['stop_tokens'], dtype=torch.float64)):
        got = lr.tacotron_loss(y, g, d, p, logits, from_logits=True, finish_weight=5., not_finish_weight=0.5)[3]
        want = (F.binary_cross_entropy_with_logits(logits, g, reduction='none') * w).mean(dim=1).numpy()
        assert np.isfinite(got).all() and np.allclose(got, want, rtol=1e-12, atol=1e-300)


# ---- 2. the loss object --------------------------------------------------------------------------------------------------------
# keras.losses.Loss.get_config gives name and reduction; TacotronLoss.get_config (tacotron_loss.py:169-179) adds the other six
REFERENCE_CONFIG_KEYS = {'name', 'reduction', 'mask_mel_padding', 'label_smoothing', 'finish_weight', 'not_finish_weight',
                         'from_logits', 'mel_loss'}


def test_loss_object_names_config_and_refusals():
    from text_to_speech_amd.losses import MEL_LOSS_KINDS, TacotronLoss, loss_output_names
    one = TacotronLoss()
    assert one.output_names == ['loss', 'mse_mel_loss', 'mse_mel_postnet_loss', 'gate_loss'] == lr.output_names('mse')
    kinds = ['mae', 'weighted_mse']
    many = TacotronLoss(mel_loss=kinds, from_logits=True, label_smoothing=0.1, finish_weight=5., not_finish_weight=0.5,
                        mask_mel_padding=False)
    assert many.output_names == ['loss', 'mae_mel_loss', 'weighted_mse_mel_loss', 'mae_mel_postnet_loss',
                                 'weighted_mse_mel_postnet_loss', 'gate_loss'] == lr.output_names(kinds) == loss_output_names(kinds)
    assert tuple(MEL_LOSS_KINDS) == lr.KINDS and list(MEL_LOSS_KINDS.values()) == [0, 1, 2, 3]
    for loss in (one, many):
        cfg = loss.get_config()
        assert set(cfg) == REFERENCE_CONFIG_KEYS
        again = TacotronLoss.from_config(cfg)
        assert again.get_config() == cfg and again.output_names == loss.output_names
    assert one.get_config() == dict(name='tacotron_loss', reduction='sum_over_batch_size', mask_mel_padding=True, label_smoothing=0,
                                    finish_weight=1., not_finish_weight=1., from_logits=False, mel_loss='mse')
    assert many.get_config()['mel_loss'] == kinds and many.get_config()['label_smoothing'] == 0.1
    for bad, needle in (('similarity', 'similarity'), (['mse', 'similarity'], 'similarity'), (np.square, 'callable'),
                        ('huber', "unknown mel_loss 'huber'"), ([], '1 to 4'), (['mse', 'mae', 'mse'], 'twice'),
                        (['mse', 'mae', 'weighted_mse', 'weighted_mae', 'mse'], '1 to 4')):
        with pytest.raises(ValueError, match=needle):
            TacotronLoss(mel_loss=bad)
    with pytest.raises(ValueError, match='engine='):
        one([np.zeros((1, 2, 80)), np.zeros((1, 2))], [np.zeros((1, 2, 80))] * 2 + [np.zeros((1, 2))])


def test_loss_object_hands_its_settings_to_the_engine():
    from text_to_speech_amd.losses import TacotronLoss
    seen = []

    class Engine:
        def tacotron2_loss(self, *args, **kw):
            seen.append((args, kw))
            return 'result'

    Out = namedtuple('Out', ['decoder_output', 'mel', 'stop_tokens', 'attention_weights'])
    loss = TacotronLoss(mel_loss=['mae', 'mse'], from_logits=True, finish_weight=2., not_finish_weight=3., mask_mel_padding=False,
                        label_smoothing=0.3)
    assert loss(['y', 'g'], Out('d', 'p', 'x', 'a'), engine=Engine()) == 'result'
    assert seen == [(('y', 'g', 'd', 'p', 'x'), dict(mel_loss=['mae', 'mse'], mask_mel_padding=False, from_logits=True,
                                                     finish_weight=2., not_finish_weight=3.))]


# ---- 3. the call's front end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    return os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')


def _call(exe, *args):
    """-> (status, message, [K, chunks, weighted, workspace bytes] or None)"""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, '--taco-loss'] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    rc, _, msg = lines[0].partition(' ')
    return int(rc), msg, [int(v) for v in lines[1].split()] if len(lines) > 1 else None


C_NAMES = dict(target='mel_target', gate='gate_target', dec='decoder_output', mel='mel', stop='stop_tokens', kinds='kinds', out='out')


def loss_check(s, kinds):
    """taco_loss_check restated: s = dict(B, T, mem, n_kinds, fw, nfw, null, odd) -> (status, message)."""
    for short, name in C_NAMES.items():
        if short in s['null']:
            return EINVAL, f'{name} is NULL'
    if s['B'] < 1:
        return EINVAL, f"B = {s['B']} must be at least 1"
    if s['T'] < 1:
        return EINVAL, f"T = {s['T']} must be at least 1"
    if s['B'] * s['T'] > 65536:
        return EINVAL, f"B*T too large (B = {s['B']}, T = {s['T']}: above 65536 frames); split the batch"
    if not 1 <= s['n_kinds'] <= 4:
        return EINVAL, f"n_kinds = {s['n_kinds']} is outside [1, 4]"
    kinds = (list(kinds) + [0] * 4)[:s['n_kinds']]
    for i, k in enumerate(kinds):
        if not 0 <= k < 4:
            return EINVAL, f'kinds[{i}] = {k} is no mel loss (0 mse, 1 mae, 2 weighted_mse, 3 weighted_mae)'
        if k in kinds[:i]:
            return EINVAL, f'kinds[{i}] repeats kinds[{kinds.index(k)}] = {k}'
    if s['mem'] not in (0, 1):
        return EINVAL, f"bad mem kind {s['mem']}"
    for key, name in (('fw', 'finish_weight'), ('nfw', 'not_finish_weight')):
        if not np.isfinite(s[key]) or s[key] < 0:
            return EINVAL, f'{name} = {s[key]:g} must be finite and not negative'
    if s['mem'] == 1:
        for short in ('target', 'dec', 'mel'):
            if short in s['odd']:
                return EINVAL, f'{C_NAMES[short]} is not 16-byte aligned'
    return 0, ''


def loss_layout(s, kinds):
    """taco_loss_layout restated -> [K, chunks, weighted, bytes]"""
    al = lambda n: (n + 255) // 256 * 256
    B, T, n = s['B'], s['T'], s['n_kinds']
    chunks = (T + lr.CHUNK - 1) // lr.CHUNK
    weighted = int(any(k >= 2 for k in kinds[:n]))
    K = 2 + 2 * n
    staged = 3 * al(B * T * 80 * 4) + 2 * al(B * T * 4) if s['mem'] == 0 else 0
    return [K, chunks, weighted, staged + al(B * chunks * 2 * 4 * weighted) + al(B * chunks * 10 * 8) + al(K * B * 4)]


def _args(s, kinds):
    out = [f'{k}={v}' for k, v in s.items() if k not in ('null', 'odd', 'n_kinds')]
    out += [f'{k}={s[k]}' for k in ('null', 'odd') if s[k]]
    if s['n_kinds'] != len(kinds):
        out.append(f"n_kinds={s['n_kinds']}")
    return out + list(kinds)


GOOD = dict(B=3, T=33, mem=0, fw=1.0, nfw=1.0, null='', odd='')


def test_front_end_refuses_by_name_before_any_gpu_work(checker):
    refusals = [
        (dict(null='target'), [0], 'mel_target is NULL'), (dict(null='gate'), [0], 'gate_target is NULL'),
        (dict(null='dec'), [0], 'decoder_output is NULL'), (dict(null='mel'), [0], 'mel is NULL'),
        (dict(null='stop'), [0], 'stop_tokens is NULL'), (dict(null='kinds'), [0], 'kinds is NULL'), (dict(null='out'), [0], 'out is NULL'),
        (dict(B=0), [0], 'B = 0 must be at least 1'), (dict(B=-4), [0], 'B = -4 must be at least 1'),
        (dict(T=0), [0], 'T = 0 must be at least 1'), (dict(T=-1), [0], 'T = -1 must be at least 1'),
        (dict(B=1, T=65537), [0], 'B*T too large (B = 1, T = 65537: above 65536 frames); split the batch'),
        (dict(B=8, T=8193), [0], 'B*T too large (B = 8, T = 8193: above 65536 frames); split the batch'),
        (dict(B=2147483647, T=2147483647), [0], 'B*T too large (B = 2147483647, T = 2147483647: above 65536 frames); split the batch'),
        (dict(), [], 'n_kinds = 0 is outside [1, 4]'), (dict(), [0, 1, 2, 3, 0], 'n_kinds = 5 is outside [1, 4]'),
        (dict(), [4], 'kinds[0] = 4 is no mel loss (0 mse, 1 mae, 2 weighted_mse, 3 weighted_mae)'),
        (dict(), [0, -1], 'kinds[1] = -1 is no mel loss (0 mse, 1 mae, 2 weighted_mse, 3 weighted_mae)'),
        (dict(), [2, 0, 2], 'kinds[2] repeats kinds[0] = 2'), (dict(), [1, 1], 'kinds[1] repeats kinds[0] = 1'),
        (dict(mem=7), [0], 'bad mem kind 7'), (dict(mem=-1), [0], 'bad mem kind -1'),
        (dict(fw='nan'), [0], 'finish_weight = nan must be finite and not negative'),
        (dict(fw='inf'), [0], 'finish_weight = inf must be finite and not negative'),
        (dict(fw=-0.5), [0], 'finish_weight = -0.5 must be finite and not negative'),
        (dict(nfw='nan'), [0], 'not_finish_weight = nan must be finite and not negative'),
        (dict(nfw=-2), [0], 'not_finish_weight = -2 must be finite and not negative'),
        (dict(mem=1, odd='target'), [0], 'mel_target is not 16-byte aligned'),
        (dict(mem=1, odd='dec'), [0], 'decoder_output is not 16-byte aligned'), (dict(mem=1, odd='mel'), [0], 'mel is not 16-byte aligned'),
        # first match wins, in the documented order
        (dict(null='out,gate', B=0), [9], 'gate_target is NULL'), (dict(B=0, T=0, mem=5), [], 'B = 0 must be at least 1'),
        (dict(T=65537, mem=5), [9], 'B*T too large (B = 3, T = 65537: above 65536 frames); split the batch'),
        (dict(mem=5, fw=-1), [0, 0], 'kinds[1] repeats kinds[0] = 0'), (dict(mem=5, fw=-1), [0], 'bad mem kind 5'),
        (dict(mem=1, fw=-1, nfw=-1, odd='mel'), [0], 'finish_weight = -1 must be finite and not negative'),
    ]
    for wrong, kinds, msg in refusals:
        rc, why, layout = _call(checker, *_args(dict(GOOD, n_kinds=len(kinds), **wrong), kinds))
        assert (rc, why, layout) == (EINVAL, 'who: ' + msg, None), (wrong, kinds, rc, why)


def test_front_end_accepts_and_sizes_at_the_limits(checker):
    for s, kinds in [
        (dict(B=1, T=1), [0]), (dict(B=3, T=33), [0, 1, 2, 3]), (dict(B=8, T=8192), [0]), (dict(B=1, T=65536), [3]),
        (dict(B=65536, T=1, mem=1), [1, 2]), (dict(B=8, T=800, mem=1), [0]), (dict(B=2, T=32, fw=0, nfw=0), [2]),
        (dict(B=2, T=31, mem=0, odd='target,dec,mel'), [0]),         # host arrays are staged: any alignment
        (dict(B=2, T=64, mem=1, odd='gate,stop,out'), [0]),          # the [B, T] arrays are read float by float
    ]:
        s = dict(GOOD, n_kinds=len(kinds), **s)
        assert _call(checker, *_args(s, kinds)) == (0, '', loss_layout(s, kinds)), (s, kinds)
    assert loss_layout(dict(B=8, T=800, mem=1, n_kinds=1), [0]) == [4, 50, 0, 8 * 50 * 10 * 8 + 256]


def test_front_end_equals_its_restatement_on_random_calls(checker):
    rng = np.random.default_rng(21)
    pick = lambda *pool: pool[int(rng.integers(len(pool)))]
    seen = set()
    for _ in range(300):
        kinds = [int(pick(0, 1, 2, 3, 3, 2, 1, 0, 4, -1)) for _ in range(int(pick(1, 1, 2, 3, 4, 4, 0, 5)))]
        s = dict(B=pick(3, 3, 1, 8, 0, -1, 65536), T=pick(33, 33, 1, 32, 8192, 0, -2, 65536, 21846), mem=pick(0, 1, 1, 7, -1),
                 fw=pick(1.0, 1.0, 5.0, 0.0, -1.0, 'nan', 'inf'), nfw=pick(1.0, 1.0, 0.5, 0.0, -0.25, 'nan', '-inf'),
                 null=','.join(n for n in C_NAMES if rng.random() < 0.04), odd=','.join(n for n in C_NAMES if rng.random() < 0.1),
                 n_kinds=len(kinds) if rng.random() < 0.9 else int(pick(0, 1, 4, 5, -1)))
        want = loss_check(dict(s, fw=float(s['fw']), nfw=float(s['nfw'])), kinds)
        rc, why, layout = _call(checker, *_args(s, kinds))
        assert (rc, why) == (want[0], 'who: ' + want[1] if want[0] else ''), (s, kinds, rc, why)
        assert layout == (loss_layout(s, (kinds + [0] * 4)) if rc == 0 else None), (s, kinds)
        seen.add(re.sub(r'-?\d+(\.\d+)?', '#', why))
    assert '' in seen and len(seen) >= 10, sorted(seen)


# ---- 4. Tacotron2.evaluate on a recording runtime -------------------------------------------------------------------------------
class _FakeRuntime:
    """Stands for HipRuntime: records both calls; the forward pass answers with values derived from its input, the loss with the
    float64 restatement."""
    Out = namedtuple('Out', ['decoder_output', 'mel', 'stop_tokens', 'attention_weights'])

    def __init__(self):
        self.forwards, self.losses = [], []

    def tacotron2_forward(self, inputs, mel_input, mel_lengths, **kwargs):
        self.forwards.append((inputs, mel_input, mel_lengths, kwargs))
        tokens = inputs[0] if isinstance(inputs, tuple) else inputs
        B, T = mel_input.shape[:2]
        stop = (0.1 + 0.8 * (np.arange(B * T).reshape(B, T) % 7) / 7).astype(np.float32)
        return self.Out(mel_input * np.float32(0.5), mel_input * np.float32(0.75) - np.float32(0.1), stop,
                        np.zeros((B, T, tokens.shape[1]), np.float32))

    def tacotron2_loss(self, mel_target, gate_target, decoder_output, mel, stop_tokens, **kw):
        self.losses.append((mel_target, gate_target, decoder_output, mel, stop_tokens, dict(kw)))
        return lr.tacotron_loss(mel_target, gate_target, decoder_output, mel, stop_tokens, mel_loss_kinds=kw.pop('mel_loss'),
                                **kw).astype(np.float32)


def test_evaluate_prepares_pads_batches_and_reports():
    from text_to_speech_amd.losses import TacotronLoss
    from text_to_speech_amd.tacotron2 import SV2TTSTacotron2, Tacotron2, shift_mel_target
    rng = np.random.default_rng(5)
    texts = ['Hello, World!', 'Hi', 'A somewhat longer sentence.', 'Good morning', 'Bye']
    mels = [rng.uniform(-8, 1, (n, 80)).astype(np.float32) for n in (9, 4, 12, 1, 6)]
    rt = _FakeRuntime()
    model = Tacotron2(rt, lang='en')
    model.pad_mel_value = -11.
    res = model.evaluate(list(zip(texts, mels)), batch_size=2, loss=TacotronLoss(mel_loss=['mae', 'weighted_mse'], finish_weight=5.))
    blank = model.tokenizer.blank_token_idx
    toks = [np.asarray(model.encode_text(model.clean_text(t), cleaned=True), np.int32) for t in texts]
    assert [f[1].shape[0] for f in rt.forwards] == [2, 2, 1] and len(rt.losses) == 3          # batch boundaries, in input order
    for call, (inputs, mel_input, mel_lengths, kwargs) in enumerate(rt.forwards):
        rows = range(2 * call, min(2 * call + 2, 5))
        T, Tin = max(len(mels[i]) for i in rows), max(len(toks[i]) for i in rows)
        assert inputs.shape == (len(rows), Tin) and inputs.dtype == np.int32 and mel_input.shape == (len(rows), T, 80)
        assert mel_lengths.tolist() == [len(mels[i]) for i in rows] and kwargs == {'deterministic': True, 'on_device': True}
        target, gate, dec, post, stop, kw = rt.losses[call]
        assert kw == dict(mel_loss=['mae', 'weighted_mse'], mask_mel_padding=True, from_logits=False, finish_weight=5.,
                          not_finish_weight=1.)
        for r, i in enumerate(rows):
            n = len(mels[i])
            assert np.array_equal(inputs[r, :len(toks[i])], toks[i]) and np.all(inputs[r, len(toks[i]):] == blank)
            assert np.array_equal(mel_input[r, :n], shift_mel_target(mels[i])) and np.all(mel_input[r, n:] == -11.)
            assert np.all(mel_input[r, 0] == 0)                                            # the go frame
            assert np.array_equal(target[r, :n], mels[i]) and np.all(target[r, n:] == -11.)
            assert gate[r].tolist() == [0.] * (n - 1) + [1.] * (T - n + 1)                     # zeros, a final 1, padded with 1
        assert target.dtype == gate.dtype == np.float32
        assert np.array_equal(dec, mel_input * np.float32(0.5)) and np.array_equal(post, mel_input * np.float32(0.75) - np.float32(0.1))
    names = res['names']
    assert names == lr.output_names(['mae', 'weighted_mse']) and res['per_item'].shape == (6, 5) and res['per_item'].dtype == np.float32
    for call in range(3):                                        # every column is its item's, where its item was in the input
        target, gate, dec, post, stop, kw = rt.losses[call]
        want = lr.tacotron_loss(target, gate, dec, post, stop, mel_loss_kinds=['mae', 'weighted_mse'], finish_weight=5.)
        assert np.array_equal(res['per_item'][:, 2 * call:2 * call + 2], want.astype(np.float32))
    assert np.all(res['per_item'][1:5, 3] == 0) and res['per_item'][5, 3] > 0                  # the one-frame item: all masked
    assert set(res['mean']) == set(names)
    for k, name in enumerate(names):
        assert isinstance(res['mean'][name], float) and res['mean'][name] == pytest.approx(float(res['per_item'][k].astype(np.float64).mean()), rel=1e-12)
    # defaults: batches of 8, TacotronLoss(), the model's own padding value; deterministic passes through
    rt.forwards.clear(), rt.losses.clear()
    plain = Tacotron2(rt, lang='en')
    out = plain.evaluate(list(zip(texts, mels)), deterministic=False)
    assert out['names'] == lr.output_names('mse') and out['per_item'].shape == (4, 5) and len(rt.forwards) == 1
    assert rt.forwards[0][3] == {'deterministic': False, 'on_device': True} and np.all(rt.forwards[0][1][1, 4:] == 0.)
    assert rt.losses[0][5]['mel_loss'] == 'mse'
    # refusals: a text that encodes to no token is named by its index; an empty list; a runtime without the two calls
    with pytest.raises(ValueError, match=r'items\[1\]: the text encodes to no token'):
        model.evaluate([(texts[0], mels[0]), ('', mels[1])])
    with pytest.raises(ValueError, match='at least one item'):
        model.evaluate([])
    with pytest.raises(ValueError, match='batch_size'):
        model.evaluate([(texts[0], mels[0])], batch_size=0)
    with pytest.raises(ValueError, match=r'items\[0\] must be a'):
        model.evaluate([texts[0]])
    with pytest.raises(ValueError, match='tacotron2_loss'):
        Tacotron2(object(), lang='en').evaluate([(texts[0], mels[0])])
    # the speaker of an SV2TTS model rides along as for infer: one row of it per batch row
    spk = rng.standard_normal((3, 256)).astype(np.float32)
    rt.forwards.clear()
    SV2TTSTacotron2(rt, lang='en', embeddings=spk).evaluate(list(zip(texts[:3], mels[:3])), batch_size=2, embeddings=2)
    for (tokens, emb), *_ in rt.forwards:
        assert emb.shape == (tokens.shape[0], 256) and np.all(emb == spk[2])


# ---- 5. the GPU bound against planted mistakes ----------------------------------------------------------------------------------
CAUGHT_BY = {'gate mean over the row length': 'three_rows', 'mask keeps the last real frame': 'three_rows',
             'mean over frames': 'three_rows', 'row extrema over real frames': 'weighted_mse', 'missing clip': 'stop_edges',
             'swapped finish weights': 'weights_5_half'}


@pytest.mark.parametrize('mistake', lr.MISTAKES)
def test_gpu_bound_is_a_tenth_of_every_planted_mistake(mistake):
    inputs, loss_kw = lr.case(CAUGHT_BY[mistake])
    ref = lr.reference(inputs, loss_kw)
    wrong = lr.reference(inputs, loss_kw, mistake=mistake, lengths=inputs['lengths'])
    assert np.isfinite(ref).all() and lr.within(ref, ref) == (True, 0.0)
    with np.errstate(invalid='ignore'):
        effect = np.where(np.isfinite(wrong), np.abs(wrong - ref), np.inf) / (lr.RTOL * np.abs(ref) + lr.ATOL)
    print(f'{mistake}: largest effect / bound = {effect.max():.3g}')
    assert effect.max() >= 10.0, (mistake, effect.max())
    assert not lr.within(wrong, ref)[0]
    # and every case sees at least the mistakes its settings can show: none of them hides inside the bound by luck
    assert set(CAUGHT_BY) == set(lr.MISTAKES) and set(CAUGHT_BY.values()) <= set(lr.CASES)


def test_cases_are_finite_and_cover_the_chunk_edges():
    Ts = {lr.CASES[n][1] for n in lr.CASES}
    assert {1, lr.CHUNK - 1, lr.CHUNK, lr.CHUNK + 1, 2 * lr.CHUNK + 1, lr.FINISH_TILE * lr.CHUNK, lr.FINISH_TILE * lr.CHUNK + 1} <= Ts
    for name in lr.CASES:
        inputs, loss_kw = lr.case(name)
        assert all(np.isfinite(inputs[k]).all() and inputs[k].dtype == np.float32 for k in NAMES), name
        ref = lr.reference(inputs, loss_kw)
        assert np.isfinite(ref).all() and ref.shape == (len(lr.output_names(loss_kw.get('mel_loss_kinds', 'mse'))), len(inputs['lengths']))
    inputs, loss_kw = lr.case('three_rows')
    assert np.all(inputs['gate_target'][2] == 1) and np.all(lr.reference(inputs, loss_kw)[1:3, 2] == 0)       # all-zero mask
