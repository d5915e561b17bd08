"""CPU: the front end of every Tacotron2 call in C++ (csrc/taco_call.h: taco_encode_check and taco_run_check, the only places
such a call is refused for what it asks, and the buffer sizes of the teacher-forced pass, as pure host code) against the
rows of tests/taco_call_cases.py and a Python restatement written here.  The C++ side is csrc/host_check.cpp's --taco-call mode,
built with -fsanitize=address,undefined like the weight-file loader (tests/test_host_sanitizer.py): `mel_lengths` is untrusted
input."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from taco_call_cases import B, EINVAL, ENOTREADY, LEN, REFUSALS, TIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')


@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    return os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')


def _call(exe, kind, *args):
    """-> (status, message, the taco_forward_sizes line or None)"""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, '--taco-call', kind] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    rc, _, msg = lines[0].partition(' ')
    return int(rc), msg, [int(v) for v in lines[1].split()] if len(lines) > 1 else None


def _front(exe, *args):
    return _call(exe, 'forward', *args)


def _sizes(B, T, enc):
    frames = B * T
    return [frames, frames * 80, frames * 256, frames * 4096, B * ((T + 255) // 256 * 256) * (1024 + enc), frames * 81]


# ---- the teacher-forced call ----------------------------------------------------------------------------------------------------
def test_front_end_refuses_by_name_before_any_gpu_work(checker):
    refusals = [
        (['T=4', 'precision=2', 4, 4], EINVAL, 'precision must be 0 (f32) or 1 (f16 weights), got 2'),
        (['T=4', 'precision=-1', 4], EINVAL, 'precision must be 0 (f32) or 1 (f16 weights), got -1'),
        (['T=4', 'mem=7', 4], EINVAL, 'bad mem kind 7'),
        (['T=4', 'ready=0', 4], ENOTREADY, 'tacotron2 weights not finalized'),
        (['T=4', 'null=encoded', 4], EINVAL, 'encoded batch is NULL or empty'),
        (['T=4', 'enc=768', 4], EINVAL, 'encoded batch belongs to other weights (width 768, model 512)'),
        (['T=4', 'null=mel', 4], EINVAL, 'mel_input or mel_lengths is NULL'),
        (['T=4', 'null=lens', 4], EINVAL, 'mel_input or mel_lengths is NULL'),
        (['T=0', 'B=1'], EINVAL, 'T = 0 must be at least 1'),
        (['T=-3', 'B=1'], EINVAL, 'T = -3 must be at least 1'),
        (['T=65537', 'B=1'], EINVAL, 'B*T too large (B = 1, T = 65537: above 65536 frames); split the batch'),
        (['T=8193', 'B=8'], EINVAL, 'B*T too large (B = 8, T = 8193: above 65536 frames); split the batch'),
        (['T=2147483647', 'B=1024'], EINVAL, 'B*T too large (B = 1024, T = 2147483647: above 65536 frames); split the batch'),
        (['T=4', 4, 0, 4], EINVAL, 'mel_lengths[1] = 0 is outside [1, T = 4]'),
        (['T=4', 4, 4, 5], EINVAL, 'mel_lengths[2] = 5 is outside [1, T = 4]'),
        (['T=4', -1], EINVAL, 'mel_lengths[0] = -1 is outside [1, T = 4]'),
        # first match wins: precision before everything, the frame limit before the lengths
        (['T=0', 'precision=3', 'ready=0', 'null=encoded,mel'], EINVAL, 'precision must be 0 (f32) or 1 (f16 weights), got 3'),
        (['T=65537', 'B=1', 'null=lens'], EINVAL, 'mel_input or mel_lengths is NULL'),
    ]
    for args, code, msg in refusals:
        rc, why, sizes = _front(checker, *args)
        assert (rc, why) == (code, 'who: ' + msg), (args, rc, why)
        assert sizes is None


def test_front_end_accepts_and_sizes_at_the_limits(checker):
    for args, (B, T, enc) in [
        (['T=1', 1], (1, 1, 512)),
        (['T=33', 33, 17, 1], (3, 33, 512)),
        (['T=256', 'B=2', 'precision=1', 'mem=1'], (2, 256, 512)),
        (['T=257', 'B=2', 'enc=768', 'model_enc=768'], (2, 257, 768)),
        (['T=65536', 'B=1'], (1, 65536, 512)),                       # the frame limit itself: G = 1 GiB
        (['T=8192', 'B=8', 'enc=768', 'model_enc=768'], (8, 8192, 768)),
        (['T=64', 'B=1024'], (1024, 64, 512)),
    ]:
        rc, why, sizes = _front(checker, *args)
        assert (rc, why) == (0, ''), (args, rc, why)
        assert sizes == _sizes(B, T, enc), args
    assert _sizes(1, 65536, 512)[3] * 4 == 1 << 30


# ---- every kind: one row per reason ---------------------------------------------------------------------------------------------
def _args(settings, lens=()):
    return [f'{k}={v}' for k, v in settings.items()] + [int(n) for n in lens]


def _good(kind):
    """The settings of the good call of tests/taco_call_cases.py."""
    return dict(B=B, Tin=TIN) if kind == 'encode' else dict(B=B, Tin=TIN, **{'T' if kind == 'forward' else 'max_len': LEN})


@pytest.mark.parametrize('kind,reason,wrong,code,msg', REFUSALS, ids=[f'{r[0]}: {r[1]}' for r in REFUSALS])
def test_refusals(checker, kind, reason, wrong, code, msg):
    wrong = dict(wrong)
    lens = wrong.pop('lens', ())
    settings = dict(_good(kind), **wrong)
    if lens:
        del settings['B']
    assert _call(checker, kind, *_args(settings, lens)) == (code, 'who: ' + msg, None)
    rc, why, _ = _call(checker, kind, *_args(_good(kind)))                   # and the good call is a good call
    assert (rc, why) == (0, '')
    # infer gives what its two halves give -- but it decodes the batch it has just encoded, in a precision and from a mask
    # source its symbol fixes, so those reasons are not its own
    if kind != 'forward' and reason not in ('precision', 'keys NULL', 'offsets NULL'):
        its_own = kind == 'encode' or reason in ('mem kind', 'not ready', 'max_len = 0')
        rc, why, _ = _call(checker, 'infer', *_args(dict(_good('decode'), **wrong)))
        assert (rc, why) == ((code, 'who: ' + msg) if its_own else (0, '')), (rc, why)


def test_refusal_precedence(checker):
    """Two faults in one call: the one earlier in the order csrc/taco_call.h documents is reported.  encode: mem kind, not
    ready, tokens / B / Tin, speaker.  decode: precision, mem kind, not ready, encoded batch, its width, keys / offsets,
    max_len.  infer: the encode order, then the decode order."""
    enc_order = [(dict(mem=9), 'bad mem kind 9'), (dict(ready=0), 'not finalized'), (dict(B=0), 'bad argument (tokens'),
                 (dict(spk_dim=256, null='speaker'), 'speaker embedding')]
    dec_order = [(dict(precision=5), 'precision must be'), (dict(mem=9), 'bad mem kind 9'), (dict(ready=0), 'not finalized'),
                 (dict(null='encoded'), 'encoded batch is NULL'), (dict(enc=768), 'other weights'),
                 (dict(masks=3, null='keys'), 'keys / offsets'), (dict(max_len=-1), 'max_len = -1')]
    for kind, order in (('encode', enc_order), ('decode', dec_order)):
        for i, (first, needle) in enumerate(order):
            for later, _ in order[i + 1:]:
                settings = dict(_good(kind), **later)
                settings.update(first)
                if 'null' in first and 'null' in later:
                    settings['null'] = first['null'] + ',' + later['null']
                rc, why, _ = _call(checker, kind, *_args(settings))
                assert rc != 0 and needle in why, (kind, first, later, why)
    # infer: every encode refusal before every decode one, and both before anything is enqueued
    assert 'bad argument (tokens' in _call(checker, 'infer', 'B=0', 'Tin=12', 'max_len=0')[1]
    assert 'speaker embedding' in _call(checker, 'infer', 'B=3', 'Tin=12', 'max_len=0', 'spk_dim=256', 'null=speaker')[1]
    assert 'max_len = 0' in _call(checker, 'infer', 'B=3', 'Tin=12', 'max_len=0')[1]


def test_the_limits_themselves_are_accepted(checker):
    for kind, settings in [
        ('encode', dict(B=1, Tin=1)), ('encode', dict(B=1024, Tin=4096)), ('encode', dict(B=1, Tin=4096)), ('encode', dict(B=1024, Tin=1)),
        ('encode', dict(B=2, Tin=5, spk_dim=256)),                                        # the 768-wide model with a speaker
        ('encode', dict(B=2, Tin=5, null='speaker')),                                     # no speaker needed: NULL is fine
        ('decode', dict(B=1, Tin=1, max_len=1)), ('decode', dict(B=1024, Tin=4096, max_len=1)),
        ('decode', dict(B=2, Tin=5, max_len=1, enc=768, model_enc=768, precision=1, mem=1)),
        ('decode', dict(B=2, Tin=5, max_len=2147483647)),                                 # no limit above: the workspace decides
        ('decode', dict(B=2, Tin=5, max_len=3, masks=2, null='keys,offsets')),            # only the row streams need them
        ('decode', dict(B=2, Tin=5, max_len=3, masks=3)),
        ('infer', dict(B=1, Tin=1, max_len=1)), ('infer', dict(B=1024, Tin=4096, max_len=1, spk_dim=256, model_enc=768)),
    ]:
        assert _call(checker, kind, *_args(settings)) == (0, '', None), (kind, settings)


# ---- a Python restatement of the two checks, and a fuzz loop against it --------------------------------------------------------
def encode_check(s):
    if s['mem'] not in (0, 1):
        return EINVAL, f"bad mem kind {s['mem']}"
    if not s['ready']:
        return ENOTREADY, 'tacotron2 weights not finalized'
    if 'tokens' in s['null'] or not 1 <= s['B'] <= 1024 or not 1 <= s['Tin'] <= 4096:
        return EINVAL, f"bad argument (tokens is NULL, or B = {s['B']} outside [1, 1024], or Tin = {s['Tin']} outside [1, 4096])"
    if s['spk_dim'] > 0 and 'speaker' in s['null']:
        return EINVAL, 'this model needs a speaker embedding'
    return 0, ''


def run_check(kind, s, lens, has_encoded):
    fwd = kind == 'forward'
    bad, n = ('', 'T') if fwd else ('bad argument: ', 'max_len')
    if s['precision'] not in (0, 1):
        return EINVAL, f"precision must be 0 (f32) or 1 (f16 weights), got {s['precision']}"
    if s['mem'] not in (0, 1):
        return EINVAL, f"bad mem kind {s['mem']}"
    if not s['ready']:
        return ENOTREADY, 'tacotron2 weights not finalized'
    if not has_encoded or s['B'] <= 0 or s['Tin'] <= 0:
        return EINVAL, bad + 'encoded batch is NULL or empty'
    if s['enc'] != s['model_enc']:
        return EINVAL, f"encoded batch belongs to other weights (width {s['enc']}, model {s['model_enc']})"
    if not fwd and s['masks'] == 3 and ('keys' in s['null'] or 'offsets' in s['null']):
        return EINVAL, 'keys / offsets is NULL'
    if fwd and ('mel' in s['null'] or 'lens' in s['null']):
        return EINVAL, 'mel_input or mel_lengths is NULL'
    if s['len'] < 1:
        return EINVAL, f"{bad}{n} = {s['len']} must be at least 1"
    if not fwd:
        return 0, ''
    if s['B'] * s['len'] > 65536:
        return EINVAL, f"B*T too large (B = {s['B']}, T = {s['len']}: above 65536 frames); split the batch"
    for b, v in enumerate(lens):
        if not 1 <= v <= s['len']:
            return EINVAL, f"mel_lengths[{b}] = {v} is outside [1, T = {s['len']}]"
    return 0, ''


def test_both_checks_equal_their_restatement_on_random_calls(checker):
    rng = np.random.default_rng(13)
    pick = lambda *pool: pool[int(rng.integers(len(pool)))]
    seen = set()
    for i in range(400):
        kind = ('encode', 'decode', 'forward', 'infer')[i % 4]
        nulls = [n for n in ('tokens', 'speaker', 'encoded', 'keys', 'offsets', 'mel', 'lens') if rng.random() < 0.15]
        s = dict(B=pick(3, 3, 1, 1024, 0, -1, 1025), Tin=pick(12, 12, 1, 4096, 0, 4097), len=pick(33, 33, 1, 0, -2, 21846, 65536),
                 enc=pick(512, 512, 768), model_enc=pick(512, 512, 768), precision=pick(0, 0, 1, 2, -1), mem=pick(0, 0, 1, 7, -1),
                 ready=pick(1, 1, 1, 0), spk_dim=pick(0, 0, 256), masks=pick(0, 1, 2, 3), null=','.join(nulls))
        lens = ()
        if kind == 'forward' and 0 < s['B'] <= 3 and rng.random() < 0.7:         # explicit mel_lengths, some of them outside [1, T]
            lens = tuple(int(v) for v in rng.integers(min(0, s['len']) if rng.random() < 0.3 else 1, max(s['len'], 1) + 2, s['B']))
        if lens:
            s['B'] = len(lens)
        want = encode_check(s) if kind in ('encode', 'infer') else (0, '')
        if kind != 'encode' and want[0] == 0:
            ss = dict(s, enc=s['model_enc']) if kind == 'infer' else s
            want = run_check(kind, ss, lens or (s['len'],) * max(s['B'], 0) if s['B'] <= 1024 else (), kind == 'infer' or 'encoded' not in nulls)
        settings = {k: v for k, v in s.items() if k not in ('len', 'null') and not (lens and k == 'B')}
        settings['T' if kind == 'forward' else 'max_len'] = s['len']
        if nulls:
            settings['null'] = s['null']
        rc, why, sizes = _call(checker, kind, *_args(settings, lens))
        assert (rc, why) == (want[0], 'who: ' + want[1] if want[0] else ''), (kind, s, lens, rc, why)
        assert sizes == (_sizes(s['B'], s['len'], s['enc']) if kind == 'forward' and rc == 0 else None)
        seen.add((kind, re.sub(r'-?\d+', '#', why)))
    for kind in ('encode', 'decode', 'forward', 'infer'):                        # the loop reached acceptance and the reasons
        assert (kind, '') in seen and sum(k == kind for k, _ in seen) >= 4, sorted(seen)


# ---- the attention window's two integers (HipEngine.tacotron2_infer / tacotron2_decode) -----------------------------------------
def test_attention_window_is_two_integers_or_an_error():
    from text_to_speech_amd.engine import attention_window
    assert attention_window(None, 0) == (0, 0) and attention_window(None, 0.5) == (0, 0) and attention_window(0, 3) == (0, 0)
    assert attention_window(12, 6) == (12, 6) and attention_window(12, None) == (12, 0) and attention_window(1, 0) == (1, 0)
    got = attention_window(np.int64(13), np.float32(6.0))                        # whole numbers of any numeric type
    assert got == (13, 6) and all(type(v) is int for v in got)
    for offset in (0.5, 0.3, np.float32(6.5)):                                   # the reference's default, passed at this level
        with pytest.raises(ValueError, match=r'HipRuntime\.tacotron2_infer'):
            attention_window(12, offset)
    for win_len in (-1, -12, 2.5):
        with pytest.raises(ValueError, match='attn_mask_win_len'):
            attention_window(win_len, 0)
