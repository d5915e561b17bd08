"""CPU: the forward flow's float64 restatement (tests/waveglow_encode_ref.py), the front end of tts_hip_waveglow_encode under
ASan / UBSan, and the host arithmetic of WaveGlow.encode / WaveGlow.evaluate on a recording runtime.

Shapes: 2 x 5 frames (160 positions a row; the widest dilation, 128 groups, still lies inside a row) -- a run of the oracle
costs about a second.  Bounds: float64 restatements of the same arithmetic agree to 1e-10 (eps 1.1e-16 times a few thousand
accumulated terms, times the flows' conditioning); the planted-mistake table uses the GPU test's own bound, ten times the
float32 floor of the case (waveglow_encode_ref.Case).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import waveglow_encode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
F64_TOL = 1e-10


def _inputs(B, T, seed=21):
    rng = np.random.default_rng(seed)
    mel = rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    audio = rng.uniform(-0.9, 0.9, (B, T * 256)).astype(np.float32)
    return audio, mel


@pytest.fixture(scope='module')
def replaced(wg_weights, wg_cfg):
    return ref.replace_invertible_kernels(wg_weights, wg_cfg)


@pytest.fixture(scope='module')
def ragged_case(replaced, wg_cfg):
    """2 x 5 frames, lengths [5, 3], on the replaced kernels: the case of the planted-mistake table."""
    audio, mel = _inputs(2, 5)
    return ref.Case(audio, mel, replaced, wg_cfg, lengths=[5, 3])


# ---- the restatement
def test_synthetic_kernels_are_orthogonal_and_the_replaced_ones_are_not(wg_weights, replaced, wg_cfg):
    """Why the kernels are replaced: on the session weights every log|det| is 0 to float32 rounding."""
    assert np.abs(ref.log_abs_dets(wg_weights, wg_cfg)).max() < 1e-6
    ld = ref.log_abs_dets(replaced, wg_cfg)
    dets = [np.linalg.det(replaced[f'waveglow/invertible_conv-{k}/conv/kernel'][0].astype(np.float64)) for k in range(12)]
    assert np.abs(ld).min() > 0.1 and abs(ld.sum()) > 1.0
    assert [d < 0 for d in dets] == [k % 3 == 1 for k in range(12)]
    for k in range(12):
        sv = np.linalg.svd(replaced[f'waveglow/invertible_conv-{k}/conv/kernel'][0].astype(np.float64), compute_uv=False)
        assert 0.5 - 1e-6 <= sv.min() and sv.max() <= 2.0 + 1e-6


@pytest.mark.parametrize('which', ['session', 'replaced'])
def test_restatement_is_the_oracles_forward_flow_and_infer_inverts_it(wg_weights, replaced, wg_cfg, which):
    from oracle import waveglow_ref
    w = wg_weights if which == 'session' else replaced
    audio, mel = _inputs(2, 5)
    z, stats = ref.forward(audio, mel, w, wg_cfg)
    assert z.dtype == np.float64 and z.shape == (2, 160, 8) and stats.shape == (3, 2)
    assert np.array_equal(z, waveglow_ref.forward_flow(audio, mel, w, wg_cfg))
    assert np.allclose(stats[0], np.square(z).sum(axis=(1, 2)), rtol=1e-13)
    assert np.allclose(stats[2], 160 * ref.log_abs_dets(w, wg_cfg).sum(), rtol=1e-12, atol=1e-12)
    back = waveglow_ref.infer(mel, w, wg_cfg, z=z, sigma=1.0, dtype=np.float64)
    err = ref.rms(back - audio)
    print(f'{which}: float64 round trip rms {err:.3e}, z rms {ref.rms(z):.3f}, stats {stats.tolist()}')
    assert err < F64_TOL


def test_sums_have_their_closed_form_without_the_end_kernels(replaced, wg_cfg):
    """end_conv kernels zeroed: (b, s) are the end biases at every position, so sum_log_s = positions * sum of the s halves of
    the twelve biases, and log_det_w = positions * sum of numpy's slogdet."""
    w = dict(replaced)
    closed = 0.0
    for k in range(12):
        w[f'waveglow/block-{k}/end_conv/kernel'] = np.zeros_like(replaced[f'waveglow/block-{k}/end_conv/kernel'])
        bias = replaced[f'waveglow/block-{k}/end_conv/bias'].astype(np.float64)
        closed += bias[len(bias) // 2:].sum()
    audio, mel = _inputs(1, 3)
    _, stats = ref.forward(audio, mel, w, wg_cfg)
    slog = sum(np.linalg.slogdet(replaced[f'waveglow/invertible_conv-{k}/conv/kernel'][0].astype(np.float64))[1] for k in range(12))
    assert abs(closed) > 0.01
    assert np.allclose(stats[1], 96 * closed, rtol=1e-12) and np.allclose(stats[2], 96 * slog, rtol=1e-12)


def test_each_planted_mistake_moves_a_compared_quantity_ten_bounds(ragged_case):
    """What the GPU comparison (z within z_bound RMS, every statistic within stats_bound relative) would notice: each mistake
    moves z or a statistic to at least ten times its bound (NaN counts: a comparison with NaN fails)."""
    c = ragged_case
    moved_by = {}
    for mistake in ref.MISTAKES:
        z, stats = c.run(np.float64, mistake)
        ez, es = c.errors(z, stats)
        by_z = not ez < 10 * c.z_bound
        by_stat = [bool(np.any(~(es[i] < 10 * c.stats_bound[i]))) for i in range(3)]
        moved_by[mistake] = (by_z, by_stat)
        print(f'{mistake}: z {ez / c.z_bound:.3g} bounds, statistics {(es / c.stats_bound).max(axis=1)} bounds')
        assert by_z or any(by_stat), mistake
    # and the ones only a statistic shows are shown by the statistic they belong to
    assert moved_by['one_flow_s_left_out'] == (False, [False, True, False])
    assert moved_by['log_det_signed'] == (False, [False, False, True])
    assert moved_by['tail_counted'][1][1] and moved_by['tail_counted'][1][2]
    assert all(moved_by[m][0] for m in ('early_swapped', 'matrix_transposed', 'exp_minus_s'))
    print(f'floors: z {c.z_floor:.3e} (z rms {ref.rms(c.z):.3f}), statistics {c.stats_floor.tolist()}')


def test_ragged_restatement_contract(ragged_case):
    c = ragged_case
    assert np.all(c.z[1, 3 * 32:] == 0) and np.all(c.z[1, :3 * 32] != 0)
    assert np.isclose(c.stats[2, 1] / c.stats[2, 0], 3 / 5, rtol=1e-12)


# ---- the front end under the sanitizers
@pytest.fixture(scope='module')
def host_check():
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    exe = os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')

    def run(T, *args):
        p = subprocess.run([exe, '--wg-encode', str(T), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        status, _, msg = p.stdout.strip().partition(' ')
        return int(status), msg
    return run


MAX_RUN = 31744


def refusal(T, B=None, lengths=None, mem=0, is_async=False, null=()):
    """The refusal order of tts_hip_waveglow_encode (include/tts_hip.h), first match wins -> the reason's key, or None."""
    if lengths is not None:
        B = len(lengths)
    if not is_async and mem not in (0, 1):
        return 'bad mem kind'
    if B <= 0:
        return 'B = '
    if 'audio' in null or 'mel' in null or T <= 0:
        return 'audio or mel is NULL'
    if 'z' in null and 'stats' in null:
        return 'both NULL'
    if lengths is not None:
        for b, n in enumerate(lengths):
            if n < 0 or n > T:
                return f'lengths[{b}] = {n} '
    if B * T > MAX_RUN:
        return 'exceeds one run'
    return None


CALLS = [
    dict(T=5, B=2), dict(T=5, lengths=[5, 0, 3]), dict(T=5, B=2, mem=1), dict(T=5, B=2, mem=7),
    dict(T=5, B=2, mem=7, is_async=True), dict(T=5, B=0, mem=7), dict(T=5, B=-3), dict(T=0, B=0), dict(T=0, B=1),
    dict(T=-2, B=1, null=('z', 'stats')), dict(T=5, B=1, null=('audio',)), dict(T=5, B=1, null=('mel', 'z', 'stats')),
    dict(T=5, B=1, null=('z',)), dict(T=5, B=1, null=('stats',)), dict(T=5, B=1, null=('z', 'stats')),
    dict(T=5, lengths=[6], null=('z', 'stats')), dict(T=5, lengths=[5, 6, -1]), dict(T=5, lengths=[5, -1]),
    dict(T=MAX_RUN, B=1), dict(T=MAX_RUN + 1, B=1), dict(T=MAX_RUN // 2, B=2), dict(T=MAX_RUN // 2 + 1, B=2),
    dict(T=MAX_RUN // 2 + 1, lengths=[0, MAX_RUN]), dict(T=70000, B=70000), dict(T=4, lengths=[9] + [4] * 7936),
]


@pytest.mark.parametrize('call', CALLS, ids=lambda c: ' '.join(f'{k}={str(v)[:24]}' for k, v in c.items()))
def test_front_end_refuses_in_the_documented_order(host_check, call):
    args = [f'{k}={v}' for k, v in (('B', call.get('B')), ('mem', call.get('mem'))) if v is not None]
    if call.get('is_async'):
        args.append('async=1')
    if call.get('null'):
        args.append('null=' + ','.join(call['null']))
    status, msg = host_check(call['T'], *args, *call.get('lengths', []))
    want = refusal(**call)
    if want is None:
        assert (status, msg) == (0, '')
    else:
        assert status == -1 and msg.startswith('who: ') and want in msg, (msg, want)


# ---- the C ABI
def test_header_and_binding_name_the_two_entry_points():
    from text_to_speech_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tts_hip.h')).read()
    for name, last in (('tts_hip_waveglow_encode', 'int mem'), ('tts_hip_waveglow_encode_async', r'void\* stream')):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 9
        assert re.search(r'int %s\(tts_hip_engine\* e, const float\* audio, const float\* mel, int B, int T, '
                         r'const int32_t\* lengths,\s+float\* z, float\* stats, %s\);' % (name, last), header)
    assert _lib.ABI_VERSION == 13                                           # additions only


# ---- WaveGlow.encode / evaluate on a recording runtime
class RecordingRuntime:
    """Stands for HipRuntime: keeps every call's arguments and answers with statistics that are simple functions of what it was
    given -- stats[0] = sum of the row's real samples squared, stats[1] = sum of its real mel, stats[2] = 0.25 * frames."""

    def __init__(self):
        self.calls = []

    def waveglow_encode(self, audio, mel, lengths=None):
        B, T = mel.shape[:2]
        lens = np.full(B, T) if lengths is None else np.asarray(lengths)
        self.calls.append((np.array(audio), np.array(mel), None if lengths is None else np.array(lengths)))
        stats = np.zeros((3, B), dtype=np.float32)
        for b in range(B):
            stats[0, b] = np.square(audio[b, :lens[b] * 256].astype(np.float64)).sum()
            stats[1, b] = mel[b, :lens[b]].astype(np.float64).sum()
            stats[2, b] = 0.25 * lens[b]
        return np.zeros((B, T * 32, 8), dtype=np.float32), stats


def _items(frames, seed=3):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-1, 1, f * 256 - (17 if f else 0)).astype(np.float32), rng.uniform(-1, 1, (f, 80)).astype(np.float32))
            for f in frames]


def test_evaluate_batches_pads_and_scores():
    from text_to_speech_amd.waveglow import WaveGlow
    rt = RecordingRuntime()
    frames = [4, 7, 0, 2, 5, 3, 1]
    items = _items(frames)
    res = WaveGlow(rt).evaluate(items, batch_size=3, sigma=0.7)
    assert res['names'] == ('nll', 'sum_z2', 'sum_log_s', 'log_det_w') and res['per_item'].shape == (4, 7)
    assert [len(c[2]) for c in rt.calls] == [3, 3, 1]                      # consecutive items, at most batch_size rows
    at = 0
    for audio, mel, lens in rt.calls:
        T = max(1, max(frames[at:at + len(lens)]))
        assert audio.shape == (len(lens), T * 256) and mel.shape == (len(lens), T, 80) and lens.dtype == np.int32
        assert lens.tolist() == frames[at:at + len(lens)]
        for r, n in enumerate(lens):
            w, m = items[at + r]
            assert np.array_equal(audio[r, :len(w)], w) and np.all(audio[r, len(w):] == 0)    # zero-padded to frames * 256 and on
            assert np.array_equal(mel[r, :n], m) and np.all(mel[r, n:] == 0)
        at += len(lens)
    for i, (w, m) in enumerate(items):
        z2, ls = float(np.float32(np.square(w.astype(np.float64)).sum())), float(np.float32(m.astype(np.float64).sum()))
        ld = 0.25 * frames[i]
        want = (z2 / (2 * 0.7 ** 2) - ls - ld) / (frames[i] * 256) if frames[i] else 0.0
        assert np.allclose(res['per_item'][:, i], [want, z2, ls, ld], rtol=1e-12, atol=0)
    assert res['per_item'][0, 2] == 0.0                                     # the empty item
    assert np.allclose(res['mean'], res['per_item'].mean(axis=1), rtol=1e-15)


def test_evaluate_keeps_a_batch_within_one_run():
    from text_to_speech_amd.waveglow import WaveGlow
    rt = RecordingRuntime()
    model = WaveGlow(rt)
    model.MAX_RUN_FRAMES = 20                                               # (instance attribute: the class keeps the engine's)
    res = model.evaluate(_items([6, 7, 7, 3, 20]), batch_size=8)
    assert [c[2].tolist() for c in rt.calls] == [[6, 7], [7, 3], [20]]       # rows x longest row <= 20
    assert res['per_item'].shape == (4, 5)
    with pytest.raises(ValueError, match='above one run'):
        model.evaluate(_items([21]))
    assert WaveGlow.MAX_RUN_FRAMES == MAX_RUN


def test_encode_pads_the_audio_and_reports_the_terms():
    from text_to_speech_amd.waveglow import WaveGlow
    rt = RecordingRuntime()
    (w, m), = _items([6])
    out = WaveGlow(rt).encode(w, m)
    audio, mel, lens = rt.calls[0]
    assert lens is None and audio.shape == (1, 6 * 256) and np.array_equal(audio[0, :len(w)], w) and np.all(audio[0, len(w):] == 0)
    assert set(out) == {'z', 'mel', 'nll', 'sum_z2', 'sum_log_s', 'log_det_w'} and out['z'].shape == (6 * 32, 8)
    assert np.isclose(out['nll'], (out['sum_z2'] / 2 - out['sum_log_s'] - out['log_det_w']) / (6 * 256), rtol=1e-12)
    assert out['log_det_w'] == 1.5 and out['mel'] is not None and np.array_equal(out['mel'], m)


def test_a_runtime_without_the_forward_flow_is_named():
    from text_to_speech_amd.waveglow import WaveGlow
    model = WaveGlow(lambda mel, **kw: None)
    with pytest.raises(ValueError, match='evaluate needs a runtime with waveglow_encode'):
        model.evaluate([])
    with pytest.raises(ValueError, match='encode needs a runtime with waveglow_encode'):
        model.encode(np.zeros(256, np.float32), np.zeros((1, 80), np.float32))
    with pytest.raises(ValueError, match='batch_size'):
        WaveGlow(RecordingRuntime()).evaluate([], batch_size=0)
