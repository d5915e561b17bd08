"""CPU: the one-flow restatement of the forward direction (waveglow_encode_ref.init_step / flow_step / chain) and the comparison
tests/test_waveglow_encode_flows_gpu.py makes with it (waveglow_encode_ref.StepCheck).

Chained from the init step, the twelve float64 steps must BE `forward`: z bit-equal, the running sums its sum_log_s.  Then the
planted mistakes: each FLOW_MISTAKE is planted in a chain that stands for the engine, and the step it touches is measured
exactly as the GPU test measures the engine -- on the source's own input to that step, in units of the step's float32 floor.
The GPU test allows ten floors; a mistake must show at ten times that bound (100 floors) in the quantity it belongs to.

Shapes: 2 x 5 frames on the `replace_invertible_kernels` weights (non-orthogonal matrices: on the session weights a transposed
matrix is still norm-preserving); one WN block costs about 0.1 s here.
"""
import os
import re

import numpy as np
import pytest

import waveglow_encode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 2, 5


def _inputs(seed=21):
    rng = np.random.default_rng(seed)
    mel = rng.uniform(-11.5, 1.2, (B, T, 80)).astype(np.float32)
    audio = rng.uniform(-0.9, 0.9, (B, T * 256)).astype(np.float32)
    return audio, mel


@pytest.fixture(scope='module')
def replaced(wg_weights, wg_cfg):
    return ref.replace_invertible_kernels(wg_weights, wg_cfg)


@pytest.fixture(scope='module')
def good(replaced, wg_cfg):
    audio, mel = _inputs()
    return ref.chain(audio, mel, replaced, wg_cfg)


@pytest.mark.parametrize('which', ['session', 'replaced'])
def test_chained_steps_are_forward(wg_weights, replaced, wg_cfg, which):
    w = wg_weights if which == 'session' else replaced
    audio, mel = _inputs()
    z, stats = ref.forward(audio, mel, w, wg_cfg)
    c = ref.chain(audio, mel, w, wg_cfg)
    assert c['z'].dtype == np.float64 and np.array_equal(c['z'], z)
    assert [c['state'][k].shape[2] for k in range(-1, 12)] == [8] * 4 + [6] * 4 + [4] * 5
    assert np.array_equal(c['state'][11], z[:, :, :4])
    sum_s = c['slog'][11].sum(axis=1)
    print(f'{which}: sum_log_s {stats[1].tolist()} chained {sum_s.tolist()}')
    assert np.allclose(sum_s, stats[1], rtol=1e-12, atol=0)               # the same terms, added in another order
    assert np.all(np.abs(stats[1]) > 1.0)


def test_z_slots(wg_cfg):
    slots = {k: ref.z_slot(k, wg_cfg) for k in range(12)}
    assert {k: (s.start, s.stop) for k, s in slots.items() if s is not None} == {3: (6, 8), 7: (4, 6), 11: (0, 4)}
    assert ref.z_slot(3, wg_cfg, 'zoff_swapped') == slice(4, 6) and ref.z_slot(7, wg_cfg, 'zoff_swapped') == slice(6, 8)


_spect = []


def _measure(source, audio, mel, w, cfg, k):
    """What the GPU test computes for flow k, with `source` (a chain) in the engine's place."""
    if not _spect:                                                      # (one mel in this module)
        _spect.append({dt: ref.spect_of(mel, w, cfg, dt) for dt in (np.float64, np.float32)})
    state_in = audio.reshape(B, -1, 8) if k < 0 else source['state'][k - 1]
    check = ref.StepCheck(state_in, _spect, w, cfg, k, ref.row_groups(B, T))
    inc = None if k < 0 else source['slog'][k] - (source['slog'][k - 1] if k > 0 else 0.0)
    return check.floors(source['state'][k], inc, source['z'])


# mistake -> [(flow, the quantity that must show it)]
TOUCHES = {
    'early_wrong_end': [(3, 'state'), (3, 'early'), (7, 'state'), (7, 'early')],
    'zoff_swapped': [(3, 'early'), (7, 'early')],
    'next_transposed': [(0, 'state'), (3, 'state'), (10, 'state')],
    'next_old_n': [(3, 'state'), (7, 'state')],
    's_summed_over_b': [(0, 'slog'), (5, 'slog')],
    'slog_not_reset': [(0, 'slog')],
}


def test_the_table_names_every_mistake():
    assert set(TOUCHES) == set(ref.FLOW_MISTAKES)


@pytest.mark.parametrize('mistake', ref.FLOW_MISTAKES)
def test_each_planted_mistake_shows_in_the_step_it_touches(replaced, wg_cfg, good, mistake):
    audio, mel = _inputs()
    bad = ref.chain(audio, mel, replaced, wg_cfg, mistake=mistake, stale_slog=good['slog'][11])
    for k, what in TOUCHES[mistake]:
        f = _measure(bad, audio, mel, replaced, wg_cfg, k)
        print(f'{mistake}: flow {k}: ' + ', '.join(f'{q} {v:.3g} floors' for q, v in f.items()))
        assert not f[what] < 10 * ref.StepCheck.MARGIN, (mistake, k, what, f)


def test_the_unmistaken_chain_measures_zero_and_a_float32_chain_one_floor(replaced, wg_cfg, good):
    """The yardstick itself: the float64 chain is its own reference, and a float32 chain -- the floor's definition -- sits at
    one floor in every quantity of every step that has it."""
    audio, mel = _inputs()
    low = ref.chain(audio, mel, replaced, wg_cfg, dtype=np.float32)
    for k in (-1, 0, 3, 7, 11):
        f = _measure(good, audio, mel, replaced, wg_cfg, k)
        assert f['state'] == 0.0 and f.get('early', 0.0) == 0.0 and f.get('slog', 0.0) < 1e-6, (k, f)   # (slog: a float64 difference)
        assert set(f) == {'state'} | ({'slog'} if k >= 0 else set()) | ({'early'} if k in (3, 7, 11) else set())
        f = _measure(low, audio, mel, replaced, wg_cfg, k)
        print(f'float32 chain, flow {k}: ' + ', '.join(f'{q} {v:.2f}' for q, v in f.items()))
        assert f['state'] == pytest.approx(1.0, abs=1e-6)
        if 'early' in f:                                                # (flows 3 and 7: passed on untouched, floor 0)
            assert f['early'] == (pytest.approx(1.0, abs=1e-6) if k == 11 else 0.0)
        if k >= 0:
            assert f['slog'] == pytest.approx(1.0, abs=1e-6)              # (the chain keeps its running sum in float64)


# ---- the hook's front end under the sanitizers
@pytest.fixture(scope='module')
def host_check():
    import subprocess
    csrc = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
    subprocess.run(['bash', os.path.join(csrc, 'build_host_asan.sh')], check=True, capture_output=True)
    exe = os.path.join(csrc, 'build_host_asan', 'ttsw_check_asan')

    def run(T, *args):
        p = subprocess.run([exe, '--wg-encode', str(T), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        status, _, msg = p.stdout.strip().partition(' ')
        return int(status), msg
    return run


def probe_refusal(T, flow, what, null=(), **call):
    """The refusal order of tts_hip_waveglow_encode_probe (include/tts_hip.h): whatever the plain call refuses of the same inputs
    -- its outputs are not looked at -- then the hook's own arguments -> the reason's key, or None."""
    from test_waveglow_encode import refusal
    plain = refusal(T, null=tuple(n for n in null if n in ('audio', 'mel')), **call)
    if plain is not None:
        return plain
    if not -1 <= flow <= 11:
        return f'flow = {flow} '
    if not 0 <= what <= 1:
        return f'what = {what} '
    if what == 1 and flow < 0:
        return 'needs flow >= 0'
    if 'out' in null:
        return 'out is NULL'
    return None


PROBE_CALLS = [
    dict(T=5, B=2, flow=-1, what=0), dict(T=5, B=2, flow=11, what=1), dict(T=5, lengths=[5, 0, 3], flow=3, what=0),
    dict(T=5, B=2, flow=0, what=0, null=('z', 'stats')),                  # the plain call's outputs are not the hook's business
    dict(T=5, B=2, flow=-2, what=0), dict(T=5, B=2, flow=12, what=1), dict(T=5, B=2, flow=3, what=2), dict(T=5, B=2, flow=3, what=-1),
    dict(T=5, B=2, flow=-1, what=1), dict(T=5, B=2, flow=3, what=0, null=('out',)), dict(T=5, B=2, flow=12, what=5, null=('out',)),
    dict(T=5, B=2, flow=-1, what=1, null=('out',)), dict(T=5, B=2, flow=12, what=0, mem=7), dict(T=5, B=0, flow=12, what=0),
    dict(T=0, B=1, flow=12, what=0), dict(T=5, B=1, flow=3, what=7, null=('mel', 'out')), dict(T=5, lengths=[5, 6], flow=-5, what=0),
    dict(T=31745, B=1, flow=3, what=0, null=('out',)), dict(T=31744, B=1, flow=3, what=0),
]


@pytest.mark.parametrize('call', PROBE_CALLS, ids=lambda c: ' '.join(f'{k}={str(v)[:24]}' for k, v in c.items()))
def test_probe_front_end_refuses_in_the_documented_order(host_check, call):
    args = [f'{k}={call[k]}' for k in ('B', 'mem', 'flow', 'what') if call.get(k) is not None]
    if call.get('null'):
        args.append('null=' + ','.join(call['null']))
    status, msg = host_check(call['T'], *args, *call.get('lengths', []))
    want = probe_refusal(**call)
    if want is None:
        assert (status, msg) == (0, '')
    else:
        assert status == -1 and msg.startswith('who: ') and want in msg, (msg, want)


def test_header_and_binding_name_the_probe():
    from text_to_speech_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tts_hip.h')).read()
    name = 'tts_hip_waveglow_encode_probe'
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 10
    assert re.search(r'int %s\(tts_hip_engine\* e, const float\* audio, const float\* mel, int B, int T, const int32_t\* lengths,'
                     r'\s+int flow, int what, float\* out, int mem\);' % name, header)
    assert 'Armed probe hooks' not in header
    assert _lib.ABI_VERSION == 13                                           # additions only
