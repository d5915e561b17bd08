"""CPU: the WaveGlow dispatch in C++ (csrc/wg_plan.h: tile family, rows per phase block and form of a call, as pure host
arithmetic) against its Python restatement `pick_variant` (tests/waveglow_cases.py), which the GPU tests use to say what a
call must have run.  The C++ side is csrc/host_check.cpp's --wg-plan mode, built with -fsanitize=address,undefined like the
weight-file loader (tests/test_host_sanitizer.py): every frame count 1..4096 and every 127th up to the 31 744 frames of the
largest run, in the three precisions and the four forms."""
import os
import shutil
import subprocess

import pytest

import waveglow_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
TILES = {0: '256-row', 1: '128-row', 2: '128x64', 3: '64-row'}       # tts_hip_last_waveglow_tiles
FORM_NAMES = {v: k for k, v in wc.FORMS.items()}
MAX_FRAMES = 31744


@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    exe = os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')
    assert os.path.exists(exe)
    return exe


def _plans(exe, lo, hi, step=1):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, '--wg-plan', str(lo), str(hi), str(step)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def test_wg_plan_agrees_with_pick_variant(checker):
    rows = _plans(checker, 1, 4096) + _plans(checker, 127, MAX_FRAMES, 127) + _plans(checker, MAX_FRAMES, MAX_FRAMES)
    bts = sorted({r[0] for r in rows})
    assert bts[:4096] == list(range(1, 4097)) and bts[-1] == MAX_FRAMES and 4096 + 95 in bts       # 33 * 127
    assert len(rows) == (4096 + len(range(127, MAX_FRAMES + 1, 127)) + 1) * 3 * 4
    bad = []
    for bt, precision, form, pr, tiles, wino in rows:
        v = wc.pick_variant(1, bt, wc.PRECISIONS[precision], FORM_NAMES[form])
        if (pr, TILES[tiles], bool(wino)) != (v.PR, v.tiles, v.wino):
            bad.append((bt, wc.PRECISIONS[precision], FORM_NAMES[form], (pr, TILES[tiles], bool(wino)), (v.PR, v.tiles, v.wino)))
    assert not bad, f'{len(bad)} disagreements (BT, precision, form, C++, Python), first: {bad[:5]}'
    # the sweep itself reaches every tile family of every precision that has it, and both answers on the form
    seen = {(p, TILES[t]) for _, p, _, _, t, _ in rows}
    assert seen == {(0, t) for t in TILES.values()} | {(1, t) for t in TILES.values()} | {(2, '64-row'), (2, '256-row')}
    assert {(f, w) for _, p, f, _, _, w in rows if p == 0} == {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)}
    assert not any(w for _, p, _, _, _, w in rows if p != 0)
