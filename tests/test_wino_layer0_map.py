"""CPU: the tap operand of the first WN layer of a flow in its Winograd form (csrc/wn_wino.hip, wino_layer0_kernel).

Its three taps act on the neighbouring POSITIONS n - 1, n, n + 1 of position n = 32 t + p.  The kernel's operand is one
16-float row per position, [a(n-1)[0..h), v(n-1) | a(n)[0..h), v(n) | a(n+1)[0..h), v(n+1) | 0 ..], copied from the rows of a0p
(h coupling channels, then the constant 1 that carries the start conv's bias) by the three functions of csrc/wg_plan.h that
wino_tap_operand_kernel runs: a neighbour outside the utterance contributes nothing, and neither does one on a tail frame of a
ragged row, whose a0p row -- the 1 included -- was cleared before.  In the phase-major layout the neighbours lie in the phase
blocks p - 1 and p + 1, carried into frame t - 1 at p = 0 and t + 1 at p = 31.

csrc/host_check.cpp's --wn-taps mode runs those functions on a model a0p (column c < h of row m holds 1 + 8 m + c, column h
holds 1, cleared tail rows) under ASan / UBSan; this file restates the operand by positions, without the layout's arithmetic:
T in 1 .. 9, B in 1 .. 3, h in 2 .. 4, with and without lengths.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
NPH = 32


@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    exe = os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')
    assert os.path.exists(exe)
    return exe


def _kernel_side(exe, h, T, lens):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, '--wn-taps', str(h), str(T)] + [str(n) for n in lens], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    PR = int(lines[0])
    rows = np.array([[int(x) for x in line.split()] for line in lines[1:]], dtype=np.int64)
    assert rows.shape == (NPH * PR, 16)
    return PR, rows


def _restated(h, T, lens, PR):
    """The operand by positions: utterance b is the sequence of its 32 T positions; position n holds the values of a0p's row
    (n % 32) * PR + b * T + n // 32 when its frame is real, nothing otherwise."""
    B = len(lens)
    want = np.zeros((NPH * PR, 16), dtype=np.int64)
    for b in range(B):
        def value(n, c):
            if n < 0 or n >= NPH * T or n // NPH >= lens[b]:
                return 0
            m = (n % NPH) * PR + b * T + n // NPH
            return 1 + 8 * m + c if c < h else 1
        for n in range(NPH * T):
            m = (n % NPH) * PR + b * T + n // NPH
            row = [value(n + s, c) for s in (-1, 0, 1) for c in range(h + 1)]
            want[m, :len(row)] = row
    return want


def _lengths(B, T):
    """Without lengths (every frame real), then rows that end early: one frame, all but one, none."""
    yield (T,) * B
    yield tuple(max(0, T - 1 - b) for b in range(B))
    yield tuple((1, T, 0)[(b + T) % 3] for b in range(B))


def test_tap_operand_is_the_three_neighbouring_positions(checker):
    cases = 0
    for T in range(1, 10):
        for B in range(1, 4):
            h = 2 + (T + B) % 3
            for lens in _lengths(B, T):
                PR, got = _kernel_side(checker, h, T, lens)
                assert PR >= B * T
                want = _restated(h, T, lens, PR)
                bad = np.argwhere(got != want)
                assert not len(bad), f'h {h} T {T} lengths {lens}: first difference at row, column {bad[0]}'
                # the indicator columns by themselves: the centre's is 1 on a real frame, a neighbour's where it exists
                real = np.zeros(NPH * PR, bool)
                for b, n in enumerate(lens):
                    for p in range(NPH):
                        real[p * PR + b * T:p * PR + b * T + n] = True
                assert (got[:, 2 * h + 1] == real).all() and not got[:, 3 * (h + 1):].any()
                cases += 1
    assert cases == 9 * 3 * 3


def test_every_coupling_width_is_covered(checker):
    for h in (2, 3, 4):
        PR, got = _kernel_side(checker, h, 5, (5, 3))
        assert (got == _restated(h, 5, (5, 3), PR)).all()
        # the first position of an utterance has no left neighbour, the last real one no right neighbour
        first, last = 0 * PR + 0, 31 * PR + 4
        assert not got[first, :h + 1].any() and got[first, h + 1:2 * (h + 1)].all()
        assert not got[last, 2 * (h + 1):].any() and got[last, :2 * (h + 1)].all()
        last_ragged = 31 * PR + 5 + 2
        assert not got[last_ragged, 2 * (h + 1):].any() and got[last_ragged, :2 * (h + 1)].all()
