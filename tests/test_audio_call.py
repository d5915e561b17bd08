"""CPU: the front end of every audio call in C++ (csrc/audio_call.h: the reasons reduce_noise, trim_silence, resample and
remove_silence refuse a call, and the geometry they derive from an accepted one, as pure host code) against a restatement
written here from the documented layouts (the probes' docstrings in text_to_speech_amd/engine.py, tests/reduce_noise_cases.py,
tests/trim_conv_cases.py, csrc/resample.hip's and csrc/silence.hip's headers).  The C++ side is csrc/host_check.cpp's
--audio-call mode, built with -fsanitize=address,undefined like the weight-file loader: `lengths` is untrusted input."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'text_to_speech_amd', 'csrc')
LIM = (1 << 31) - 65536                               # bytes a GEMM descriptor addresses (reduce_noise, trim_silence)
LIM31 = 1 << 31                                       # bytes the resample / remove_silence kernels index
SIZES = [1, 511, 512, 513, 2047, 2048, 2049]


@pytest.fixture(scope='module')
def checker():
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    subprocess.run(['bash', os.path.join(CSRC, 'build_host_asan.sh')], check=True, capture_output=True)
    exe = os.path.join(CSRC, 'build_host_asan', 'ttsw_check_asan')
    assert os.path.exists(exe)
    return exe


def _call(exe, kind, lengths=(), **settings):
    """-> (status, message, rows of ints printed behind an accepted call)."""
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    args = [exe, '--audio-call', kind] + [f'{k}={v}' for k, v in settings.items()] + [str(int(n)) for n in lengths]
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    status, _, message = lines[0].partition(' ')
    if int(status) != 0:
        assert len(lines) == 1
        return int(status), message, None
    assert message == ''
    return 0, '', [[int(x) for x in line.split()] for line in lines[1:]]


def _accepted(exe, kind, lengths=(), **settings):
    rc, msg, rows = _call(exe, kind, lengths, **settings)
    assert rc == 0, msg
    return rows


def _refused(exe, kind, needles, lengths=(), **settings):
    rc, msg, rows = _call(exe, kind, lengths, **settings)
    assert rc == -1 and rows is None and msg.startswith('who: '), (rc, msg)
    assert all(n in msg for n in needles), msg
    return msg


def ceil_div(a, b):
    return -(-a // b)


def carved(*slices):
    """Extent of a workspace whose slices each start on a 256-byte boundary."""
    return sum(ceil_div(n, 256) * 256 for n in slices)


def ceil_log2(v):
    return max(0, (v - 1).bit_length())


# ---- geometry of accepted calls ---------------------------------------------------------------------------------------------
def rn_geometry(B, N, noise_len):
    """reduce_noise_probe's docstring: Fr = ceil((N + 2560) / 512) frame slots of 512 per row, Frn = ceil((noise_len + 2048) /
    512); the workspace: [4][B] row facts, [2][B] maxima, [B][1025] thresholds, the padded rows (+ 2048 floats the last frames
    read), the spectra [.][2080], the frames [.][2048], the byte mask [.][1025]."""
    Fr, Frn = ceil_div(N + 2560, 512), ceil_div(noise_len + 2048, 512)
    total = carved(16 * B, 8 * B, B * 1025 * 4, (B * Fr * 512 + 2048) * 4, (B * Frn * 512 + 2048) * 4, B * Fr * 2080 * 4,
                   B * Frn * 2080 * 4, B * Fr * 2048 * 4, B * Fr * 1025)
    return [Fr, Fr * 512, Frn, Frn * 512, total]


@pytest.mark.parametrize('N', SIZES)
def test_reduce_noise_geometry(checker, N):
    for B, noise_len, lengths in ((1, 1, ()), (3, 4410, (N, 1, max(1, N // 2))), (2, 2049, ())):
        rows = _accepted(checker, 'reduce_noise', lengths, B=B, N=N, noise_len=noise_len)
        assert rows == [rn_geometry(B, N, noise_len)], (B, N, noise_len)


@pytest.mark.parametrize('N', SIZES)
def test_trim_geometry(checker, N):
    """trim_silence_probe's docstring: conv [B, max(N, W) + 1], W = 2 * (window_length // 2); the taps are padded to 4."""
    for wl in (2, 3, 201, 4410):
        W = 2 * (wl // 2)
        assert _accepted(checker, 'trim', (N, 1), N=N, window_length=wl) == [[W, ceil_div(W, 4) * 4, max(N, W) + 1]]


def sil_geometry(B, N, method, rate, min_silence, bs):
    """csrc/silence.hip: tiles of 2048 samples; rms: NB = ceil(N / bs) block flags per row and room for one silence per
    q + 1 blocks, q = blocks per min_silence less one (at least 1); mean-window: w = int(min_silence * rate) taps, fp64
    tile sums, prefix sums [B][N + 1] and totals."""
    NT, NB, cap, w = ceil_div(N, 2048), 0, 1, 0
    rms, mw = method == 0, method == 2
    if rms:
        NB = ceil_div(N, bs)
        cap = NB // (max(1, int(min_silence / (bs / rate)) - 1) + 1) + 1
    if mw:
        w = int(min_silence * rate)
    total = carved(4 * B, B * N, 4 * B * NT, 4 * B * NT, 4 * B, 4 * B, 4 * B * cap, 4 * B * cap,
                   B * NB if rms else 0, *([4 * B * cap] * 2 if rms else [0, 0]),
                   *([8 * B * NT] * 2 + [8 * B * (N + 1), 8 * B] if mw else [0] * 4))
    return [NT, NB, cap, w, total]


@pytest.mark.parametrize('N', SIZES)
def test_silence_geometry(checker, N):
    for method, min_silence, bs in ((0, 0.1, 220), (0, 0.0, 1), (0, 0.5, 7), (1, 0.0, 1), (2, 1 / 22050, 1), (2, N / 22050, 1)):
        if method == 2 and int(min_silence * 22050) not in range(1, N + 1):       # (float rounding of N / 22050 * 22050)
            continue
        rows = _accepted(checker, 'silence', (N, N, max(1, N - 1)) if method != 2 else (), B=3, N=N, method=method, rate=22050,
                         min_silence=repr(min_silence), block_size=bs, threshold=0.025)
        assert rows == [sil_geometry(3, N, method, 22050, min_silence, bs)], (N, method, min_silence, bs)


def rs_geometry(n, rate, target):
    """csrc/resample.hip: M_b = int(N_b / rate * target_rate); Bluestein lengths L_fwd >= N + N // 2 and L_inv >= 2 M - 1,
    powers of two of at least 64."""
    m = int(n / rate * target)
    return [max(6, ceil_log2(n + n // 2)), max(6, ceil_log2(2 * m - 1)), m]


@pytest.mark.parametrize('N', SIZES)
def test_resample_geometry(checker, N):
    for rate, target in ((16000, 22050), (22050, 16000), (44100, 44100), (1, 3)):
        lengths = [n for n in (N, max(1, N - 1), N // 2 + 1, 3) if n <= N and int(n / rate * target) >= 1]
        if int(N / rate * target) < 1:
            continue
        rows = _accepted(checker, 'resample', lengths, N=N, rate=rate, target_rate=target, M=int(N / rate * target))
        assert rows == [rs_geometry(n, rate, target) for n in lengths], (N, rate, target)


def test_resample_groups_on_either_side_of_a_power_of_two(checker):
    """Rows are grouped by (L_fwd, L_inv): N + N // 2 = 8191 / 8193 around 2^13, and 2 M - 1 = 8191 / 8193."""
    assert 5461 + 5461 // 2 == 8191 and 5462 + 5462 // 2 == 8193
    rows = _accepted(checker, 'resample', (5461, 5462), N=5462, rate=22050, target_rate=8000, M=int(5462 / 22050 * 8000))
    assert [r[0] for r in rows] == [13, 14] and rows == [rs_geometry(n, 22050, 8000) for n in (5461, 5462)]
    for N, rate, target, M, logi in ((2048, 1, 2, 4096, 13), (4096, 5, 5, 4096, 13), (4097, 5, 5, 4097, 14)):
        rows = _accepted(checker, 'resample', B=1, N=N, rate=rate, target_rate=target, M=M)
        assert rows == [rs_geometry(N, rate, target)] and rows[0][1:] == [logi, M]
    rows = _accepted(checker, 'resample', (4096, 4097), N=4097, rate=7, target_rate=7, M=4097)
    assert [r[1:] for r in rows] == [[13, 4096], [14, 4097]]


# ---- refusals: every reason of every family once ----------------------------------------------------------------------------
SIL_OK = dict(N=4100, B=2, rate=22050, block_size=220)
REFUSALS = [
    # (kind, lengths, settings, substrings of the message)
    ('reduce_noise', (), dict(B=2, N=100, null='audio'), ['bad argument']),
    ('reduce_noise', (), dict(B=2, N=100, null='out'), ['bad argument']),
    ('reduce_noise', (), dict(B=0, N=100), ['bad argument']),
    ('reduce_noise', (), dict(B=2, N=0), ['bad argument']),
    ('reduce_noise', (), dict(B=2, N=100, noise_len=0), ['noise_len = 0 < 1']),
    ('reduce_noise', (100, 0), dict(N=100), ['lengths[1] = 0 outside [1, N = 100]']),
    ('reduce_noise', (101, 5), dict(N=100), ['lengths[0] = 101 outside [1, N = 100]']),
    ('reduce_noise', (), dict(B=2, N=100, mem=7), ['bad mem kind 7']),
    ('trim', (), dict(B=2, N=100, null='audio'), ['bad argument']),
    ('trim', (), dict(B=2, N=100, null='out'), ['bad argument']),
    ('trim', (), dict(B=-1, N=100), ['bad argument']),
    ('trim', (), dict(B=2, N=100, window_length=1), ['window_length = 1 < 2']),
    ('trim', (), dict(B=2, N=100, mode=3), ['mode 3 not 0 (start_end), 1 (start) or 2 (end)']),
    ('trim', (), dict(B=2, N=100, threshold='nan'), ['threshold / margins must be finite']),
    ('trim', (), dict(B=2, N=100, add_end=-1), ['threshold / margins must be finite']),
    ('trim', (), dict(B=2, N=100, window_length=1000, add_start=1e7), ['not oversized']),
    ('trim', (), dict(B=2, N=100, mem=-1), ['bad mem kind -1']),
    ('trim', (0, 100), dict(N=100), ['lengths[0] = 0 outside [1, N = 100]']),
    ('trim', (100, 101), dict(N=100), ['lengths[1] = 101 outside [1, N = 100]']),
    ('resample', (), dict(B=1, N=100, M=100, null='out'), ['bad argument']),
    ('resample', (), dict(B=1, N=0, M=100), ['bad argument']),
    ('resample', (), dict(B=1, N=100, M=100, rate=0), ['rates must be > 0 (rate 0, target_rate 1)']),
    ('resample', (), dict(B=1, N=100, M=100, target_rate=-2), ['rates must be > 0']),
    ('resample', (), dict(B=1, N=(1 << 24) + 1, M=(1 << 24) + 1), ['> 2^24 samples per row']),
    ('resample', (), dict(B=1, N=1 << 24, rate=1 << 24, target_rate=(1 << 24) + 1, M=(1 << 24) + 1), ['give more than 2^24 samples']),
    ('resample', (), dict(B=1, N=1, rate=3, target_rate=2, M=0), ['give M = 0 < 1']),
    ('resample', (), dict(B=1, N=300, rate=16000, target_rate=22050, M=414), ['M = 414, but int(300 / 16000 * 22050) = 413']),
    ('resample', (300, 0), dict(N=300, rate=16000, target_rate=22050, M=413), ['lengths[1] = 0 outside [1, N = 300]']),
    ('resample', (301, 300), dict(N=300, rate=16000, target_rate=22050, M=413), ['lengths[0] = 301 outside [1, N = 300]']),
    ('resample', (300, 1), dict(N=300, rate=3, target_rate=2, M=200), ['lengths[1] = 1 resamples to 0 < 1 samples']),
    ('resample', (), dict(B=1, N=100, M=100, mem=2), ['bad mem kind 2']),
    ('silence', (), dict(SIL_OK, null='audio'), ['bad argument']),
    ('silence', (), dict(SIL_OK, null='lens'), ['bad argument']),
    ('silence', (), dict(SIL_OK, method=3), ['method 3 not 0 (rms), 1 (threshold) or 2 (mean-window)']),
    ('silence', (), dict(SIL_OK, mode=4), ['mode 4 not 0']),
    ('silence', (), dict(SIL_OK, mode=3, method=1), ['mode 3 (remove) belongs to the rms method (got method 1)']),
    ('silence', (), dict(SIL_OK, mode=3, method=2), ['mode 3 (remove) belongs to the rms method (got method 2)']),
    ('silence', (), dict(SIL_OK, rate=0), ['rate = 0 <= 0']),
    ('silence', (), dict(SIL_OK, B=65536, N=1), ['B = 65536 x N = 1 too large']),
    ('silence', (), dict(SIL_OK, B=1, N=(1 << 24) + 1), ['too large']),
    ('silence', (4100, 0), SIL_OK, ['lengths[1] = 0 outside [1, N = 4100]']),
    ('silence', (4101, 1), SIL_OK, ['lengths[0] = 4101 outside [1, N = 4100]']),
    ('silence', (), dict(SIL_OK, threshold='inf'), ['threshold = inf must be finite']),
    ('silence', (), dict(SIL_OK, method=1, threshold=-0.5), ['threshold = -0.5 must be finite and >= 0']),
    ('silence', (), dict(SIL_OK, block_size=0), ['block_size = 0 < 1']),
    ('silence', (), dict(SIL_OK, replace_by=-1), ['replace_by = -1 < 0']),
    ('silence', (), dict(SIL_OK, min_voice_time=-1), ['min_voice_time = -1 must be finite and >= 0']),
    ('silence', (), dict(SIL_OK, min_silence='nan'), ['min_silence = nan must be finite and >= 0']),
    ('silence', (), dict(SIL_OK, method=2, threshold=0), ['threshold = 0 <= 0 (mean-window)']),
    ('silence', (), dict(SIL_OK, method=2, min_silence=0.00001), ['window w = (int)(min_silence * rate) = 0 < 1']),
    ('silence', (4100, 3306), dict(SIL_OK, method=2, min_silence=0.15),
     ['a row of L = 3306 samples is shorter than the window w = 3307']),
    ('silence', (), dict(SIL_OK, method=2, min_silence=1e9), ['is shorter than the window w = 22050000000000']),
    ('silence', (), dict(SIL_OK, overlap=1), ['out overlaps audio']),
    ('silence', (), dict(SIL_OK, mem=5), ['bad mem kind 5']),
    # the FFT probe of the resampling chains (behind the rest: the ids of the cases above stay what they were)
    ('resample_fft', (), dict(lines=1, logL=6, null='audio'), ['bad argument']),
    ('resample_fft', (), dict(lines=1, logL=6, null='out'), ['bad argument']),
    ('resample_fft', (), dict(lines=1, logL=5), ['logL = 5 outside [6, 25]']),
    ('resample_fft', (), dict(lines=1, logL=26), ['logL = 26 outside [6, 25]']),
    ('resample_fft', (), dict(lines=0, logL=10), ['lines = 0 < 1']),
    ('resample_fft', (), dict(lines=-3, logL=10), ['lines = -3 < 1']),
    ('resample_fft', (), dict(lines=8, logL=25), ['lines = 8 x 2^25 points too large for 31-bit offsets']),
    ('resample_fft', (), dict(lines=(1 << 31) - 1, logL=25), ['too large for 31-bit offsets']),
]


@pytest.mark.parametrize('kind,lengths,settings,needles', REFUSALS)
def test_refusals(checker, kind, lengths, settings, needles):
    _refused(checker, kind, needles, lengths, **settings)


def test_the_31_bit_limits_at_the_first_batch_that_crosses_them(checker):
    # reduce_noise: the spectrum [B * Fr][2080] fp32 is the largest buffer; Fr is a grid dimension (<= 65535)
    N = 110250
    row = ceil_div(N + 2560, 512) * 2080 * 4
    B = (LIM - 1) // row
    assert _accepted(checker, 'reduce_noise', B=B, N=N) == [rn_geometry(B, N, 1)]
    _refused(checker, 'reduce_noise', [f'B = {B + 1} x N = {N} (noise_len 1) too large for 31-bit offsets'], B=B + 1, N=N)
    N = 65535 * 512 - 2560
    assert _accepted(checker, 'reduce_noise', B=1, N=N)[0][0] == 65535
    _refused(checker, 'reduce_noise', ['too large for 31-bit offsets'], B=1, N=N + 1)
    # ... and a noise clip longer than the audio makes the noise spectrum the largest
    nl = 1 << 20
    B = (LIM - 1) // (ceil_div(nl + 2048, 512) * 2080 * 4)
    assert _accepted(checker, 'reduce_noise', B=B, N=100, noise_len=nl)
    _refused(checker, 'reduce_noise', ['too large for 31-bit offsets'], B=B + 1, N=100, noise_len=nl)
    # trim_silence: the fp64 convolution rows [B][max(N, W) + 1]
    for N, wl in ((1000, 2), (10, 4001)):
        row = (max(N, 2 * (wl // 2)) + 1) * 8
        B = (LIM - 1) // row
        assert _accepted(checker, 'trim', B=B, N=N, window_length=wl)
        _refused(checker, 'trim', [f'B = {B + 1} x N = {N} too large for 31-bit offsets'], B=B + 1, N=N, window_length=wl)
    # resample: the rows in and out, 4 bytes a sample
    assert _accepted(checker, 'resample', B=255, N=1 << 20, rate=1, target_rate=2, M=1 << 21)
    _refused(checker, 'resample', ['(M 2097152) too large for 31-bit offsets'], B=256, N=1 << 20, rate=1, target_rate=2, M=1 << 21)
    assert _accepted(checker, 'resample', B=255, N=1 << 21, rate=2, target_rate=1, M=1 << 20)
    _refused(checker, 'resample', ['too large for 31-bit offsets'], B=256, N=1 << 21, rate=2, target_rate=1, M=1 << 20)
    # the FFT probe: lines of 2^logL complex fp32 points, 8 bytes each
    for logL in (6, 13, 22, 25):
        most = (LIM31 - 1) // (8 << logL)
        assert _accepted(checker, 'resample_fft', lines=most, logL=logL) == [[most * (8 << logL)]]
        _refused(checker, 'resample_fft', [f'lines = {most + 1} x 2^{logL} points too large'], lines=most + 1, logL=logL)
    # remove_silence: the rows, and B as a grid dimension
    assert _accepted(checker, 'silence', **dict(SIL_OK, B=31, N=1 << 24))
    _refused(checker, 'silence', ['B = 32 x N = 16777216 too large'], **dict(SIL_OK, B=32, N=1 << 24))
    assert _accepted(checker, 'silence', **dict(SIL_OK, B=65535, N=1))


def test_what_is_no_refusal(checker):
    # the mean-window's w equal to the shortest row; out next to audio but not inside it; both mem kinds
    assert _accepted(checker, 'silence', (4100, 3307), **dict(SIL_OK, method=2, min_silence=0.15))[0][3] == 3307
    for kind, settings in (('reduce_noise', dict(B=1, N=10)), ('trim', dict(B=1, N=10)), ('resample', dict(B=1, N=10, M=10)),
                           ('silence', SIL_OK)):
        for mem in (0, 1):
            assert _accepted(checker, kind, **dict(settings, mem=mem))


def test_refusal_precedence(checker):
    """One input that breaks two rules per family; the message is the one the check that stood first gave before the checks
    moved into audio_call.h:
      reduce_noise    arguments, noise_len, lengths[b], 31-bit limits, mem kind
      trim_silence    arguments, window_length, mode, threshold / margins, mem kind, lengths[b], 31-bit limits
      resample        arguments, rates, N, M against 2^24, M < 1, M != int(..), 31-bit limits, per row (lengths[b], then what it
                      resamples to), mem kind
      fft probe       arguments, logL, lines, 31-bit limit
      remove_silence  arguments, method, mode, mode 3 without rms, rate, size limits, lengths[b], threshold, rms settings,
                      min_silence, mean-window settings, out overlaps audio, mem kind"""
    _refused(checker, 'reduce_noise', ['noise_len = 0'], (0, 5), N=100, noise_len=0)
    _refused(checker, 'reduce_noise', ['lengths[0] = 0'], (0, 5), N=100, mem=7)
    _refused(checker, 'reduce_noise', ['31-bit'], B=1 << 20, N=110250, mem=7)
    _refused(checker, 'trim', ['bad mem kind 7'], (0, 5), N=100, mem=7)
    _refused(checker, 'trim', ['threshold / margins'], N=100, B=1, mem=7, add_start=-1)
    _refused(checker, 'trim', ['lengths[1] = 0'], (5, 0), N=1 << 24, window_length=1 << 29)
    _refused(checker, 'resample', ['M = 5, but'], (0, 5), N=300, rate=16000, target_rate=22050, M=5)
    _refused(checker, 'resample', ['31-bit'], (0,) * 256, N=1 << 21, rate=2, target_rate=1, M=1 << 20)
    _refused(checker, 'resample', ['lengths[0] = 1 resamples to 0'], (1, 301), N=300, rate=3, target_rate=2, M=200)
    _refused(checker, 'resample', ['lengths[1] = 0'], (300, 0), N=300, rate=3, target_rate=2, M=200, mem=9)
    _refused(checker, 'resample_fft', ['logL = 30'], lines=0, logL=30)
    _refused(checker, 'resample_fft', ['lines = 0'], lines=0, logL=25)
    _refused(checker, 'silence', ['mode 3 (remove)'], **dict(SIL_OK, mode=3, method=1, rate=0))
    _refused(checker, 'silence', ['too large'], (0, 5), **dict(SIL_OK, N=(1 << 24) + 1))
    _refused(checker, 'silence', ['lengths[0] = 0'], (0, 5), **dict(SIL_OK, method=2, threshold=0))
    _refused(checker, 'silence', ['shorter than the window'], **dict(SIL_OK, method=2, min_silence=1.0, overlap=1))
    _refused(checker, 'silence', ['out overlaps audio'], **dict(SIL_OK, overlap=1, mem=7))
