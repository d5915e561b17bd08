"""CPU: the front end of a mel plan in C++ (csrc/audio_call.h: mel_cfg_check, what tts_hip_mel_fn_create refuses, and
mel_call_check, what a run or a probe refuses and the geometry it derives) against a restatement written here from the
contract in include/tts_hip.h.  The C++ side is the `mel_fn` kind of csrc/host_check.cpp's --audio-call mode, a stand-alone
program built with -fsanitize=address,undefined as tests/test_audio_call.py builds it: `lengths` is untrusted input."""
import pytest

import mel_fn_cases as M
from test_audio_call import LIM, _accepted, _refused, carved, ceil_div, checker      # noqa: F401  (checker: the fixture)

KINDS = {'tacotron': 0, 'whisper': 1}
NORMS = {None: 0, 'per_feature': 1, 'all_feature': 2}


def settings_of(cfg, **more):
    return dict(mel_kind=KINDS[cfg.kind], sampling_rate=cfg.sampling_rate, n_mel_channels=cfg.n_mel_channels,
                filter_length=cfg.filter_length, hop_length=cfg.hop_length, win_length=cfg.win_length,
                normalize_mode=NORMS[cfg.normalize_mode], mel_fmin=cfg.mel_fmin, mel_fmax=cfg.mel_fmax, pre_emph=cfg.pre_emph, **more)


def geometry(cfg, B, N, lengths):
    """The operand widths of the plan (K4 / Kpad: filter_length up to 4 / 32; NB, MAGK: 2 * bins, bins up to 32; gathered when
    the hop is no multiple of 4), the call's frames, padded widths and its workspace -- row facts [2][B] int, row maxima
    [B], padded rows [B][NP] (+ 256 bytes), gathered frames, spectrum, magnitudes, Whisper's linear mel -- and every row's
    frames."""
    fl, cut, whisper = cfg.filter_length, cfg.cut, cfg.kind == 'whisper'
    K4, Kpad, NB, MAGK, gathered = ceil_div(fl, 4) * 4, ceil_div(fl, 32) * 32, ceil_div(2 * cut, 32) * 32, ceil_div(cut, 32) * 32, \
        int(cfg.hop_length % 4 != 0)
    Fr = cfg.dft_frames(N)
    PW = max(N, cfg.win_length) + 2 * cfg.half
    NP = ceil_div(PW + K4 - fl, 4) * 4
    rows = B * Fr
    total = carved(8 * B, 4 * B, B * NP * 4 + 256, rows * Kpad * 4 if gathered else 0, rows * NB * 4, rows * MAGK * 4,
                   rows * cfg.n_mel_channels * 4 if whisper else 0)
    return [[K4, Kpad, NB, MAGK, gathered], [Fr, Fr - whisper, PW, NP, total], [cfg.frames(n) for n in lengths or [N] * B],
            [cfg.frames(N)]]


@pytest.mark.parametrize('config', list(M.CONFIGS))
def test_geometry(checker, config):
    cfg = M.CONFIGS[config]
    for n in M.lengths_of(cfg):
        assert _accepted(checker, 'mel_fn', B=1, N=n, **settings_of(cfg)) == geometry(cfg, 1, n, None), (config, n)
        assert _accepted(checker, 'mel_fn', B=2, N=n, mem=0, **settings_of(cfg)) == geometry(cfg, 2, n, None), (config, n)
    ragged = M.BY_NAME[f'{config}_ragged']
    assert _accepted(checker, 'mel_fn', ragged.lengths, N=ragged.N, **settings_of(cfg)) == geometry(cfg, 3, ragged.N, ragged.lengths)


def test_default_plan_frames(checker):
    for n in (1, 500, 1023, 1024, 1279, 1280, 22050):
        assert _accepted(checker, 'mel_fn', B=1, N=n)[3] == [max(n, 1024) // 256 + 1]


OK = dict(B=2, N=5000)
REFUSALS = [
    # (lengths, settings, substrings of the message), in the documented order: create, then run
    ((), dict(OK, null='cfg'), ['bad argument']),
    ((), dict(OK, mel_kind=2), ['kind 2 not 0 (tacotron) or 1 (whisper)']),
    ((), dict(OK, mel_kind=-1), ['kind -1 not 0']),
    ((), dict(OK, normalize_mode=3), ['normalize_mode 3 not 0 (none), 1 (per_feature) or 2 (all_feature)']),
    ((), dict(OK, normalize_mode=-1), ['normalize_mode -1 not 0']),
    ((), dict(OK, sampling_rate=0), ['sampling_rate = 0 < 1']),
    ((), dict(OK, filter_length=1, win_length=1), ['filter_length = 1 outside [2, 4096]']),
    ((), dict(OK, filter_length=4097), ['filter_length = 4097 outside [2, 4096]']),
    ((), dict(OK, win_length=0), ['win_length = 0 outside [1, filter_length = 1024]']),
    ((), dict(OK, win_length=1025), ['win_length = 1025 outside [1, filter_length = 1024]']),
    ((), dict(OK, hop_length=0), ['hop_length = 0 < 1']),
    ((), dict(OK, n_mel_channels=0), ['n_mel_channels = 0 outside [1, 1024]']),
    ((), dict(OK, n_mel_channels=1025), ['n_mel_channels = 1025 outside [1, 1024]']),
    ((), dict(OK, mel_fmin=-1), ['need 0 <= mel_fmin = -1 < mel_fmax = 8000 <= sampling_rate / 2 = 11025']),
    ((), dict(OK, mel_fmin=8000), ['need 0 <= mel_fmin = 8000 < mel_fmax = 8000']),
    ((), dict(OK, mel_fmax=11026), ['mel_fmax = 11026 <= sampling_rate / 2 = 11025']),
    ((), dict(OK, mel_fmax='nan'), ['need 0 <= mel_fmin']),
    ((), dict(OK, pre_emph=-0.5), ['pre_emph = -0.5 must be finite and >= 0']),
    ((), dict(OK, pre_emph='inf'), ['pre_emph = inf must be finite and >= 0']),
    ((), dict(OK, window='7:nan'), ['window[7] is not finite']),
    ((), dict(OK, window='1023:inf'), ['window[1023] is not finite']),
    ((), dict(OK, null='fn'), ['bad argument']),
    ((), dict(OK, null='audio'), ['bad argument']),
    ((), dict(OK, null='out'), ['bad argument']),
    ((), dict(OK, B=0), ['bad argument']),
    ((), dict(OK, N=0), ['bad argument']),
    ((5000, 0), dict(N=5000), ['lengths[1] = 0 outside [1, N = 5000]']),
    ((5001, 5), dict(N=5000), ['lengths[0] = 5001 outside [1, N = 5000]']),
    ((5000, 9), dict(N=5000, win_length=100), ['row 1: max(L = 9, win_length = 100) samples are not more than filter_length // 2 = 512']),
    ((), dict(B=1, N=512, win_length=512), ['row 0: max(L = 512, win_length = 512) samples are not more than filter_length // 2 = 512']),
    ((5000, 30), dict(N=5000, mel_kind=1, win_length=20, filter_length=40, hop_length=64), ['row 1: L = 30 samples give one frame']),
    ((), dict(OK, mem=7), ['bad mem kind 7']),
]


@pytest.mark.parametrize('lengths,settings,needles', REFUSALS)
def test_refusals(checker, lengths, settings, needles):
    _refused(checker, 'mel_fn', needles, lengths, **settings)


def test_what_is_no_refusal(checker):
    assert _accepted(checker, 'mel_fn', B=1, N=513, win_length=512)                     # L' one above filter_length // 2
    assert _accepted(checker, 'mel_fn', B=1, N=1, window='0:0.5')                       # an explicit window, a one-sample row
    assert _accepted(checker, 'mel_fn', (5000, 64), N=5000, mel_kind=1, win_length=20, filter_length=40, hop_length=64)  # two frames
    assert _accepted(checker, 'mel_fn', B=1, N=10, mel_fmax=11025, filter_length=2, win_length=1, hop_length=1, n_mel_channels=1024)
    assert _accepted(checker, 'mel_fn', B=1, N=10, filter_length=4096, win_length=4096, pre_emph=0)


def test_the_31_bit_limits_at_the_first_batch_that_crosses_them(checker):
    # the default plan: the spectrum [B * F][1056] fp32 is the largest buffer
    N = 220500
    row = (N // 256 + 1) * 1056 * 4
    B = (LIM - 1) // row
    assert _accepted(checker, 'mel_fn', B=B, N=N)[1][0] == N // 256 + 1
    _refused(checker, 'mel_fn', [f'B = {B + 1} x N = {N} too large for 31-bit offsets'], B=B + 1, N=N)
    # hop 1: one frame per sample; the gathered frames and the spectrum, both [B * F][1120], are the largest
    cfg = M.CONFIGS['gather']._replace(hop_length=1)
    row = cfg.dft_frames(4000) * 1120 * 4
    B = (LIM - 1) // row
    assert _accepted(checker, 'mel_fn', B=B, N=4000, **settings_of(cfg))
    _refused(checker, 'mel_fn', ['too large for 31-bit offsets'], B=B + 1, N=4000, **settings_of(cfg))
    # B is a grid dimension
    assert _accepted(checker, 'mel_fn', B=65535, N=1, filter_length=2, win_length=2, hop_length=1, n_mel_channels=1)
    _refused(checker, 'mel_fn', ['B <= 65535'], B=65536, N=1, filter_length=2, win_length=2, hop_length=1, n_mel_channels=1)


def test_refusal_precedence(checker):
    """One input that breaks two rules; the message is the one of the check documented first: create -- pointers, kind,
    normalize_mode, sampling_rate, filter_length, win_length, hop_length, n_mel_channels, mel_fmin / mel_fmax, pre_emph,
    window; then run -- pointers / B / N, lengths[b], a row reflect cannot pad, a Whisper row of one frame, the 31-bit limits,
    mem kind."""
    chain = [('mel_kind', 5, 'kind 5'), ('normalize_mode', 9, 'normalize_mode 9'), ('sampling_rate', 0, 'sampling_rate = 0'),
             ('filter_length', 1, 'filter_length = 1'), ('win_length', 2000, 'win_length = 2000'), ('hop_length', 0, 'hop_length = 0'),
             ('n_mel_channels', 0, 'n_mel_channels = 0'), ('mel_fmax', 99999, 'mel_fmax = 99999'), ('pre_emph', -1, 'pre_emph = -1'),
             ('window', '0:nan', 'window[0]'), ('N', 0, 'bad argument')]
    for i in range(len(chain) - 1):
        first, second = chain[i], chain[i + 1]
        if first[0] == 'filter_length':              # (filter_length = 1 also puts win_length = 1024 out of range: the next rule)
            second = chain[i + 2]
        _refused(checker, 'mel_fn', [first[2]], **{**OK, first[0]: first[1], second[0]: second[1]})
    _refused(checker, 'mel_fn', ['bad argument'], (0, 5), N=5000, null='audio')
    _refused(checker, 'mel_fn', ['lengths[0] = 0'], (0, 5), N=5000, win_length=100)
    _refused(checker, 'mel_fn', ['row 1: max(L = 5'], (5000, 5), N=5000, win_length=100, mem=7)
    _refused(checker, 'mel_fn', ['row 0: max(L = 5'], (5, 30), N=5000, mel_kind=1, win_length=20, filter_length=40, hop_length=64)
    _refused(checker, 'mel_fn', ['give one frame'], (30,) * 3, N=1 << 30, mel_kind=1, win_length=20, filter_length=40, hop_length=64)
    _refused(checker, 'mel_fn', ['31-bit'], B=1 << 20, N=220500, mem=7)
