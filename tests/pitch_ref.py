"""Float64 restatement of the pitch calls (include/tts_hip.h: tts_hip_pitch, tts_hip_f0_error): frames, difference, normalised
difference, pick, interpolation, the three planes, the F0 comparison, and the bounds the GPU tests hold the kernels to.

Every function takes a `mistake=` name: one of MISTAKES planted into that stage, so that tests/test_pitch.py can show that each
bound lies a factor ten below what the mistake changes.
"""
import numpy as np

EPS = 2.0 ** -24                     # unit roundoff of float32
MARGIN = 1e-4                        # what a STABLE decision keeps clear of, in float64

MISTAKES = ('window_start', 'read_past_length', 'prefix_shifted', 'no_tau_factor', 'threshold_le', 'no_walk', 'argmin_last',
            'delta_sign', 'delta_on_d', 'no_delta', 'natural_log', 'pair_transposed', 'vuv_counts_unvoiced')


def frame_count(n, hop):
    return 1 + int(n) // int(hop)


def frames(x, length, hop, win, tau_max, mistake=None):
    """[F_b, win + tau_max] float64: frame t holds x[s + j], s = t hop - win // 2, zeros outside [0, length)."""
    x = np.asarray(x)
    F = frame_count(length, hop)
    s = np.arange(F)[:, None] * hop - win // 2 + np.arange(win + tau_max)[None, :]
    if mistake == 'window_start':
        s = s + 1
    end = len(x) if mistake == 'read_past_length' else length
    ok = (s >= 0) & (s < end)
    return np.where(ok, x[np.clip(s, 0, len(x) - 1)].astype(np.float64), 0.0)


def difference(fr, win, tau_max):
    """d [F, tau_max + 1]: d(tau) = sum_{j < win} (x[j] - x[j + tau])^2"""
    d = np.empty((fr.shape[0], tau_max + 1))
    for tau in range(tau_max + 1):
        d[:, tau] = ((fr[:, :win] - fr[:, tau:tau + win]) ** 2).sum(1)
    return d


def cmnd(d, mistake=None):
    """d' [F, lags]: d'(0) = 1, d'(tau) = d(tau) tau / S(tau), S(tau) = d(1) + ... + d(tau); 1 where S(tau) = 0"""
    d = np.asarray(d, dtype=np.float64)
    tau = np.arange(d.shape[1], dtype=np.float64)
    S = np.cumsum(d[:, 1:], axis=1)
    S = np.concatenate([np.zeros((d.shape[0], 1)), S], axis=1)
    if mistake == 'prefix_shifted':                  # the sum taken one lag short: S(tau) = d(0) + ... + d(tau - 1)
        S = np.concatenate([np.zeros((d.shape[0], 1)), S[:, :-1]], axis=1)
    num = d if mistake == 'no_tau_factor' else d * tau
    with np.errstate(divide='ignore', invalid='ignore'):
        out = np.where(S == 0, 1.0, num / np.where(S == 0, 1.0, S))
    out[:, 0] = 1.0
    return out


def pick(dp, tau_min, tau_max, threshold, mistake=None):
    """(voiced bool [F], tau* int [F]) of the documented rule on d' [F, tau_max + 1]"""
    dp = np.asarray(dp, dtype=np.float64)
    thr = float(np.float32(threshold))
    voiced, taus = np.zeros(len(dp), bool), np.zeros(len(dp), np.int64)
    for f, q in enumerate(dp):
        seg = q[tau_min:tau_max + 1]
        below = np.nonzero(seg <= thr if mistake == 'threshold_le' else seg < thr)[0]
        if len(below):
            tau = tau_min + int(below[0])
            while mistake != 'no_walk' and tau + 1 <= tau_max and q[tau + 1] < q[tau]:
                tau += 1
            voiced[f] = True
        else:
            tau = tau_min + (len(seg) - 1 - int(np.argmin(seg[::-1])) if mistake == 'argmin_last' else int(np.argmin(seg)))
        taus[f] = tau
    return voiced, taus


def planes(dp, voiced, taus, rate, tau_max, d=None, mistake=None):
    """(f0, period, aperiodicity), float64 [F] each, from d' (float32 values when they are the run's own), the pick and `rate`"""
    dp = np.asarray(dp, dtype=np.float64)
    src = np.asarray(d, dtype=np.float64) if mistake == 'delta_on_d' else dp
    f0, period, ap = np.zeros(len(dp)), np.zeros(len(dp)), np.zeros(len(dp))
    for f, tau in enumerate(taus):
        delta = 0.0
        if tau - 1 >= 1 and tau + 1 <= tau_max and mistake != 'no_delta':
            a, b, c = src[f, tau - 1], src[f, tau], src[f, tau + 1]
            if a - 2 * b + c > 0:
                delta = (a - c) / (2 * (a - 2 * b + c))
                if mistake == 'delta_sign':
                    delta = -delta
        period[f] = tau + delta
        f0[f] = rate / period[f] if voiced[f] else 0.0
        ap[f] = dp[f, tau]
    return f0, period, ap


def track(x, length, *, rate, hop, win, tau_min, tau_max, threshold, mistake=None):
    """Everything of one row in float64 -> dict(frames, d, dp, voiced, tau, f0, period, aperiodicity), F_b rows each"""
    fr = frames(x, length, hop, win, tau_max, mistake)
    d = difference(fr, win, tau_max)
    dp = cmnd(d, mistake)
    voiced, taus = pick(dp, tau_min, tau_max, threshold, mistake)
    f0, period, ap = planes(dp, voiced, taus, rate, tau_max, d, mistake)
    return dict(frames=fr, d=d, dp=dp, voiced=voiced, tau=taus, f0=f0, period=period, aperiodicity=ap)


def track32(x, length, *, rate, hop, win, tau_min, tau_max, threshold):
    """The same row with the float32 stages done in float32 (numpy: sequential sums, no fused multiply-add): what the distance of
    a float32 implementation from `track` is measured with -> dict(voiced, tau, f0)"""
    fr = frames(x, length, hop, win, tau_max).astype(np.float32)
    d = np.empty((fr.shape[0], tau_max + 1), np.float32)
    for tau in range(tau_max + 1):
        d[:, tau] = np.cumsum((fr[:, :win] - fr[:, tau:tau + win]) ** 2, axis=1, dtype=np.float32)[:, -1]
    S = np.concatenate([np.zeros((len(d), 1), np.float32), np.cumsum(d[:, 1:], axis=1, dtype=np.float32)], axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        dp = np.where(S == 0, np.float32(1), d * np.arange(tau_max + 1, dtype=np.float32) / np.where(S == 0, np.float32(1), S))
    dp = dp.astype(np.float32)
    dp[:, 0] = 1
    voiced, taus = pick(dp, tau_min, tau_max, threshold)
    f0, _, _ = planes(dp, voiced, taus, rate, tau_max)
    return dict(voiced=voiced, tau=taus, f0=f0.astype(np.float32).astype(np.float64))


def stable(d, dp, tau_min, tau_max, threshold, margin=MARGIN):
    """bool [F]: a frame's decision is STABLE when, in float64, these margins are at least `margin`: |d' - threshold| for every
    lag examined up to the crossing (unvoiced: for every lag of the range), and every difference the walk or the argmin decides
    (the walk: each step it takes and the one it refuses; the argmin: d' of every other lag of the range above the minimum).
    Two lags whose S is 0 do not count against the argmin: there d' is 1 by rule, and S = 0 means every term of every d up to
    that lag is an exact zero, in float32 as in float64 -- both decide that tie by the smallest-tau rule."""
    thr = float(np.float32(threshold))
    S = np.concatenate([np.zeros((len(d), 1)), np.cumsum(np.asarray(d, np.float64)[:, 1:], axis=1)], axis=1)
    ok = np.zeros(len(dp), bool)
    for f, q in enumerate(np.asarray(dp, np.float64)):
        seg = q[tau_min:tau_max + 1]
        below = np.nonzero(seg < thr)[0]
        if len(below):
            tau = tau_min + int(below[0])
            good = np.abs(q[tau_min:tau + 1] - thr).min() >= margin
            while tau + 1 <= tau_max and q[tau + 1] < q[tau]:
                good &= q[tau] - q[tau + 1] >= margin
                tau += 1
            if tau + 1 <= tau_max:
                good &= q[tau + 1] - q[tau] >= margin
        else:
            good = np.abs(seg - thr).min() >= margin
            k = int(np.argmin(seg))
            others = np.delete(seg, k)
            by_rule = np.delete(S[f, tau_min:tau_max + 1] == 0, k) & (S[f, tau_min + k] == 0)
            gaps = (others - seg[k])[~by_rule]
            good &= len(gaps) == 0 or gaps.min() >= margin
        ok[f] = good
    return ok


def f0_error(f0_a, f0_b, la, lb, path=None, gross_cents=1200 * np.log2(1.2), mistake=None):
    """One row in float64 -> [pairs, voiced_pairs, rmse_cents, mean_cents, vuv_errors, gross_errors]"""
    gross = float(np.float32(gross_cents))
    if path is None:
        path = [(t, t) for t in range(min(la, lb))]
    pairs = both = one = n_gross = 0
    cents = []
    for i, j in path:
        if mistake == 'pair_transposed':
            i, j = j, i
        if i < 0 or i >= la or j < 0 or j >= lb:
            break
        pairs += 1
        a, b = float(f0_a[i]), float(f0_b[j])
        va, vb = a > 0, b > 0
        if va and vb:
            c = 1200.0 * (np.log(a / b) if mistake == 'natural_log' else np.log2(a / b))
            cents.append(c)
            both += 1
            n_gross += abs(c) > gross
        elif va != vb or mistake == 'vuv_counts_unvoiced':
            one += 1
    cents = np.asarray(cents)
    return np.array([pairs, both, np.sqrt((cents ** 2).mean()) if both else 0.0, cents.mean() if both else 0.0, one, n_gross], np.float64)


# ---- the bounds (first order in EPS; how each is derived: DESIGN 4.3g)
def bound_d(d, win):
    """|d - float64 d| on the same float32 samples: each difference rounds once (2 EPS on its square), each of the win
    accumulations once, all terms non-negative"""
    return (win + 4) * EPS * np.asarray(d, np.float64)


def bound_cmnd(dp):
    """|d' - float64 d'| on the run's own d: the prefix S(tau) has at most tau roundings (a blocked scan far fewer), the product
    and the quotient one each"""
    dp = np.asarray(dp, np.float64)
    return (np.arange(dp.shape[-1]) + 4) * EPS * dp


def bound_rounded(v, roundings):
    return roundings * EPS * np.abs(np.asarray(v, np.float64))
