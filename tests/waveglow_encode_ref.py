"""Float64 restatement of WaveGlow's forward flow WITH its log-likelihood terms, for tests/test_waveglow_encode*.py.

`oracle.waveglow_ref.forward_flow` restates the flow (audio -> z) only; the engine's `waveglow_encode` also returns the three
sums the likelihood is made of.  This module returns both, built from the oracle's own pieces (`upsample`, `regroup`,
`wn_block` are imported, not copied), in the oracle's operation order, so that in float64 its z is `np.array_equal` to
`forward_flow`'s (tests/test_waveglow_encode.py).

    stats[0, b] = sum z^2 over all 8 channels
    stats[1, b] = sum over flows, positions and coupling channels of s
    stats[2, b] = positions * sum_k log|det kernel_k[0]|

`mistake=` plants one of MISTAKES, for the table that shows what each of them moves.

One flow at a time (tests/test_waveglow_encode_flows*.py): `init_step` and `flow_step` restate what the engine stores between two
flows -- the state with the NEXT flow's matrix already applied -- so that one flow of the engine can be compared on the engine's
own input to that flow; `chain` strings them together into everything `HipEngine.waveglow_encode_probe` can return, `StepCheck`
measures one (case, flow) of any such source against `flow_step` in units of the step's float32 floor.  FLOW_MISTAKES are
planted in `flow_step` / `chain`.
"""
import numpy as np

from oracle.waveglow_ref import regroup, upsample, wn_block

F32_EPS = 2.0 ** -24                # half a unit in the last place of a float32 of magnitude 1: what storing a result as float32 costs
MISTAKES = ('early_swapped', 'matrix_transposed', 'exp_minus_s', 'one_flow_s_left_out', 'log_det_signed', 'tail_counted')


_cast_cache = {}                    # id(array) -> (array, its float64 copy): the weights are 1 GB, a copy per run costs seconds


def _cast(w, dtype):
    """The WaveGlow tensors of `w` in `dtype`; float64 copies are made once per array and kept."""
    out = {}
    for k, v in w.items():
        if not k.startswith('waveglow/'):
            continue
        if v.dtype == dtype:
            out[k] = v
        elif dtype == np.float64:
            if id(v) not in _cast_cache:
                _cast_cache[id(v)] = (v, v.astype(np.float64))
            out[k] = _cast_cache[id(v)][1]
        else:
            out[k] = v.astype(dtype)
    return out


def log_abs_dets(w, cfg, dtype=np.float64):
    """log|det kernel_k[0]| of the twelve flows, in `dtype` arithmetic."""
    return np.array([np.linalg.slogdet(w[f'waveglow/invertible_conv-{k}/conv/kernel'][0].astype(dtype))[1]
                     for k in range(cfg.n_flows)])


def forward(audio, mel, w, cfg, dtype=np.float64, mistake=None):
    """audio [B, T*256], mel [B, T, 80] -> (z [B, T*32, 8] in `dtype`, stats [3, B] in `dtype`).  The sums are formed in float64
    from the `dtype` values, then stored as `dtype`: a float32 run shows the error of float32 values, not of a float32 sum."""
    assert mistake is None or mistake in MISTAKES
    w = _cast(w, dtype)
    spect = regroup(upsample(np.asarray(mel, dtype=dtype), w['waveglow/upsample/kernel'], w['waveglow/upsample/bias'],
                             cfg.upsample_stride), cfg.n_group)
    B, L, _ = spect.shape
    a = np.asarray(audio, dtype=dtype).reshape(B, L, cfg.n_group)
    early = []
    sum_s = np.zeros(B, dtype=np.float64)
    log_det = 0.0
    for k in range(cfg.n_flows):
        if k % cfg.n_early_every == 0 and k > 0:
            early.append(a[:, :, :cfg.n_early_size])
            a = a[:, :, cfg.n_early_size:]
        kernel = w[f'waveglow/invertible_conv-{k}/conv/kernel'][0]
        a = a @ (kernel.T if mistake == 'matrix_transposed' else kernel)
        sign, logabs = np.linalg.slogdet(kernel)
        if mistake == 'log_det_signed':
            with np.errstate(invalid='ignore'):
                log_det += float(np.log(sign * np.exp(logabs)))              # NaN where the determinant is negative
        else:
            log_det += float(logabs)
        n_half = a.shape[2] // 2
        a0, a1 = a[:, :, :n_half], a[:, :, n_half:]
        out = wn_block(a0, spect, w, f'waveglow/block-{k}', cfg.n_layers, cfg.n_channels)
        s = out[:, :, n_half:]
        a1 = np.exp(-s if mistake == 'exp_minus_s' else s) * a1 + out[:, :, :n_half]
        a = np.concatenate([a0, a1], axis=2)
        if not (mistake == 'one_flow_s_left_out' and k == 5):
            sum_s += s.sum(axis=(1, 2), dtype=np.float64)
    z = np.concatenate([a] + (early if mistake == 'early_swapped' else early[::-1]), axis=2)
    stats = np.stack([np.square(z.astype(np.float64)).sum(axis=(1, 2)), sum_s, np.full(B, L * log_det)])
    return z, stats.astype(dtype)


# ---- one flow at a time
FLOW_MISTAKES = ('early_wrong_end', 'zoff_swapped', 'next_transposed', 'next_old_n', 's_summed_over_b', 'slog_not_reset')


def spect_of(mel, w, cfg, dtype=np.float64):
    """The conditioning [B, T*32, 640] every flow's WN block reads, as `forward` forms it."""
    w = _cast(w, dtype)
    return regroup(upsample(np.asarray(mel, dtype=dtype), w['waveglow/upsample/kernel'], w['waveglow/upsample/bias'],
                            cfg.upsample_stride), cfg.n_group)


def init_step(audio, w, cfg, dtype=np.float64):
    """audio [B, T*256] -> the state entering flow 0: audio.reshape(B, L, 8) @ kernel_0."""
    w = _cast(w, dtype)
    B = audio.shape[0]
    return np.asarray(audio, dtype=dtype).reshape(B, -1, cfg.n_group) @ w['waveglow/invertible_conv-0/conv/kernel'][0]


def leaves_after(k, cfg):
    """Whether the first n_early_size channels leave between flow k and flow k + 1 (before flows 4 and 8)."""
    return (k + 1) % cfg.n_early_every == 0 and k + 1 < cfg.n_flows


def z_slot(k, cfg, mistake=None):
    """The channels of z that flow k's step writes: what leaves after flows 3 and 7 goes to 6:8 and 4:6 (latest first behind
    the final four), flow 11's state to 0:4; None for every other flow."""
    if k == cfg.n_flows - 1:
        return slice(0, cfg.n_remaining_channels)
    if not leaves_after(k, cfg):
        return None
    nth = (k + 1) // cfg.n_early_every - 1                              # 0 after flow 3, 1 after flow 7
    if mistake == 'zoff_swapped':
        nth = 1 - nth
    hi = cfg.n_group - nth * cfg.n_early_size
    return slice(hi - cfg.n_early_size, hi)


def flow_step(state_in, spect, w, cfg, k, dtype=np.float64, mistake=None):
    """One flow of `forward` on the state as the engine stores it.  state_in [B, L, n]: the state entering flow k, kernel_k
    already applied.  -> (state_out, early, s_sum): state_out is what flow k + 1 reads (the early channels dropped, kernel_k+1
    applied; after the last flow the final n_remaining channels), early [B, L, 2] the channels that leave before flows 4 and 8
    (else None), s_sum [B, L] float64 the position's sum of s over the coupling channels.  The operations are `forward`'s, in
    its order: chained from `init_step`, the float64 result is bit-equal to `forward`'s z.
    mistake: one of FLOW_MISTAKES ('zoff_swapped' and 'slog_not_reset' concern where a step's results go: see `chain`)."""
    assert mistake is None or mistake in FLOW_MISTAKES
    w = _cast(w, dtype)
    a = np.asarray(state_in, dtype=dtype)
    n_half = a.shape[2] // 2
    a0, a1 = a[:, :, :n_half], a[:, :, n_half:]
    out = wn_block(a0, spect, w, f'waveglow/block-{k}', cfg.n_layers, cfg.n_channels)
    s = out[:, :, n_half:]
    a1 = np.exp(s) * a1 + out[:, :, :n_half]
    a = np.concatenate([a0, a1], axis=2)
    s_sum = (out[:, :, :n_half] if mistake == 's_summed_over_b' else s).sum(axis=2, dtype=np.float64)
    if k == cfg.n_flows - 1:
        return a, None, s_sum
    early = None
    n_old = a.shape[2]
    if leaves_after(k, cfg):
        if mistake == 'early_wrong_end':
            early, a = a[:, :, -cfg.n_early_size:], a[:, :, :-cfg.n_early_size]
        else:
            early, a = a[:, :, :cfg.n_early_size], a[:, :, cfg.n_early_size:]
    kernel = w[f'waveglow/invertible_conv-{k + 1}/conv/kernel'][0]
    if mistake == 'next_transposed':
        kernel = kernel.T
    elif mistake == 'next_old_n':                                       # element (j, c) read at j * n_old + c; past the end: 0
        n = kernel.shape[0]
        flat = np.concatenate([kernel.ravel(), np.zeros(n * n_old, dtype=kernel.dtype)])
        kernel = flat[np.arange(n)[:, None] * n_old + np.arange(n)[None, :]]
    return a @ kernel, early, s_sum


def chain(audio, mel, w, cfg, dtype=np.float64, mistake=None, stale_slog=None):
    """init_step and the twelve flow_steps -> {'state': {-1 .. 11: the stored state after that step}, 'slog': {0 .. 11: the
    running per-position sum of s}, 'z': [B, L, 8]}: the answers of HipEngine.waveglow_encode_probe / waveglow_encode.
    mistake 'slog_not_reset': the running sum starts from stale_slog (what an earlier call left) instead of 0."""
    spect = spect_of(mel, w, cfg, dtype)
    state = {-1: init_step(audio, w, cfg, dtype)}
    B, L, _ = state[-1].shape
    z = np.zeros((B, L, cfg.n_group), dtype=dtype)
    run = np.zeros((B, L)) if mistake != 'slog_not_reset' else np.array(stale_slog, dtype=np.float64)
    slog = {}
    for k in range(cfg.n_flows):
        state[k], early, s_sum = flow_step(state[k - 1], spect, w, cfg, k, dtype, mistake)
        run = run + s_sum
        slog[k] = run
        if early is not None:
            z[:, :, z_slot(k, cfg, mistake)] = early
    z[:, :, z_slot(cfg.n_flows - 1, cfg)] = state[cfg.n_flows - 1]
    return {'state': state, 'slog': slog, 'z': z}


def _in_floors(err, floor):
    """err / floor; a floor of exactly 0 (channels the step only passes on: float32 loses nothing) allows only err == 0."""
    return err / floor if floor > 0 else (0.0 if err == 0 else float('inf'))


def row_groups(B, T, lengths=None):
    """[(rows, n)]: the rows of a batch by their number of real frames, empty rows left out."""
    if lengths is None:
        return [(list(range(B)), T)]
    return [([b for b in range(B) if lengths[b] == n], int(n)) for n in sorted(set(int(v) for v in lengths)) if n > 0]


class StepCheck:
    """One (inputs, flow k) comparison.  `state_in` is the source's own stored state after flow k - 1 (for k = -1: the audio as
    [B, L, 8]), groups [(rows, n)]: the batch rows (a list of b) whose first n frames are real, n > 0, each group run as a call
    of its own on those frames (`row_groups`), spect_groups[i][dtype] its conditioning (`spect_of` on mel[rows, :n]).  The float64 `flow_step` on that input is
    the reference, its float32 run the floor (RMS distance of state_out, of s_sum, of early / of flow 11's final channels, over
    the real positions): both from the restatement alone.  A source is allowed TEN floors (`Case`'s margin).  The channels that
    leave after flows 3 and 7 are a0 channels, which the coupling passes on untouched: their floor is exactly 0 and they must
    be the input's bits."""
    MARGIN = 10.0

    def __init__(self, state_in, spect_groups, w, cfg, k, groups):
        self.k, self.cfg, self.groups = k, cfg, groups
        ref, low = [], []
        for (rows, n), sp in zip(groups, spect_groups):
            x = np.asarray(state_in)[rows, :n * 32]
            if k < 0:
                ref.append((init_step(x.reshape(len(rows), -1), w, cfg, np.float64), None, None))
                low.append((init_step(x.reshape(len(rows), -1), w, cfg, np.float32), None, None))
            else:
                ref.append(flow_step(x, sp[np.float64], w, cfg, k, np.float64))
                low.append(flow_step(x, sp[np.float32], w, cfg, k, np.float32))
        cat = lambda runs, i: None if runs[0][i] is None else np.concatenate([r[i].reshape((-1,) + r[i].shape[2:]) for r in runs])
        self.ref = [cat(ref, i) for i in range(3)]                       # real positions of all rows, one after another
        self.floor = [None if r is None else rms(np.asarray(cat(low, i), dtype=np.float64) - r) for i, r in enumerate(self.ref)]

    def floor_of(self, quantity):
        """The floor of 'state', 'slog' or 'early' (at the last flow 'early' is the final channels: the state's floor)."""
        last = self.k == self.cfg.n_flows - 1
        return self.floor[{'state': 0, 'slog': 2, 'early': 0 if last else 1}[quantity]]

    def gather(self, x):
        """[B, T*32, ...] -> the real positions of the rows, one after another."""
        x = np.asarray(x, dtype=np.float64)
        return np.concatenate([x[rows, :n * 32].reshape((-1,) + x.shape[2:]) for rows, n in self.groups])

    def floors(self, state_out, slog_inc=None, z=None):
        """The source's results in floors: {'state', 'slog', 'early'} (what the step does not produce is absent).  state_out:
        its stored state after flow k; slog_inc: slog after flow k minus slog after flow k - 1 (slog after flow 0 itself); z:
        the plain call's z (read at flows 3, 7 and 11 only)."""
        out = {'state': _in_floors(rms(self.gather(state_out) - self.ref[0]), self.floor[0])}
        if self.k >= 0:
            out['slog'] = _in_floors(rms(self.gather(slog_inc) - self.ref[2]), self.floor[2])
        slot = z_slot(self.k, self.cfg) if self.k >= 0 else None
        if slot is not None:
            last = self.k == self.cfg.n_flows - 1
            want, floor = (self.ref[0], self.floor[0]) if last else (self.ref[1], self.floor[1])
            out['early'] = _in_floors(rms(self.gather(z)[:, slot] - want), floor)
        return out


def forward_ragged(audio, mel, lengths, w, cfg, dtype=np.float64, mistake=None):
    """The ragged contract: row b is a call of its own on its first lengths[b] frames; z is 0 behind them, an empty row's
    statistics are 0.  (audio / mel behind a row's length are not looked at.)  mistake 'tail_counted': the padded rows, their
    tails cleared, run whole and every position of a row is counted."""
    B, T = mel.shape[:2]
    if mistake == 'tail_counted':
        audio, mel = np.array(audio, dtype=dtype), np.array(mel, dtype=dtype)
        for b in range(B):
            audio[b, lengths[b] * 256:] = 0
            mel[b, lengths[b]:] = 0
        return forward(audio, mel, w, cfg, dtype)
    z = np.zeros((B, T * 32, 8), dtype=dtype)
    stats = np.zeros((3, B), dtype=dtype)
    for b in range(B):
        n = int(lengths[b])
        if n:
            zb, sb = forward(audio[b:b + 1, :n * 256], mel[b:b + 1, :n], w, cfg, dtype, mistake)
            z[b, :n * 32], stats[:, b] = zb[0], sb[:, 0]
    return z, stats


def replace_invertible_kernels(w, cfg, seed=5):
    """A copy of `w` whose invertible 1x1 kernels are Q1 diag(d) Q2 with d in [0.5, 2] and det < 0 in flows 1, 4, 7, 10.
    `weights.synth_waveglow` makes them orthogonal: every log|det| is 0 (to float32 rounding) and a transposed matrix is still
    an inverse-like, norm-preserving map, so stats[2] and layout mistakes that orthogonality forgives go untested on them."""
    rng = np.random.default_rng(seed)
    out = dict(w)
    for k in range(cfg.n_flows):
        name = f'waveglow/invertible_conv-{k}/conv/kernel'
        n = w[name].shape[1]
        q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
        q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
        m = q1 @ np.diag(rng.uniform(0.5, 2.0, n)) @ q2
        if (np.linalg.det(m) < 0) != (k % 3 == 1):
            m[:, 0] = -m[:, 0]
        out[name] = m.astype(np.float32)[None]
    return out


def rel_err(x, ref):
    """|x - ref| / |ref| elementwise; where ref is exactly 0: 0 if x is 0 too, else inf."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(ref == 0, np.where(x == 0, 0.0, np.inf), np.abs(x - ref) / np.abs(ref))


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, dtype=np.float64)))))


class Case:
    """One set of inputs with its float64 reference and its float32 floor, both from this restatement alone (never from the
    engine): z_floor = RMS(z of the float32 run - z64); stats_floor = the float32 run's relative error per statistic, and not
    below F32_EPS, the relative rounding of a result that is stored as one float32 -- a single number's float32 error can
    come out far below that by chance, a float32 output cannot.  An engine is allowed TEN times these floors."""

    def __init__(self, audio, mel, w, cfg, lengths=None):
        run = (lambda dt, mistake=None: forward(audio, mel, w, cfg, dt, mistake)) if lengths is None else \
              (lambda dt, mistake=None: forward_ragged(audio, mel, lengths, w, cfg, dt, mistake))
        self.run = run
        self.z, self.stats = run(np.float64)
        z32, stats32 = run(np.float32)
        self.z_floor = rms(z32 - self.z)
        self.stats_floor = np.maximum(rel_err(stats32, self.stats), F32_EPS)
        for a in (self.z, self.stats, self.stats_floor):
            a.setflags(write=False)

    @property
    def z_bound(self):
        return 10.0 * self.z_floor

    @property
    def stats_bound(self):
        return 10.0 * self.stats_floor

    def errors(self, z, stats):
        """(RMS error of z, relative error [3, B] of the statistics) of a result against the float64 reference."""
        return rms(np.asarray(z, dtype=np.float64) - self.z), rel_err(stats, self.stats)
