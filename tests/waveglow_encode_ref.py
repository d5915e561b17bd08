"""Float64 restatement of WaveGlow's forward flow WITH its log-likelihood terms, for tests/test_waveglow_encode*.py.

`oracle.waveglow_ref.forward_flow` restates the flow (audio -> z) only; the engine's `waveglow_encode` also returns the three
sums the likelihood is made of.  This module returns both, built from the oracle's own pieces (`upsample`, `regroup`,
`wn_block` are imported, not copied), in the oracle's operation order, so that in float64 its z is `np.array_equal` to
`forward_flow`'s (tests/test_waveglow_encode.py).

    stats[0, b] = sum z^2 over all 8 channels
    stats[1, b] = sum over flows, positions and coupling channels of s
    stats[2, b] = positions * sum_k log|det kernel_k[0]|

`mistake=` plants one of MISTAKES, for the table that shows what each of them moves.
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
