"""Packed WaveGlow calls restated in numpy and plain Python (shared by tests/test_waveglow_packed*.py).

`packing_plan` is the host plan of tts_hip_waveglow_infer_packed (csrc/wg_call.h, wg_call_table; compared with it on the
CPU by tests/test_wg_call.py): the rows that hold frames
one after another in ONE row, `gap` zero frames between two of them, rows of length 0 without space and without gap.
`infer_packed` is oracle.waveglow_ref.infer on such a row with the frames that are not real held at 0 where the engine
holds them at 0: mel and z, the WN residual stream after the start conv and after every residual sum, the flow state after
every inverse 1x1 conv.  It is built from the oracle's functions; the oracle itself is not changed.
"""
import os
import re

import numpy as np

from oracle import waveglow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_gap_frames():
    """TTS_HIP_WG_GAP_FRAMES as include/tts_hip.h defines it."""
    src = open(os.path.join(ROOT, 'include', 'tts_hip.h')).read()
    found = re.findall(r'^#define\s+TTS_HIP_WG_GAP_FRAMES\s+(\d+)\s*$', src, flags=re.M)
    assert len(found) == 1, 'include/tts_hip.h must define TTS_HIP_WG_GAP_FRAMES once'
    return int(found[0])


def packing_plan(lengths, T, gap):
    """-> dict(starts [B] (0 for an empty row), F, flags [F] (1 + b * T + t on the packed frame that holds frame t of row b,
    0 on a gap frame), gaps (the gap frames, ascending))."""
    starts, flags, gaps = [], [], []
    first = True
    for b, n in enumerate(lengths):
        n = int(n)
        assert 0 <= n <= T
        if n == 0:
            starts.append(0)
            continue
        if not first:
            gaps.extend(range(len(flags), len(flags) + gap))
            flags.extend([0] * gap)
        first = False
        starts.append(len(flags))
        flags.extend(1 + b * T + t for t in range(n))
    return {'starts': starts, 'F': len(flags), 'flags': flags, 'gaps': gaps}


def wn_block_masked(a0, spect, w, prefix, real, n_layers=8, n_channels=512, collect=None, unmasked=()):
    """oracle.waveglow_ref.wn_block with the residual stream x times `real` after the start conv and each residual sum.
    `collect` (a list): gets the gated activations of every layer.  `unmasked`: the places where x is NOT multiplied -- 'start',
    or the index of a residual sum -- for the controls of tests/test_waveglow_variants.py that plant exactly that mistake."""
    x = a0 @ w[f'{prefix}/start_conv/kernel'][0] + w[f'{prefix}/start_conv/bias']
    if 'start' not in unmasked:
        x = x * real
    output = None
    for i in range(n_layers):
        in_act = R.conv1d_dilated_same(x, w[f'{prefix}/in_conv-{i}/kernel'], w[f'{prefix}/in_conv-{i}/bias'], 2 ** i)
        cond = spect @ w[f'{prefix}/cond_layer-{i}/kernel'][0] + w[f'{prefix}/cond_layer-{i}/bias']
        s = in_act + cond
        acts = np.tanh(s[..., :n_channels]) * R._sigmoid(s[..., n_channels:])
        if collect is not None:
            collect.append(acts)
        rs = acts @ w[f'{prefix}/res_skip_conv-{i}/kernel'][0] + w[f'{prefix}/res_skip_conv-{i}/bias']
        if i < n_layers - 1:
            x = rs[..., :n_channels] + x
            if i not in unmasked:
                x = x * real
            skip = rs[..., n_channels:]
        else:
            skip = rs
        output = skip if output is None else skip + output
    return output @ w[f'{prefix}/end_conv/kernel'][0] + w[f'{prefix}/end_conv/bias']


def infer_packed(mel, z, flags, w, cfg, dtype=np.float32, states=None, mask_z=True, mask_state=True):
    """mel [1, F, 80], z [1, F * 32, 8], flags [F] (non-zero = real) -> audio [F * 256]; what mel / z hold on a frame that is
    not real does not enter.  Works on any [B, F] batch with flags [B, F] as well (a ragged call: flags = t < lengths[b]).
    `states` (a dict): gets the flow state after flows 11, 8, 4 and 0, early outputs included.  mask_z / mask_state = False:
    z, or the state after every flow, is NOT cleared on the frames that are not real -- planted mistakes for the controls of
    tests/test_waveglow_variants.py."""
    w = {k: np.asarray(v, dtype) for k, v in w.items() if k.startswith('waveglow/')}
    keep = (np.asarray(flags) != 0).astype(dtype)
    keep = keep[None] if keep.ndim == 1 else keep
    mel = np.where(keep[:, :, None] != 0, np.asarray(mel, dtype), dtype(0))
    spect = R.regroup(R.upsample(mel, w['waveglow/upsample/kernel'], w['waveglow/upsample/bias'], cfg.upsample_stride),
                      cfg.n_group)
    real = np.repeat(keep, spect.shape[1] // keep.shape[1], axis=1)[:, :, None]
    z = np.where(real != 0, np.asarray(z, dtype), dtype(0)) if mask_z else np.asarray(z, dtype)
    n_rem = cfg.n_remaining_channels
    audio, z = z[:, :, :n_rem], z[:, :, n_rem:]
    for k in reversed(range(cfg.n_flows)):
        n_half = audio.shape[2] // 2
        a0, a1 = audio[:, :, :n_half], audio[:, :, n_half:]
        out = wn_block_masked(a0, spect, w, f'waveglow/block-{k}', real, cfg.n_layers, cfg.n_channels)
        a1 = (a1 - out[:, :, :n_half]) / np.exp(out[:, :, n_half:])
        audio = np.concatenate([a0, a1], axis=2) @ R.inv1x1_reverse_matrix(w[f'waveglow/invertible_conv-{k}/conv/kernel'])
        if mask_state:
            audio = audio * real
        if k % cfg.n_early_every == 0 and k > 0:
            audio = np.concatenate([z[:, :, :cfg.n_early_size], audio], axis=2)
            z = z[:, :, cfg.n_early_size:]
        if states is not None and k in (11, 8, 4, 0):
            states[k] = audio
    return audio.reshape(-1)
