"""GPU half of the decoder-variant matrix (tests/decoder_cases.py): every case on every decoder machine that accepts it, in
both precisions (the attention-window cases included), against the numpy oracle -- fp32 calls against the fp32 oracle, fp16 calls against the oracle with the
same weights rounded to fp16 -- at the north-star bound and at the much tighter regression bounds of decoder_cases.py.

Each call first asserts that the requested machine really ran (a shape the machine does not accept, or an exchange
timeout, falls back to the per-step graph without any other sign); the engine's last error goes into the message."""
import numpy as np
import pytest

import decoder_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engines():
    """One engine per weight set, closed at module end."""
    from text_to_speech_amd.engine import HipEngine
    made = {}

    def get(case):
        key = dc.weights_key(case)
        if key not in made:
            eng = HipEngine(0)
            eng.load_state(dc.weights_of(case))
            eng.finalize()
            made[key] = eng
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def _last_error(eng):
    msg = eng._lib.tts_hip_last_error(eng._h)
    return msg.decode('utf-8', 'replace') if msg else ''


def _run(eng, case, machine, precision):
    tok, spk, masks = dc.inputs(case)
    eng.set_decoder_mode(machine)
    try:
        out = eng.tacotron2_infer(tok, speaker=spk, max_len=case.max_len, early_stopping=case.early_stopping,
                                  prenet_masks=masks, precision=precision, **case.win_kwargs)
        ran = eng.last_decoder_mode
    finally:
        eng.set_decoder_mode('auto')
    want = dc.pick_variant(machine, case.B, case.Tin, case.enc, precision).machine
    assert ran == want, f'{case.name} {precision}: asked for {machine}, expected {want}, ran {ran}; last error: ' \
                        f'{_last_error(eng)!r}'
    return out, eng.last_steps


def _errors(out, ref):
    e = {n: float(np.abs(getattr(out, n) - getattr(ref, n)).max()) for n in ('decoder_output', 'mel', 'stop_tokens')}
    e['attention_abs'] = float(np.abs(out.attention_weights - ref.attention_weights).max())
    e['attention_rms_rel'] = dc.attention_rms_rel(out.attention_weights, ref.attention_weights)
    return e


@pytest.mark.parametrize('name', [c.name for c in dc.CASES])
def test_decoder_variant_matches_oracle(engines, name):
    case = dc.CASE_BY_NAME[name]
    eng = engines(case)
    sens = dc.scripted(name)[1] if case.early_stopping else None
    stop_reg = dc.STOP_REG * sens if case.early_stopping else dc.MEL_REG
    failures, f32_out = [], {}
    for precision in ('f32', 'f16'):
        runs = dc.machines(case, precision) + [('auto', dc.pick_variant('auto', case.B, case.Tin, case.enc, precision))]
        for machine, variant in runs:
            out, steps = _run(eng, case, machine, precision)
            ref = dc.reference(case, dc.reference_kind(variant.machine, precision))
            e = _errors(out, ref)
            per_sens = f' ({e["stop_tokens"] / sens:.2e} per unit of gate norm {sens:.0f})' if sens else ''
            print(f'{name:16s} {precision} {machine:10s} {variant.machine} {variant.inst}'
                  f'{" two_pairs" if variant.two_pairs else ""}: frames {e["decoder_output"]:.2e} mel {e["mel"]:.2e} '
                  f'stop {e["stop_tokens"]:.2e}{per_sens} attention {e["attention_abs"]:.2e} abs, '
                  f'{e["attention_rms_rel"]:.2e} RMS-rel (bounds {dc.MEL_REG:.0e} / {dc.ATT_REG:.0e}, north star {dc.MEL_TOL:.0e})')
            tag = f'{precision} {machine}'
            want_steps = min(case.max_len, int(ref.lengths.max()) + 1) if case.early_stopping else case.max_len
            if not np.array_equal(out.lengths, ref.lengths) or steps != want_steps:
                failures.append(f'{tag}: lengths {out.lengths.tolist()} vs {ref.lengths.tolist()}, steps {steps} vs {want_steps}')
                continue
            for k, bound in (('decoder_output', dc.MEL_REG), ('mel', dc.MEL_REG), ('stop_tokens', stop_reg),
                             ('attention_abs', dc.MEL_TOL), ('attention_rms_rel', dc.ATT_REG)):
                if not e[k] <= bound:
                    failures.append(f'{tag}: {k} {e[k]:.3e} > {bound:.1e}')
            for b in range(case.B):
                if not np.all(out.attention_weights[b, :, dc.lens_of(case)[b]:] == 0):
                    failures.append(f'{tag}: row {b}: attention on padded positions')
            if case.win is not None:
                # exactly zero outside the window that the oracle's arg max of the step before puts around each step
                _, lo, hi = dc.window_bounds(case, ref.attention_weights[:, :steps])
                tau = np.arange(case.Tin)
                outside = (tau < lo[..., None]) | (tau > hi[..., None])
                bad = np.argwhere(outside & (out.attention_weights[:, :steps] != 0))
                if len(bad):
                    b, t, pos = bad[0]
                    failures.append(f'{tag}: {len(bad)} nonzero weights outside the window, first at row {b} step {t} position '
                                    f'{pos} (window {lo[b, t]} .. {hi[b, t]})')
            if case.early_stopping:
                for b, n in enumerate(ref.lengths):
                    d = float(np.abs(out.decoder_output[b, n] - ref.decoder_output[b, n]).max())
                    if not (d <= dc.MEL_REG and np.abs(out.decoder_output[b, n]).max() > 0):
                        failures.append(f'{tag}: row {b}: the firing frame {n} is off by {d:.2e}')
                if not (np.all(out.decoder_output[:, steps:] == 0) and np.all(out.attention_weights[:, steps:] == 0)):
                    failures.append(f'{tag}: frames after the last step are not zero')
            if precision == 'f32':
                f32_out[machine] = out
            else:
                # the flag is used: the same machine's fp32 output is outside the bound of the rounded-weight reference
                d = float(np.abs(f32_out[machine].mel - ref.mel).max())
                if d <= dc.MEL_REG:
                    failures.append(f'{tag}: the fp32 call is within {d:.2e} of the fp16 reference')
    assert not failures, '\n'.join(failures)
