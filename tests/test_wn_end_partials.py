"""CPU half of the end-partial-sum tests (tests/wn_end_cases.py): the cases reach the residual tile families they are named
for, and an oracle-only control of the bound the GPU half uses."""
import numpy as np
import pytest

import waveglow_cases as wc
import wn_end_cases as ec


def test_cases_reach_every_residual_tile_family():
    seen = set()
    for name, form, tiles, _ in ec.STATE_RUNS:
        case = wc.CASE_BY_NAME[name]
        v = wc.pick_variant(case.B, case.T, 'f32', form)
        assert v.tiles == tiles, f'{name} {form}: {v.tiles}'
        assert v.wino == (form == 'winograd'), f'{name} {form}: wino {v.wino}'
        seen.add(v.tiles)
    assert seen == {'64-row', '128x64', '128-row', '256-row'}
    for name, form in ec.ACTS_RUNS:
        case = wc.CASE_BY_NAME[name]
        assert wc.pick_variant(case.B, case.T, 'f32', form).wino == (form == 'winograd')


def test_split_sum_is_the_end_conv_and_a_dropped_partial_shows():
    """sum_{i<7} partial_i + layer 7 + bias, in float64, is the oracle's state after flow 11 (b5_t13, end_scale 0.2); without
    any one layer's partial the state moves by more than 1000 x STATE_REL -- a layer carries about an eighth of the skip
    sum, so the `end` output is off by a third of its size -- which the bound of the GPU test cannot miss."""
    case = wc.CASE_BY_NAME['b5_t13']
    ref = wc.states(case)[11]
    e = wc.state_errors(ec.state11(case), ref)
    print(f'split sum vs oracle: rel {e["rel"]:.2e} max_rel {e["max_rel"]:.2e}')
    assert e['rel'] <= 1e-12 and e['max_rel'] <= 1e-12
    for drop in range(7):
        e = wc.state_errors(ec.state11(case, drop=drop), ref)
        print(f'without the partial of layer {drop}: rel {e["rel"]:.2e} max_rel {e["max_rel"]:.2e}')
        assert e['rel'] > 1000 * wc.STATE_REL['f32'] and e['max_rel'] > 1000 * wc.STATE_MAX_REL['f32']
