"""CPU: the sentence pipeline over fake models reproduces tests/golden/pipeline_trace.json, scenario by scenario.

The fixture was recorded (scripts/make_pipeline_fixture.py) from the three modules of the commit before `tacotron2.py`,
`runtime.py` and `pipeline.py` were restructured: every synthesizer and vocoder call, callback, saver call, result,
`predicted` entry, engine call and running offset of tests/pipeline_cases.py's scenarios has to come out as it did there."""
import json
import os

import pytest

import pipeline_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pipeline_trace.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def traced():
    return json.loads(json.dumps(pipeline_cases.trace()))          # through JSON, like the fixture: tuples are lists there


def test_the_scenarios_take_the_paths_they_name(traced, golden):
    pipeline_cases.check_paths(traced)
    pipeline_cases.check_paths(golden)


@pytest.mark.parametrize('section', ['predict', 'refusals', 'runtime', 'pipeline', 'frame_cap'])
def test_trace_matches_the_recorded_one(traced, golden, section):
    got, want = traced[section], golden[section]
    if isinstance(want, dict):
        assert sorted(got) == sorted(want)
        for name in want:                                             # scenario by scenario: the first difference names its scenario
            assert got[name] == want[name], f'{section}: {name}'
    else:
        assert got == want
