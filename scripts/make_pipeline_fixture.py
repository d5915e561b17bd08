"""Run the scenarios of tests/pipeline_cases.py and record what the fake models, callbacks and callers saw.

    python scripts/make_pipeline_fixture.py [<directory holding tacotron2.py, runtime.py and pipeline.py>]

Without an argument the package's own three modules are traced.  With one, the three files in that directory stand in for
`text_to_speech_amd.tacotron2`, `.runtime` and `.pipeline` (the rest of the package is the checkout's): copy the three
modules of the commit to compare against aside (`git show <commit>:text_to_speech_amd/tacotron2.py > aside/tacotron2.py`,
...) and name that directory.  tests/golden/pipeline_trace.json was written that way from the commit before the sentence
pipeline was restructured, so tests/test_pipeline_trace.py holds the restructured code to what that commit did.
Output: tests/golden/pipeline_trace.json, one scenario per line.
"""
import importlib.util
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
if len(sys.argv) > 2:
    sys.exit('usage: python scripts/make_pipeline_fixture.py [<directory with tacotron2.py, runtime.py, pipeline.py>]')

import text_to_speech_amd  # noqa: E402

if len(sys.argv) == 2:
    for name in ('runtime', 'pipeline', 'tacotron2'):               # (runtime first: the others may import it)
        full = 'text_to_speech_amd.' + name
        spec = importlib.util.spec_from_file_location(full, os.path.join(sys.argv[1], name + '.py'))
        module = importlib.util.module_from_spec(spec)
        sys.modules[full] = module
        spec.loader.exec_module(module)
        setattr(text_to_speech_amd, name, module)

import pipeline_cases  # noqa: E402

logging.getLogger('text_to_speech_amd').addHandler(logging.NullHandler())   # the scenarios provoke warnings: not printed
trace = pipeline_cases.trace()
pipeline_cases.check_paths(trace)                                   # every scenario took the path it names

out = os.path.join(ROOT, 'tests', 'golden', 'pipeline_trace.json')
with open(out, 'w') as f:
    pipeline_cases.dump(trace, f)
print('wrote', out, os.path.getsize(out), 'bytes;', {k: len(v) for k, v in trace.items()})
