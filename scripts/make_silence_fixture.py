"""Run the reference's rms, threshold and mean-window silence removal on the inputs of the silence tests and record what
it returns.

Run where the reference checkout exists:  python scripts/make_silence_fixture.py <reference root>
It imports utils/audio/audio_processing.py from there at run time (with stand-ins for the `loggers` package and, where
it is not installed, `librosa`, neither of which the three functions use; utils/wrappers.py is loaded from the reference)
and calls trim_silence_rms / trim_silence_simple / remove_silence on every case of tests/silence_ref.py: the deterministic
builder rows and the normalized tests/golden/audio_test_16k.wav.
Output: tests/golden/silence_fixture.json, per case the result's length and the sha256 of its float32 bytes, or the name of
the exception the reference raised (IndexError in the slice modes for a row without silence).
"""
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 2:
    sys.exit('usage: python scripts/make_silence_fixture.py <reference root>')
REF = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import silence_ref  # noqa: E402


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference(ref):
    _stand_in('loggers', timer=lambda fn=None, **kw: fn if fn is not None else (lambda f: f))
    try:
        import librosa.util  # noqa: F401
    except ImportError:
        _stand_in('librosa', util=_stand_in('librosa.util'))
    _stand_in('utils', __path__=[os.path.join(ref, 'utils')])
    _stand_in('utils.audio', __path__=[os.path.join(ref, 'utils', 'audio')])
    _load('utils.wrappers', os.path.join(ref, 'utils', 'wrappers.py'))
    return _load('utils.audio.audio_processing', os.path.join(ref, 'utils', 'audio', 'audio_processing.py'))


ap = load_reference(REF)
FUNCS = {'rms': ap.trim_silence_rms, 'threshold': ap.trim_silence_simple, 'remove': ap.remove_silence}

cases = {}
for name, inp, method, kw in silence_ref.CASES:
    rate, x = silence_ref.make_input(inp)
    try:
        y = FUNCS[method](x.copy(), rate=rate, **kw)
    except Exception as exc:                                       # recorded, not hidden: the tests pin its name
        cases[name] = {'raises': type(exc).__name__}
        continue
    y = np.ascontiguousarray(y)
    assert y.dtype == np.float32 and y.ndim == 1, (name, y.dtype, y.shape)
    cases[name] = {'len': int(y.shape[0]), 'sha256': hashlib.sha256(y.tobytes()).hexdigest()}

out = os.path.join(ROOT, 'tests', 'golden', 'silence_fixture.json')
with open(out, 'w') as f:
    json.dump({'cases': cases}, f, indent=0, sort_keys=True)
    f.write('\n')
raised = sorted(k for k, v in cases.items() if 'raises' in v)
print('wrote', out, os.path.getsize(out), 'bytes;', len(cases), 'cases;', len(raised), 'raise:', ', '.join(raised))
