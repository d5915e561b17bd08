"""Full-size WaveGlow checkpoint of a given WN width in the Keras layout, written with the REAL HDF5 library (h5py), plus the
same tensors as .npz: what `make_h5_fixtures.py --full-waveglow` writes for the 512-channel model, for any `--channels`.
Run by tests/test_waveglow_channels_gpu.py with the interpreter that has h5py:

    /opt/conda/bin/python3.9 tests/golden/make_h5_waveglow_channels.py --full-waveglow <saving dir> [walk] --channels 256
"""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_h5_fixtures import keras_waveglow_paths  # noqa: E402


def write(out_dir, walk, channels):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    from text_to_speech_amd.config import WaveGlowConfig
    from text_to_speech_amd.weights import synth_waveglow
    w = synth_waveglow(WaveGlowConfig(n_channels=channels), seed=4321)
    table = keras_waveglow_paths(walk, n_flows=12, n_layers=8)
    assert sorted(table) == sorted(w)
    os.makedirs(out_dir, exist_ok=True)
    with h5py.File(os.path.join(out_dir, 'ckpt-0000.weights.h5'), 'w') as f:
        for tensor, path in table.items():
            f.create_dataset(path, data=w[tensor])
    np.savez(os.path.join(out_dir, 'tensors.npz'), **{k.replace('/', '|'): v for k, v in w.items()})


if __name__ == '__main__':
    rest = sys.argv[3:]
    if len(sys.argv) < 3 or sys.argv[1] != '--full-waveglow' or '--channels' not in rest:
        sys.exit(__doc__)
    write(sys.argv[2], 'walk' in rest, int(rest[rest.index('--channels') + 1]))
