"""Stores what tests/test_stft_oracle.py::test_oracle_reproduces_whole_reference_h5 compares: the whole int16 samples of the three
01M utterances of the reference's data/subset and the X_train / Y_train arrays of its Clean_ibm_labels_upsampled.h5 (outputs of the
reference's own pipeline), as tests/golden/stft_whole_fixture.part*.npz (data only).  The HDF5 file is read by a child interpreter
that has h5py (the second argument, default: this one):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_stft_whole_golden.py <reference checkout> [<python with h5py>]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # tests/
import golden_util as gu

UTTS = ("sa1", "sa2", "si462")


def main(ref, h5_python):
    sub = os.path.join(ref, "data", "subset")
    out = {}
    for u in UTTS:
        fs, w = wavfile.read(os.path.join(sub, "raw", "ntcd_timit", "Clean", "volunteers", "01M", "straightcam", u + ".wav"))
        assert fs == 16000 and w.dtype == np.int16
        out["01M_" + u + "_wav_i16"] = w
    h5 = os.path.join(sub, "processed", "ntcd_timit", "Clean_ibm_labels_upsampled.h5")
    with tempfile.TemporaryDirectory() as tmp:
        code = "import h5py, numpy as np, sys; f = h5py.File(sys.argv[1], 'r'); np.savez(sys.argv[2], X=f['X_train'][:], Y=f['Y_train'][:])"
        subprocess.check_call([h5_python, "-c", code, h5, os.path.join(tmp, "m.npz")])
        m = np.load(os.path.join(tmp, "m.npz"))
        out["X_train"] = m["X"]
        assert set(np.unique(m["Y"])) <= {0.0, 1.0}
        out["Y_train"] = m["Y"].astype(np.uint8)
    print("wrote", gu.save_golden("stft_whole_fixture", out))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else sys.executable)
