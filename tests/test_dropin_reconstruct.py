"""The drop-in surface the reference's reconstruct / evaluate scripts use beside the model: the NTCD-TIMIT listing helpers
(packages/dataset/ntcd_timit.py) and the figure helper (packages/visualization.py)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_listing_helpers_equal_the_reference_on_data_subset(tmp_path):
    """packages/dataset/ntcd_timit.py (own pathlib implementation) returns exactly what the reference's functions returned on
    the reference's data/subset tree, for every split / size / label name the scripts use.  The tree is rebuilt from its recorded
    file names as empty files, the reference's return values are recorded (tests/golden/make_listing_golden.py)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("_mine_ntcd", os.path.join(ROOT, "packages", "dataset", "ntcd_timit.py"))
    mine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mine)
    with open(os.path.join(ROOT, "tests", "golden", "ntcd_listing_fixture.json")) as f:
        fix = json.load(f)
    for rel in fix["files"]:
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.touch()
    raw, proc = str(tmp_path) + "/raw/", str(tmp_path) + "/processed/"
    for split in ("train", "validation", "test", "other"):
        assert [list(v) for v in mine.speech_list(raw, split)] == fix["speech_list"][split]
        assert mine.video_list(raw, split) == fix["video_list"][split]
        for size in ("subset", "complete"):
            for up in (False, True):
                for lab in ("vad_labels", "ibm_labels"):
                    got = mine.proc_noisy_clean_pair_dict(proc, split, size, lab, up)
                    assert [list(kv) for kv in got.items()] == fix["pairs"][f"{split}|{size}|{int(up)}|{lab}"]
    assert len(mine.speech_list(raw, "test")[0]) == 3


def test_display_multiple_signals_draws_a_figure(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_own_visualization", os.path.join(ROOT, "packages", "visualization.py"))
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    display_multiple_signals = V.display_multiple_signals
    rng = np.random.default_rng(0)
    wave = rng.standard_normal(16000)
    tf = rng.standard_normal((513, 60)) + 1j * rng.standard_normal((513, 60))
    fig = display_multiple_signals([[wave, tf, None], [None, np.abs(tf), (rng.random((1, 60)) > 0.5).astype(np.float32)]],
                                   fs=16000, vmin=-40, vmax=20, wlen_sec=64e-3, hop_percent=0.25, xticks_sec=2.0, fontsize=30)
    out = tmp_path / "f.png"
    fig.savefig(str(out))
    assert out.stat().st_size > 10000
    import matplotlib.pyplot as plt
    plt.close(fig)
