"""Records what the reference's packages/dataset/ntcd_timit.py listing helpers return on the reference's data/subset tree, and the
file names of that tree, into tests/golden/ntcd_listing_fixture.json (names only: the test rebuilds the tree from empty files).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_listing_golden.py <reference checkout>
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    spec = importlib.util.spec_from_file_location("_ref_ntcd", os.path.join(ref, "packages", "dataset", "ntcd_timit.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    sub = os.path.join(ref, "data", "subset")
    raw, proc = sub + "/raw/", sub + "/processed/"
    files = []
    for top in ("raw", "processed"):
        for d, _, fs in os.walk(os.path.join(sub, top)):
            files += [os.path.relpath(os.path.join(d, f), sub) for f in fs]
    out = {"files": sorted(files), "speech_list": {}, "video_list": {}, "pairs": {}}
    for split in ("train", "validation", "test", "other"):
        out["speech_list"][split] = [list(v) for v in m.speech_list(raw, split)]
        out["video_list"][split] = m.video_list(raw, split)
        for size in ("subset", "complete"):
            for up in (False, True):
                for lab in ("vad_labels", "ibm_labels"):
                    out["pairs"][f"{split}|{size}|{int(up)}|{lab}"] = [list(kv) for kv in m.proc_noisy_clean_pair_dict(proc, split, size, lab, up).items()]
    path = os.path.join(HERE, "ntcd_listing_fixture.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
