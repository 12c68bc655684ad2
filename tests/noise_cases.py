"""Cases shared by the CPU and GPU tests of the reparametrisation noise (oracle/noise_oracle.py).

EXTREME: counters whose Philox words sit on the edges of the uniform quantisation, found by find_extremes() below (run this file to
repeat the search: ~2^24 blocks, a few seconds) and committed as constants, so the device test can ask Trainer.noise() for exactly
these elements:

  radius_min   radius word with w >> 8 = 0         : u = 2^-25, the largest radius sqrt(50 ln 2) = 5.887
  radius_one   radius word with w >> 8 = 2^24 - 1  : u rounds to exactly 1.0f, radius 0 -- both outputs of that pair must be 0.0
  angle_one    angle word with w >> 8 = 2^24 - 1   : angle = 2 pi exactly as float32 rounds it: (cos, sin) = (1, ~0)

Each entry: (seed, step, frame, draw, pair) -- pair 0 = words 0 / 1 (outputs 0, 1 of the draw), pair 1 = words 2 / 3 (outputs 2, 3).
"""
import numpy as np

from oracle import noise_oracle as no

SEARCH_SEED = 7
SEARCH_FRAMES = 4096
TOP = (1 << 24) - 1

EXTREME = {
    "radius_min": [(7, 320, 1988, 2, 1), (7, 730, 2089, 0, 1)],
    "radius_one": [(7, 1081, 1311, 1, 1), (7, 1937, 4019, 3, 0)],
    "angle_one": [(7, 192, 2910, 3, 1), (7, 375, 3195, 1, 1)],
}


def find_extremes(seed=SEARCH_SEED, steps=range(1, 2049), frames=SEARCH_FRAMES, per_kind=2):
    """Scan (step, frame, draw) under one seed for words on the quantisation's edges; the first `per_kind` hits of each kind."""
    fr = np.arange(frames, dtype=np.uint64)
    found = {k: [] for k in EXTREME}
    for step in steps:
        for draw in range(4):
            k = no.words(seed, fr, step, draw) >> np.uint64(8)
            for kind, cols, val in (("radius_min", (0, 2), 0), ("radius_one", (0, 2), TOP), ("angle_one", (1, 3), TOP)):
                for c in cols:
                    for f in np.nonzero(k[:, c] == np.uint64(val))[0]:
                        found[kind].append((seed, step, int(f), draw, c >> 1))
        if all(len(v) >= per_kind for v in found.values()):
            break
    return {k: v[:per_kind] for k, v in found.items()}


def element_columns(draw, pair):
    """The two latent features that (draw, pair) fills."""
    f0 = no.DRAW_FEATURE0[draw] + 2 * pair
    return f0, f0 + 1


if __name__ == "__main__":
    for kind, hits in find_extremes().items():
        print(f'    "{kind}": {hits},')
