"""Golden values of the reference's packages/metrics.py (si_sdr_components, energy_ratios, si_sdr_leroux) on seeded inputs.
Build-container only (imports /root/reference):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_metrics_golden.py
Output: tests/golden/metrics_golden.npz.  The inputs are STORED (float32: the reference then works on their exact float64
images, as it does on what soundfile reads from a 16-bit file) next to the reference's results on them."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

import numpy as np

from packages import metrics as R

# (name, samples, input SNR in dB, artefact level relative to the speech in dB, seed): s_hat = 0.8 s + 0.3 n + artefact
CASES = [
    ("n2", 2, 0.0, -20.0, 1),
    ("n63", 63, -15.0, -10.0, 2),
    ("n4097", 4097, 5.0, -30.0, 3),
    ("n8192", 8192, 40.0, -70.0, 4),
    ("n12289", 12289, -5.0, -5.0, 5),
    ("n16000a", 16000, 20.0, -40.0, 6),
    ("n16000b", 16000, -15.0, -25.0, 7),
]


def make(n, snr_db, art_db, seed):
    rng = np.random.default_rng(seed)
    env = np.repeat((rng.random(n // 800 + 1) > 0.4).astype(np.float64), 800)[:n] + 0.05
    s = env * rng.standard_normal(n) * 0.1
    noise = rng.standard_normal(n)
    noise *= np.linalg.norm(s) / np.linalg.norm(noise) * 10 ** (-snr_db / 20)
    art = rng.standard_normal(n)
    art *= np.linalg.norm(s) / np.linalg.norm(art) * 10 ** (art_db / 20)
    s, noise = s.astype(np.float32), noise.astype(np.float32)
    s_hat = (0.8 * s.astype(np.float64) + 0.3 * noise.astype(np.float64) + art).astype(np.float32)
    return s_hat, s, noise


def kappa(a, b):
    a, b = a.astype(np.longdouble), b.astype(np.longdouble)
    return float(np.sum(np.abs(a * b)) / abs(np.sum(a * b)))


def main():
    out = {"names": np.array([c[0] for c in CASES])}
    for name, n, snr_db, art_db, seed in CASES:
        s_hat, s, noise = make(n, snr_db, art_db, seed)
        ks, kn = kappa(s_hat, s), kappa(s_hat, noise)
        assert ks <= 1e3 and kn <= 1e3, (name, ks, kn)             # the condition the tests' error bounds are stated under
        a, b, c = (x.astype(np.float64) for x in (s_hat, s, noise))
        comps = R.si_sdr_components(a, b, c)
        out[name + "/s_hat"], out[name + "/s"], out[name + "/n"] = s_hat, s, noise
        out[name + "/energy_ratios"] = np.array(R.energy_ratios(a, b, c), np.float64)
        out[name + "/si_sdr_leroux"] = np.array(R.si_sdr_leroux(a, b), np.float64)
        # the components are recorded by their energies and a few samples (the arrays themselves would triple the file)
        out[name + "/component_energy"] = np.array([np.linalg.norm(x) ** 2 for x in comps], np.float64)
        out[name + "/component_head"] = np.stack([x[:2] for x in comps]).astype(np.float64)
        print(name, n, "kappa %.1f %.1f" % (ks, kn), out[name + "/energy_ratios"], float(out[name + "/si_sdr_leroux"]))
    path = os.path.join(HERE, "metrics_golden.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "entries")


if __name__ == "__main__":
    main()
