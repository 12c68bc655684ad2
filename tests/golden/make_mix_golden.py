"""Golden outputs of the reference's scripts/create_test_set.py (process_save_utt with packages.dataset.qut_database.noise_segment)
on seeded inputs.  Build-container only (imports /root/reference):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mix_golden.py
Output: tests/golden/mix_golden.npz.

The script is loaded by path and its own functions are called; three preparations stand in for what is not installed here:
a stub `soundfile` whose read serves the stored arrays (as float64, what soundfile returns) and whose write captures the float64
arrays the script saves, a stub `librosa.core` (qut_database imports resample and never calls it on this path), and the module
global noise_audios, which the script's main() would fill, set by hand.  The segment start is the reference's own draw
(np.random.randint(len(bank) - len(speech)) from the global generator): seeded before the call, re-derived after it and recorded.

The inputs are STORED (float32, so that their float64 images are exact; one bank is float64) next to the outputs.  Whole outputs
of every case would make the file larger than the largest fixture part here (930 kB), so the cases longer than 100 samples record
the first and last 64 samples, every 23rd sample, and np.sum of each output and of its square."""
import importlib.util
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import numpy as np

STRIDE, EDGE, WHOLE_BELOW = 23, 64, 100
# (name, samples, snr_dB, seed, negative speech peak, float64 bank)
CASES = [
    ("n63", 63, -15.0, 1, False, False),
    ("n4096", 4096, 40.0, 2, False, False),
    ("n4097", 4097, 5.0, 3, False, True),
    ("n12289", 12289, -5.0, 4, True, False),
    ("n16000", 16000, 0.0, 5, False, False),
    ("n48000", 48000, -10.0, 6, False, False),
]


def make(n, seed, negative_peak, bank_f64):
    rng = np.random.default_rng(seed)
    env = np.repeat((rng.random(n // 800 + 1) > 0.4).astype(np.float64), 800)[:n] + 0.05
    speech = env * rng.standard_normal(n) * 0.1
    i = int(np.argmax(np.abs(speech)))
    speech[i] = (-1.25 if negative_peak else 1.25) * abs(speech[i])
    m = n + n // 8 + 17                                             # the bank: at most three times the utterance
    white = rng.standard_normal(m + 1)
    bank = 0.05 * (white[1:] + 0.7 * white[:-1])
    return speech.astype(np.float32), bank if bank_f64 else bank.astype(np.float32)


def load_reference(store, written):
    sf = types.ModuleType("soundfile")
    sf.read = lambda path: (np.array(store[path], np.float64), 16000)
    sf.write = lambda path, data, fs: written.__setitem__(path, np.array(data, copy=True))
    librosa, core = types.ModuleType("librosa"), types.ModuleType("librosa.core")
    core.resample = None
    librosa.core = core
    sys.modules.update({"soundfile": sf, "librosa": librosa, "librosa.core": core})
    spec = importlib.util.spec_from_file_location("create_test_set", os.path.join(REF, "scripts", "create_test_set.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    os.chdir(tempfile.mkdtemp())                                    # the script makes its output directories relative to the cwd
    store, written = {}, {}
    R = load_reference(store, written)
    out = {"names": np.array([c[0] for c in CASES]), "stride": np.array(STRIDE), "edge": np.array(EDGE)}
    for name, n, snr_db, seed, negative_peak, bank_f64 in CASES:
        speech, bank = make(n, seed, negative_peak, bank_f64)
        assert len(bank) <= 3 * n
        assert (speech[np.argmax(np.abs(speech))] < 0) == negative_peak
        store[R.input_speech_dir + name + ".wav"] = speech
        R.noise_audios = {"cafe": np.array(bank, np.float64)}
        np.random.seed(seed)
        R.process_save_utt([name + ".wav", name + ".wav", "cafe", snr_db])
        np.random.seed(seed)
        start = int(np.random.randint(len(bank) - len(speech)))
        got = {k: written[R.output_wav_dir + name + "_" + k + ".wav"] for k in ("s", "n", "x")}
        assert all(v.dtype == np.float64 and v.shape == (n,) for v in got.values())
        peak = max(np.max(np.abs(v)) for v in got.values())
        achieved = 10 * np.log10(np.sum(got["s"] ** 2) / np.sum(got["n"] ** 2))
        print(name, n, "start", start, "common peak", peak, "achieved SNR", achieved, "requested", snr_db)
        assert peak == 1.0 and abs(achieved - snr_db) < 1e-9
        out[name + "/speech"], out[name + "/bank"] = speech, bank
        out[name + "/seed"], out[name + "/start"], out[name + "/snr_db"] = np.array(seed), np.array(start), np.array(snr_db)
        for k, v in got.items():
            if n < WHOLE_BELOW:
                out[f"{name}/out_{k}"] = v
            else:
                out[f"{name}/out_{k}_head"], out[f"{name}/out_{k}_tail"] = v[:EDGE].copy(), v[-EDGE:].copy()
                out[f"{name}/out_{k}_strided"] = v[::STRIDE].copy()
                out[f"{name}/out_{k}_sums"] = np.array([np.sum(v), np.sum(v * v)], np.float64)
    path = os.path.join(HERE, "mix_golden.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "entries")


if __name__ == "__main__":
    main()
