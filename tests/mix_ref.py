"""The mixing arithmetic of the reference's scripts/create_test_set.py:95-115 (process_save_utt) restated in numpy, operation for
operation: tests/test_mix_cpu.py holds it to the recorded outputs of the reference itself (tests/golden/mix_golden.npz) bit for
bit, and tests/test_gpu_mix.py holds the device to it."""
import numpy as np

STATS = ("p", "Ps", "Pn", "k", "norm", "snr_db")             # the columns of the [U, 6] stats of dvae_mix_snr_batch


def snr_factor(snr_db):
    """np.power(10, -snr_dB / 10) as the reference calls it: one scalar at a time."""
    return np.power(10, -float(snr_db) / 10)


def mix_one(speech, bank, start, snr_db, normalise_speech=True):
    """speech: 1-D array; bank: the long noise recording; start: the first sample of the noise segment -> dict of the three float64
    outputs (speech, noise, mixture) and the scalars p, Ps, Pn, k, norm, snr_db (the achieved SNR of the outputs)."""
    speech = np.asarray(speech, np.float64)
    noise = np.asarray(bank, np.float64)[int(start):int(start) + len(speech)]
    assert len(noise) == len(speech), "the noise segment leaves its bank"
    with np.errstate(all="ignore"):
        p = np.max(abs(speech)) if normalise_speech else 1.0
        if normalise_speech:
            speech = speech / p
        else:
            speech = speech.copy()
        speech_power = np.sum(np.power(speech, 2))
        noise_power = np.sum(np.power(noise, 2))
        noise_power_target = speech_power * np.power(10, -float(snr_db) / 10)
        k = noise_power_target / noise_power
        noise = noise * np.sqrt(k)
        norm = np.max(abs(np.concatenate([speech, noise, speech + noise])))
        mixture = (speech + noise) / norm
        speech /= norm
        noise /= norm
        achieved = 10.0 * np.log10(np.sum(speech * speech) / np.sum(noise * noise))
    return dict(speech=speech, noise=noise, mixture=mixture, p=float(p), Ps=float(speech_power), Pn=float(noise_power), k=float(k),
                norm=float(norm), snr_db=float(achieved))


def load_golden(path):
    """tests/golden/mix_golden.npz -> {name: dict(speech, bank, seed, start, snr_db, out={s, n, x: recorded arrays or samples})}.
    A case stored whole has out[k] = {"whole": array}; the others {"head", "tail", "strided", "sums"} with the file's stride."""
    z = np.load(path)
    cases = {}
    for name in (str(n) for n in z["names"]):
        c = dict(speech=z[name + "/speech"], bank=z[name + "/bank"], seed=int(z[name + "/seed"]), start=int(z[name + "/start"]),
                 snr_db=float(z[name + "/snr_db"]), stride=int(z["stride"]), edge=int(z["edge"]), out={})
        for k in ("s", "n", "x"):
            if f"{name}/out_{k}" in z:
                c["out"][k] = {"whole": z[f"{name}/out_{k}"]}
            else:
                c["out"][k] = {part: z[f"{name}/out_{k}_{part}"] for part in ("head", "tail", "strided", "sums")}
        cases[name] = c
    return cases


def recorded_parts(v, case):
    """The parts of a whole output v that the fixture records for `case`, in the fixture's own form."""
    if "whole" in case["out"]["s"]:
        return {"whole": v}
    return {"head": v[:case["edge"]], "tail": v[-case["edge"]:], "strided": v[::case["stride"]],
            "sums": np.array([np.sum(v), np.sum(v * v)], np.float64)}
