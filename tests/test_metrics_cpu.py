"""Host side of the scorer (no GPU): packages.metrics on host arrays against the reference's recorded values
(tests/golden/metrics_golden.npz, written by tests/golden/make_metrics_golden.py), the offset table of dvae_si_ratios_batch
(ratio_tables) with every refusal, and trim.

Bounds: the drop-in functions run numpy on the host like the reference, but are not required to round like it operation for
operation, so both sides are held to the reference's own worst case against the exact value (tests/metrics_bounds.py: ref_db, n u
per sum in any order): |got - recorded| <= 2 ref_db.  On the fixture that is 5.6e-14 dB (n = 2) ... 6.3e-9 dB (n = 16 000, kappa_n = 14,
SI-SAR +38 dB); the recorded values themselves lie within ref_db of the long-double evaluation, which is asserted first."""
import importlib
import os

import numpy as np
import pytest
import torch

import metrics_bounds as MB
from packages import metrics as PM

M = importlib.import_module("disentangled-vae_amd.metrics")
FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics_golden.npz"))
NAMES = [str(n) for n in FIX["names"]]


def case(name):
    return tuple(FIX[f"{name}/{k}"].astype(np.float64) for k in ("s_hat", "s", "n"))


@pytest.mark.parametrize("name", NAMES)
def test_recorded_values_lie_inside_the_reference_bound(name):
    sh, s, n = case(name)
    q = MB.exact(sh, s, n)
    MB.check_kappa(q)
    b = MB.ref_db(q)
    rec = FIX[name + "/energy_ratios"]
    for i, (ratio, _) in enumerate(MB.RATIOS):
        print(name, ratio, "recorded - exact", rec[i] - q[ratio], "bound", b[ratio])
        assert abs(rec[i] - q[ratio]) <= b[ratio], (name, ratio)
    assert abs(float(FIX[name + "/si_sdr_leroux"]) - q["si_sdr"]) <= b["si_sdr"]


@pytest.mark.parametrize("name", NAMES)
def test_dropin_functions_on_host_arrays(name):
    sh, s, n = case(name)
    b = MB.ref_db(MB.exact(sh, s, n))
    got = PM.energy_ratios(sh, s, n)
    rec = FIX[name + "/energy_ratios"]
    assert len(got) == 3 and all(isinstance(g, float) for g in got)
    for i, (ratio, _) in enumerate(MB.RATIOS):
        print(name, ratio, "got - recorded", got[i] - rec[i], "bound", 2 * b[ratio])
        assert abs(got[i] - rec[i]) <= 2 * b[ratio], (name, ratio)
    leroux = PM.si_sdr_leroux(sh, s)
    assert abs(leroux - float(FIX[name + "/si_sdr_leroux"])) <= 2 * b["si_sdr"]
    comps = PM.si_sdr_components(sh, s, n)
    assert [c.shape for c in comps] == [sh.shape] * 3 and all(c.dtype == np.float64 for c in comps)
    # the components' energies against the recorded ones: each within twice the bound of its own energy
    e = MB.relative(MB.exact(sh, s, n), MB.gamma_ref(sh.size))
    for c, rec_e, key in zip(comps, FIX[name + "/component_energy"], ("s_target", "e_noise", "e_art")):
        assert abs(np.linalg.norm(c) ** 2 - rec_e) <= 2 * e[key] * rec_e, (name, key)
    # s_hat = s_target + e_noise + e_art, sample by sample (three roundings of magnitudes up to |s_hat| + |s_target| + |e_noise|)
    mag = np.abs(sh) + np.abs(comps[0]) + np.abs(comps[1])
    assert np.all(np.abs(comps[0] + comps[1] + comps[2] - sh) <= 4 * MB.U * 2 * mag)


def test_dropin_accepts_host_tensors_and_float32():
    sh, s, n = case("n4097")
    want = PM.energy_ratios(sh, s, n)
    assert PM.energy_ratios(torch.from_numpy(sh), torch.from_numpy(s), torch.from_numpy(n)) == want
    f32 = PM.energy_ratios(*(FIX[f"n4097/{k}"] for k in ("s_hat", "s", "n")))              # float32 in: numpy computes in float32
    assert np.allclose(f32, want, atol=1e-2)


def test_degenerate_inputs_follow_numpy():
    s = np.array([1.0, -2.0, 0.5])
    with np.errstate(all="ignore"):
        assert PM.si_sdr_leroux(2.0 * s, s) == np.inf                                    # a perfect estimate
        assert np.isnan(PM.si_sdr_leroux(s, np.zeros(3)))                                 # all-zero s
        sdr, sir, sar = PM.energy_ratios(s, s, np.zeros(3))                               # all-zero n
        assert np.isnan(sir) and np.isnan(sar) and np.isnan(sdr)


# ---- the table ---------------------------------------------------------------------------------------------------------------------

def test_ratio_tables_layout():
    lengths = [1, 4096, 4097, 80000]
    off_a = [0, 64, 4160 + 3, 9000]
    off_b = [5, 6, 5000, 10000]
    off_c = [0, 1, 4097, 8194]
    tab = M.ratio_tables([(off_a, lengths), (off_b, lengths), (off_c, lengths)], [90000, 90000, 90000])
    U = 4
    assert tab.dtype == np.int64 and tab.size == 5 * U + 1
    assert tab[:U + 1].tolist() == [0, 1, 2, 4, 24]                                       # ceil(len / 4096) items each
    assert tab[U + 1:2 * U + 1].tolist() == off_a and tab[2 * U + 1:3 * U + 1].tolist() == off_b
    assert tab[3 * U + 1:4 * U + 1].tolist() == off_c and tab[4 * U + 1:].tolist() == lengths
    two = M.ratio_tables([(off_a, lengths), (off_b, lengths)], [90000, 90000])
    assert two[3 * U + 1:4 * U + 1].tolist() == [0] * U and np.array_equal(two[:3 * U + 1], tab[:3 * U + 1])
    assert np.array_equal(M.ratio_tables([(off_a, lengths), (off_b, lengths), None], [90000, 90000]), two)
    assert M.SI_CHUNK == 4096


def test_an_utterances_items_do_not_depend_on_the_batch():
    alone = M.ratio_tables([([0], [12289]), ([0], [12289])], [12289, 12289])
    many = M.ratio_tables([([0, 100, 20000], [7, 12289, 5000])] * 2, [30000, 30000])
    assert alone[1] - alone[0] == many[2] - many[1] == 4


def test_trim_moves_the_offsets():
    lengths, off = [2000, 1601], [0, 2048]
    tab = M.ratio_tables([(off, lengths), (off, lengths), (off, lengths)], [4096] * 3, trim=800)
    U = 2
    assert tab[:U + 1].tolist() == [0, 1, 2]
    for k in range(3):
        assert tab[(k + 1) * U + 1:(k + 2) * U + 1].tolist() == [800, 2848]
    assert tab[4 * U + 1:].tolist() == [400, 1]


def test_every_refusal():
    ok = ([0, 100], [100, 50])
    with pytest.raises(ValueError, match="utterance 1: s_hat has 50 samples, s 51"):
        M.ratio_tables([ok, ([0, 100], [100, 51])], [200, 200])
    with pytest.raises(ValueError, match="utterance 0: s_hat has 100 samples, n 99"):
        M.ratio_tables([ok, ok, ([0, 100], [99, 50])], [200, 200, 200])
    with pytest.raises(ValueError, match="utterance 1 has 50 samples: not longer than 2 \\* trim = 50"):
        M.ratio_tables([ok, ok], [200, 200], trim=25)
    M.ratio_tables([ok, ok], [200, 200], trim=24)
    with pytest.raises(ValueError, match="utterance 1 has 0 samples"):
        M.ratio_tables([([0, 100], [100, 0])] * 2, [200, 200])
    with pytest.raises(ValueError, match="utterance 1 of s .* leaves its buffer \\(149 elements\\)"):
        M.ratio_tables([ok, ok], [200, 149])
    with pytest.raises(ValueError, match="utterance 0 of n .* leaves its buffer"):
        M.ratio_tables([ok, ok, ([-1, 100], [100, 50])], [200, 200, 200])
    with pytest.raises(ValueError, match="n holds 1 utterances, s_hat 2"):
        M.ratio_tables([ok, ok, ([0], [100])], [200, 200, 200])
    with pytest.raises(ValueError, match="no utterances"):
        M.ratio_tables([([], []), ([], [])], [0, 0])
    with pytest.raises(ValueError, match="trim must not be negative"):
        M.ratio_tables([ok, ok], [200, 200], trim=-1)
    with pytest.raises(ValueError, match="views of s_hat and s"):
        M.ratio_tables([ok], [200])


def test_batch_functions_refuse_before_touching_the_device():
    """Unequal lengths and too-short utterances are refused from the lengths alone: the same ValueError with or without a GPU."""
    a = [np.zeros(2000), np.zeros(1600)]
    with pytest.raises(ValueError, match="utterance 1 has 1600 samples: not longer than 2 \\* trim = 1600"):
        M.energy_ratios_batch(a, a, a, trim=800)
    with pytest.raises(ValueError, match="utterance 0: s_hat has 2000 samples, s 1999"):
        M.si_sdr_batch(a, [np.zeros(1999), np.zeros(1600)])
    with pytest.raises(ValueError, match="not a 1-D array"):
        M.si_sdr_batch([np.zeros((2, 3))], [np.zeros(6)])
    with pytest.raises(ValueError, match="the noise is required"):
        M.energy_ratios_batch(a, a, None)


def test_binding_types_the_scorer():
    native = importlib.import_module("disentangled-vae_amd.native")
    lib = native.load()
    assert native.ABI_VERSION == 1
    assert lib.dvae_si_ratios_workspace_bytes(10) == 10 * 6 * 8
    assert lib.dvae_si_ratios_batch(None, 0, 0, None, 0, 0, None, 0, 0, 1, None, 1, None, None, None, None) != 0
    assert b"si_ratios_batch" in lib.dvae_last_error()


def test_mcem_batch_has_a_score_method():
    assert callable(importlib.import_module("disentangled-vae_amd.mcem").McemBatch.score)
