"""Host side of the device mixer (no GPU): the numpy restatement tests/mix_ref.py against the recorded outputs of the reference's own
process_save_utt bit for bit, the table of dvae_mix_snr_batch and every refusal of mix_tables, the condition grid, the segment draw."""
import importlib
import os

import numpy as np
import pytest

import mix_bounds as XB
import mix_ref as XR

X = importlib.import_module("disentangled-vae_amd.mix")
H = importlib.import_module("disentangled-vae_amd.stft")
R = importlib.import_module("disentangled-vae_amd.ragged")
native = importlib.import_module("disentangled-vae_amd.native")
GOLD = XR.load_golden(os.path.join(os.path.dirname(__file__), "golden", "mix_golden.npz"))


def test_fixture_holds_the_cases_the_bounds_are_checked_on():
    assert sorted(len(c["speech"]) for c in GOLD.values()) == [63, 4096, 4097, 12289, 16000, 48000]
    snrs = sorted(c["snr_db"] for c in GOLD.values())
    assert snrs[-1] == 40.0 and all(-15.0 <= s <= 5.0 for s in snrs[:-1])
    assert any(c["speech"][np.argmax(np.abs(c["speech"]))] < 0 for c in GOLD.values())                # a negative speech peak
    assert any(c["bank"].dtype == np.float64 for c in GOLD.values()) and all(c["speech"].dtype == np.float32 for c in GOLD.values())
    assert all(len(c["bank"]) <= 3 * len(c["speech"]) for c in GOLD.values())


@pytest.mark.parametrize("name", sorted(GOLD))
def test_numpy_restatement_equals_the_reference_bit_for_bit(name):
    c = GOLD[name]
    np.random.seed(c["seed"])
    assert np.random.randint(len(c["bank"]) - len(c["speech"])) == c["start"]                       # the reference's own draw
    got = XR.mix_one(c["speech"], c["bank"], c["start"], c["snr_db"])
    for k, key in (("s", "speech"), ("n", "noise"), ("x", "mixture")):
        assert got[key].dtype == np.float64
        for part, want in c["out"][k].items():
            assert np.array_equal(XR.recorded_parts(got[key], c)[part], want), (name, k, part)
    assert max(np.max(np.abs(got[key])) for key in ("speech", "noise", "mixture")) == 1.0
    assert abs(got["snr_db"] - c["snr_db"]) < 1e-9
    assert got["k"] == (got["Ps"] * XR.snr_factor(c["snr_db"])) / got["Pn"]


def test_snr_factors_are_the_reference_scalars():
    snrs = [-15.0, -10.0, -5.0, 0.0, 5.0, 40.0, 3]
    f = X.snr_factors(snrs)
    assert f.dtype == np.float64 and [float(v) for v in f] == [float(np.power(10, -s / 10)) for s in snrs]


# ---- the table -------------------------------------------------------------------------------------------------------------------------

def test_table_default_layout_with_repeated_speech():
    s_off, s_len = [0, 0, 5000, 0], [5000, 5000, 4096, 5000]                                        # utterance 0 three times
    b_off, b_len = [0, 20000], [20000, 9000]
    tab = X.mix_tables((s_off, s_len), (b_off, b_len, [0, 1, 1, 0]), [7, 0, 4904, 15000], None, (9096, 29000))
    U = 4
    assert tab.dtype == np.int64 and tab.size == 6 * U + 1
    assert tab[:U + 1].tolist() == [0, 2, 4, 5, 7]                                                   # ceil(len / 4096) items each
    assert tab[U + 1:2 * U + 1].tolist() == s_off
    assert tab[2 * U + 1:3 * U + 1].tolist() == [7, 20000, 24904, 15000]                             # bank offset + start
    assert tab[3 * U + 1:4 * U + 1].tolist() == [0, 5056, 10112, 14208]                              # packed at multiples of 64
    assert tab[4 * U + 1:5 * U + 1].tolist() == s_len and tab[5 * U + 1:].tolist() == s_len


def test_table_explicit_layout_and_head_lengths():
    plan = H.plan_stft_batch([16000, 32000, 1024])
    assert plan["end_pad"].tolist() == [1, 0, 0]
    tab = X.mix_tables(([0, 16000, 48000], [16000, 32000, 1024]), ([0], [60000], [0, 0, 0]), [0, 100, 5], None,
                       (49024, 60000, int(plan["padded"].sum())), (plan["x0"], plan["padded"]))
    U = 3
    assert tab[3 * U + 1:4 * U + 1].tolist() == [0, 16256, 48256] and tab[5 * U + 1:].tolist() == [16256, 32000, 1024]
    head = X.mix_tables(([0], [16000]), ([0], [60000], [0]), [50000], [9000], (16000, 60000))      # the first 9000 samples only
    assert head[1] == 3 and head[4 * 1 + 1] == 9000 and head[2 * 1 + 1] == 50000


GOOD = dict(speech_view=([0, 100], [100, 200]), noise_view=([0, 1000], [1000, 500], [0, 1]), starts=[900, 300], lengths=None, totals=(300, 1500))


def table(**kw):
    return X.mix_tables(**{**GOOD, **kw})


def test_every_refusal_names_the_utterance():
    assert table().size == 13
    with pytest.raises(ValueError, match=r"utterance 1: the noise segment \[301, 501\) leaves its bank \(500 samples\)"):
        table(starts=[900, 301])
    with pytest.raises(ValueError, match="utterance 0: the noise segment"):
        table(starts=[-1, 0])
    with pytest.raises(ValueError, match=r"utterance 1 of speech \(\[100, 300\)\) leaves its buffer \(299 elements\)"):
        table(totals=(299, 1500))
    with pytest.raises(ValueError, match="utterance 0 of speech"):
        table(speech_view=([-1, 100], [100, 200]))
    with pytest.raises(ValueError, match="starts has 3 entries for 2 utterances"):
        table(starts=[0, 0, 0])
    with pytest.raises(ValueError, match="noise_index has 1 entries for 2 utterances"):
        table(noise_view=([0, 1000], [1000, 500], [0]))
    with pytest.raises(ValueError, match="utterance 1 names noise bank 2 of 2"):
        table(noise_view=([0, 1000], [1000, 500], [0, 2]))
    with pytest.raises(ValueError, match="utterance 1: noise bank 1 leaves the noise buffer"):
        table(totals=(300, 1499))
    with pytest.raises(ValueError, match="utterance 0 mixes 0 samples"):
        table(lengths=[0, 200])
    with pytest.raises(ValueError, match="utterance 1 mixes 201 samples of 200"):
        table(lengths=[100, 201])
    with pytest.raises(ValueError, match="no utterances"):
        table(speech_view=([], []), noise_view=([0], [10], []), starts=[])
    # output layouts
    ok = table(totals=(300, 1500, 400), out_layout=([200, 0], [150, 200]))
    assert ok[7:9].tolist() == [200, 0] and ok[11:].tolist() == [150, 200]
    with pytest.raises(ValueError, match="utterance 1: out_extent 199 is shorter than its 200 samples"):
        table(totals=(300, 1500, 400), out_layout=([0, 100], [100, 199]))
    with pytest.raises(ValueError, match="output ranges of utterances 0 and 1 overlap"):
        table(totals=(300, 1500, 400), out_layout=([0, 99], [100, 200]))
    with pytest.raises(ValueError, match="output ranges of utterances 1 and 0 overlap"):
        table(totals=(300, 1500, 400), out_layout=([100, 0], [100, 201]))
    with pytest.raises(ValueError, match=r"utterance 1 of the outputs \(\[100, 300\)\) leaves its buffer \(299 elements\)"):
        table(totals=(300, 1500, 299), out_layout=([0, 100], [100, 200]))
    with pytest.raises(ValueError, match="element count of each buffer"):
        table(out_layout=([0, 100], [100, 200]))                                                     # no extent of the outputs given


def test_the_batch_call_refuses_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(native, "LIB_PATH", "/nonexistent/libdvae_hip.so")
    monkeypatch.setattr(native, "_lib", None)
    speech = [np.zeros(100, np.float32), np.zeros(200, np.float32)]
    banks = [np.zeros(1000, np.float32), np.zeros(500)]
    with pytest.raises(ValueError, match="utterance 1: the noise segment"):
        X.mix_at_snr_batch(speech, banks, [0, 1], [0, 301], [0.0, 5.0])
    with pytest.raises(ValueError, match="snr_db has 1 entries for 2 utterances"):
        X.mix_at_snr_batch(speech, banks, [0, 1], [0, 300], [0.0])
    with pytest.raises(ValueError, match="starts has 1 entries"):
        X.mix_at_snr_batch(speech, banks, [0, 1], [0], [0.0, 5.0])
    with pytest.raises(ValueError, match="noise_index has 3 entries"):
        X.mix_at_snr_batch(speech, banks, [0, 1, 1], [0, 0], [0.0, 5.0])
    with pytest.raises(ValueError, match="too small to analyze"):                                 # the STFT layout needs a frame
        X.mix_at_snr_batch(speech, banks, [0, 1], [0, 0], [0.0, 5.0], stft_layout=True)
    with pytest.raises(ValueError, match="entry 1 is not a 1-D"):
        X.mix_at_snr_batch([speech[0], np.zeros((2, 50))], banks, [0, 1], [0, 0], [0.0, 5.0])
    with pytest.raises(TypeError, match="not floating point"):
        X.mix_at_snr_batch([speech[0], np.zeros(50, np.int16)], banks, [0, 1], [0, 0], [0.0, 5.0])
    with pytest.raises(RuntimeError):                                                               # a good call reaches the device path
        X.mix_at_snr_batch(speech, banks, [0, 1], [0, 300], [0.0, 5.0])


def test_a_repeated_array_is_packed_once():
    a, b = np.zeros(100, np.float32), np.zeros(50, np.float32)
    offs, lens, total = R.view([a, b, a, a], dedupe=True)
    assert offs.tolist() == [0, 100, 0, 0] and lens.tolist() == [100, 50, 100, 100] and total == 150


# ---- the grid and the draw -------------------------------------------------------------------------------------------------------------

def test_condition_grid_expands_utterances_noises_snrs():
    si, ni, snr = X.condition_grid(2, ["cafe", "home", "car"], [-5, 0.0])
    assert si == [0] * 6 + [1] * 6 and ni == [0, 0, 1, 1, 2, 2] * 2 and snr == [-5.0, 0.0] * 6
    si, ni, snr = X.condition_grid(5, 3, [-5.0, 0.0, 5.0, 10.0])
    assert len(si) == len(ni) == len(snr) == 60 and sorted(set(zip(si, ni, snr))) == sorted(zip(si, ni, snr))
    with pytest.raises(ValueError):
        X.condition_grid(0, 3, [0.0])
    with pytest.raises(ValueError):
        X.condition_grid(2, 3, [])


def test_drawn_starts_stay_inside_their_banks():
    rng = np.random.default_rng(0)
    banks, index = [1001, 50000, 16001], [int(i) for i in rng.integers(0, 3, 500)]
    lengths = [int(rng.integers(1, [1001, 50000, 16001][b])) for b in index]
    starts = X.draw_noise_starts(np.random.default_rng(1), banks, index, lengths)
    assert len(starts) == 500 and all(0 <= s and s + n <= banks[b] for s, n, b in zip(starts, lengths, index))
    assert starts == X.draw_noise_starts(np.random.default_rng(1), banks, index, lengths)          # a Generator repeats
    tight = X.draw_noise_starts(np.random.default_rng(2), [101], [0] * 50, [100] * 50)
    assert set(tight) == {0}                                                                          # integers(1): the one start there is
    X.mix_tables((np.zeros(500, np.int64), lengths), ([0, 1001, 51001], banks, index), starts, None, (50000, 67002))
    with pytest.raises(ValueError, match="utterance 1: noise bank 0 .* is not longer"):
        X.draw_noise_starts(rng, [100], [0, 0], [50, 100])
    with pytest.raises(TypeError):
        X.draw_noise_starts(np.random, [100], [0], [50])
    assert "not reproducible" in X.draw_noise_starts.__doc__


# ---- the bound -------------------------------------------------------------------------------------------------------------------------

def test_bound_as_a_function_of_the_length():
    u = 2.0 ** -53
    assert XB.e_power(63) == (70 + 1 + 62) * u and XB.e_power(48000) == (70 + 12 + 47999) * u
    b = XB.bounds(48000)
    assert b["speech"] < b["noise"] < b["mix"] and 1.0e-11 < b["noise"] < 1.1e-11
    assert XB.bounds(63)["mix"] < 4e-14
    ref = XR.mix_one(GOLD["n63"]["speech"], GOLD["n63"]["bank"], GOLD["n63"]["start"], -15.0)
    w = XB.worst(ref, ref)
    assert set(w) == {"speech", "noise", "mix", "k", "norm"} and all(v == 0.0 for v in w.values())
