"""The batched mixer on the MI355X (dvae_mix_snr_batch; mix.mix_at_snr_batch): the reference's recorded outputs within a derived bound,
bit-identity across batches and runs and over a condition grid, the float32 forms, the STFT layout, IEEE degenerate cases, a bad
table entry, and the enhancement example's path.

The bound is derived, not tuned: tests/mix_bounds.py states it as a function of the length (u = 2^-53).  Device and reference differ
only in the order of the two power sums; with e_P = (70 + ceil(n / 4096) + n - 1) u that gives e_P + 12 u on out_speech and
2 e_P + 18 u on out_noise per element, 2 e_P + 20 u on out_mix relative to |out_speech| + |out_noise|, 2 e_P + 4 u on k and
e_P + 10 u on norm: 1.07e-11 on out_noise at 48 000 samples, nearly all of it the worst case of the reference's own sum.
Every test prints its figures in units of the bound before it asserts.  Not yet measured on an MI355X.
"""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mix_bounds as XB
import mix_ref as XR

pytestmark = pytest.mark.gpu
X = importlib.import_module("disentangled-vae_amd.mix")
H = importlib.import_module("disentangled-vae_amd.stft")
N = importlib.import_module("disentangled-vae_amd.native")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = XR.load_golden(os.path.join(os.path.dirname(__file__), "golden", "mix_golden.npz"))
KEYS = ("speech", "noise", "mixture")


def speechlike(n, seed):
    rng = np.random.default_rng(seed)
    env = np.repeat((rng.random(n // 800 + 1) > 0.4).astype(np.float64), 800)[:n] + 0.05
    return env * rng.standard_normal(n) * 0.1


def bank(n, seed):
    w = np.random.default_rng(seed).standard_normal(n + 1)
    return 0.05 * (w[1:] + 0.7 * w[:-1])


def host(mb):
    """A MixBatch as a list of per-utterance dicts of host arrays and stats scalars."""
    parts = [b.numpy() for b in (mb.speech, mb.noise, mb.mixture)]
    stats = mb.stats.cpu().numpy()
    return [dict(speech=parts[0][u], noise=parts[1][u], mixture=parts[2][u], **dict(zip(X.STATS, stats[u]))) for u in range(len(mb))]


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS) and \
        np.array_equal([a[k] for k in X.STATS], [b[k] for k in X.STATS], equal_nan=True)


# ---- the reference's recorded outputs --------------------------------------------------------------------------------------------------

def test_fixture_cases_in_one_batch_within_the_derived_bound():
    names = sorted(GOLD)
    cases = [GOLD[n] for n in names]
    mb = X.mix_at_snr_batch([c["speech"] for c in cases], [c["bank"] for c in cases], list(range(len(cases))), [c["start"] for c in cases],
                            [c["snr_db"] for c in cases])
    assert mb.stats.shape == (len(cases), 6) and mb.stats.dtype == torch.float64 and mb.stats.is_cuda
    assert all(b.y.is_cuda and b.y.dtype == torch.float64 for b in (mb.speech, mb.noise, mb.mixture))
    worst = {}
    for name, c, got in zip(names, cases, host(mb)):
        ref = XR.mix_one(c["speech"], c["bank"], c["start"], c["snr_db"])
        for k, key in zip("snx", KEYS):                                   # the restatement IS the recorded reference, bit for bit
            for part, want in c["out"][k].items():
                assert np.array_equal(XR.recorded_parts(ref[key], c)[part], want), (name, key, part)
        w = XB.worst(got, ref)
        print(name, "errors in units of their bounds", w, "bounds", XB.bounds(len(c["speech"])), "achieved SNR - request",
              got["snr_db"] - c["snr_db"])
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (name, k, v)
        assert got["p"] == ref["p"]                                       # a maximum: exact
        assert abs(got["snr_db"] - c["snr_db"]) <= 1e-9, name
        assert max(np.max(np.abs(got[key])) for key in KEYS) == 1.0       # the common peak divides itself
    print("worst over the fixture, in units of the bound:", worst)


def test_without_speech_normalisation_and_from_device_buffers():
    s = [speechlike(9000, 1) * 3.0, speechlike(5000, 2)]
    banks = [bank(20000, 3), bank(12000, 4)]
    packed = torch.from_numpy(np.concatenate(s)).cuda()
    wb = H.WaveBatch(packed, [0, 9000, 0], [9000, 5000, 9000])             # ranges may repeat
    nb = torch.from_numpy(banks[0]).cuda()
    mb = X.mix_at_snr_batch(wb, [nb], [0, 0, 0], [100, 7000, 11000], [0.0, -5.0, 5.0], normalise_speech=False)
    for u, (got, su, start, snr) in enumerate(zip(host(mb), (s[0], s[1], s[0]), (100, 7000, 11000), (0.0, -5.0, 5.0))):
        ref = XR.mix_one(su, banks[0], start, snr, normalise_speech=False)
        assert all(v <= 1.0 for v in XB.worst(got, ref).values()), u
        assert got["p"] == 1.0 and abs(got["snr_db"] - snr) <= 1e-9


# ---- bit-identity ----------------------------------------------------------------------------------------------------------------------

def test_alone_and_inside_37_ragged_utterances_and_twice():
    rng = np.random.default_rng(11)
    lengths = [int(x) for x in rng.integers(64, 30000, 37)]
    lengths[5], lengths[20] = 4096, 80000
    speech = [speechlike(L, 100 + i).astype(np.float32 if i % 2 else np.float64) for i, L in enumerate(lengths)]
    banks = [bank(100000, 7), bank(90000, 8).astype(np.float32), bank(81000, 9)]
    index = [i % 3 for i in range(37)]
    starts = X.draw_noise_starts(np.random.default_rng(1), [len(b) for b in banks], index, lengths)
    snrs = [float(rng.choice([-15.0, -10.0, -5.0, 0.0, 5.0])) for _ in range(37)]
    a = host(X.mix_at_snr_batch(speech, banks, index, starts, snrs))
    b = host(X.mix_at_snr_batch(speech, banks, index, starts, snrs))
    assert all(same_bits(x, y) for x, y in zip(a, b))
    for u in (0, 5, 20, 36):
        alone = host(X.mix_at_snr_batch([speech[u]], banks, [index[u]], [starts[u]], [snrs[u]]))[0]
        assert same_bits(alone, a[u]), u
    ref = XR.mix_one(speech[20], banks[index[20]], starts[20], snrs[20])
    assert all(v <= 1.0 for v in XB.worst(a[20], ref).values())


def test_condition_grid_equals_its_sixty_single_calls():
    speech = [speechlike(L, 200 + i) for i, L in enumerate([5000, 8192, 4097, 12000, 6001])]
    banks = [bank(30000, 20), bank(25000, 21), bank(20000, 22)]
    si, ni, snr = X.condition_grid(5, 3, [-10.0, -5.0, 0.0, 5.0])
    grid = [speech[u] for u in si]                                         # the same arrays again and again: the same speech ranges
    starts = X.draw_noise_starts(np.random.default_rng(3), [len(b) for b in banks], ni, [len(g) for g in grid])
    mb = X.mix_at_snr_batch(grid, banks, ni, starts, snr)
    assert len(mb) == 60
    got = host(mb)
    for c in range(60):
        alone = host(X.mix_at_snr_batch([grid[c]], banks, [ni[c]], [starts[c]], [snr[c]]))[0]
        assert same_bits(alone, got[c]), c
    assert all(abs(g["snr_db"] - want) <= 1e-9 for g, want in zip(got, snr))


def test_float32_inputs_and_float32_outputs():
    lengths = [63, 4097, 16000]
    s32 = [speechlike(L, 300 + i).astype(np.float32) for i, L in enumerate(lengths)]
    b32 = [bank(40000, 30).astype(np.float32)]
    args = ([0, 0, 0], [5, 20000, 23999], [-5.0, 0.0, 40.0])
    a = X.mix_at_snr_batch(s32, b32, *args)
    b = X.mix_at_snr_batch([x.astype(np.float64) for x in s32], [b32[0].astype(np.float64)], *args)
    assert all(same_bits(x, y) for x, y in zip(host(a), host(b)))          # float32 samples are read as their exact float64 images
    c = X.mix_at_snr_batch(s32, b32, *args, out_dtype=torch.float32)
    assert c.mixture.y.dtype == torch.float32 and torch.equal(c.stats, a.stats)
    for x, y in zip(host(c), host(a)):
        assert all(np.array_equal(x[k], y[k].astype(np.float32)) for k in KEYS)   # one more rounding of the double result


# ---- the STFT layout -------------------------------------------------------------------------------------------------------------------

def test_stft_layout_feeds_the_batch_transform_in_place():
    lengths = [16000, 32000, 11008, 20000]                                 # end pad: yes, no, yes, ...
    speech = [speechlike(L, 400 + i) for i, L in enumerate(lengths)]
    banks = [bank(50000, 40)]
    mb = X.mix_at_snr_batch(speech, banks, [0] * 4, [0, 1000, 30000, 29999], [0.0, -5.0, 5.0, -15.0], stft_layout=True)
    plan = H.plan_stft_batch(lengths)
    assert plan["end_pad"].sum() >= 2 and mb.mixture.offsets == plan["x0"].tolist()
    spec = mb.spec()
    want = H.stft_batch(mb.mixture.numpy())                                # the host copies, padded and packed by the host
    assert spec.counts == want.counts and torch.equal(torch.view_as_real(spec.frames), torch.view_as_real(want.frames))
    power = mb.spec(layout=1)
    assert torch.equal(power.frames, H.stft_batch(mb.mixture.numpy(), layout=1).frames)
    plain = X.mix_at_snr_batch(speech, banks, [0] * 4, [0, 1000, 30000, 29999], [0.0, -5.0, 5.0, -15.0])
    assert all(same_bits(x, y) for x, y in zip(host(mb), host(plain)))     # the layout moves the outputs, nothing else
    with pytest.raises(RuntimeError, match="stft_layout=True"):
        plain.spec()


def prefilled_call(speech, noise, tab, factors, n_out, dtype=torch.float64, fill=7.0):
    outs = [torch.full((n_out,), fill, dtype=dtype, device="cuda") for _ in range(3)]
    return X.mix_packed(speech, noise, tab, factors, True, dtype, n_out, outs)


def test_pad_is_written_as_zeros_and_the_gaps_are_untouched():
    lengths = [5000, 63, 8192]
    speech = [speechlike(L, 500 + i) for i, L in enumerate(lengths)]
    nb = bank(20000, 50)
    s_off = [0, 5000, 5063]
    out0, extent = [17, 6000, 6400], [5256, 63, 8192 + 4096 + 300]         # a pad of a hop, none, one longer than a work item
    n_out = 6400 + extent[2] + 29
    tab = X.mix_tables((s_off, lengths), ([0], [20000], [0, 0, 0]), [0, 100, 11000], None, (13255, 20000, n_out), (out0, extent))
    sp, nz = torch.from_numpy(np.concatenate(speech)).cuda(), torch.from_numpy(nb).cuda()
    for dtype in (torch.float64, torch.float32):
        outs = prefilled_call(sp, nz, tab, X.snr_factors([0.0, 5.0, -5.0]), n_out, dtype)
        written = np.zeros(n_out, bool)
        for u, L in enumerate(lengths):
            ref = XR.mix_one(speech[u], nb, [0, 100, 11000][u], [0.0, 5.0, -5.0][u])
            written[out0[u]:out0[u] + extent[u]] = True
            for o, key in zip(outs[:3], KEYS):
                h = o.cpu().numpy()
                assert np.all(h[out0[u] + L:out0[u] + extent[u]] == 0.0), (u, key)          # exact zeros
                got = h[out0[u]:out0[u] + L].astype(np.float64)
                tol = XB.bounds(L)["mix"] + (2.0 ** -24 if dtype == torch.float32 else 0.0)
                assert np.all(np.abs(got - ref[key]) <= tol * (np.abs(ref["speech"]) + np.abs(ref["noise"]))), (u, key)
        for o in outs[:3]:
            assert bool((o.cpu().numpy()[~written] == 7.0).all())           # between and around the utterances: as they were


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------------

def test_zero_nan_and_inf_inputs_follow_numpy_and_spare_the_others():
    n = 6000
    good = [speechlike(n, 600), speechlike(4097, 601)]
    with_nan, with_inf = speechlike(n, 602), speechlike(n, 603)
    with_nan[4500], with_inf[100] = np.nan, np.inf
    speech = [good[0], speechlike(n, 604), np.zeros(n), with_nan, with_inf, good[1], speechlike(n, 605)]
    b0 = bank(30000, 60)
    b0[10000:10000 + n] = 0.0                                               # an all-zero noise segment
    b1 = bank(30000, 61)
    b1[123] = np.nan                                                        # a NaN in the noise (utterance 6 reads it)
    index, starts, snrs = [0, 0, 0, 0, 0, 1, 1], [0, 10000, 500, 700, 900, 20000, 0], [0.0, 0.0, -5.0, 5.0, -10.0, -15.0, 0.0]
    got = host(X.mix_at_snr_batch(speech, [b0, b1], index, starts, snrs))
    for u in range(7):
        ref = XR.mix_one(speech[u], (b0, b1)[index[u]], starts[u], snrs[u])
        for key in KEYS:
            assert np.array_equal(np.isnan(got[u][key]), np.isnan(ref[key])), (u, key)
            assert np.array_equal(np.isinf(got[u][key]), np.isinf(ref[key])), (u, key)
        for k in ("p", "Ps", "Pn", "k", "norm"):
            assert np.isnan(got[u][k]) == np.isnan(ref[k]) and np.isinf(got[u][k]) == np.isinf(ref[k]), (u, k)
        if u in (0, 5):
            assert all(v <= 1.0 for v in XB.worst(got[u], ref).values())
            alone = host(X.mix_at_snr_batch([speech[u]], [b0, b1], [index[u]], [starts[u]], [snrs[u]]))[0]
            assert same_bits(alone, got[u]), u                              # the others of the batch are as if alone
        else:
            assert all(np.isnan(got[u][key]).all() for key in KEYS), u      # what numpy gives the reference: NaN throughout
    assert got[1]["Pn"] == 0.0 and np.isposinf(got[1]["k"]) and got[2]["p"] == 0.0 and np.isposinf(got[4]["p"])


# ---- a bad table entry, through the C ABI ----------------------------------------------------------------------------------------------

def test_a_bad_table_entry_leaves_nan_stats_and_writes_nothing_else():
    """The kernels recheck the table: an utterance whose entry leaves a buffer (the host check bypassed) is dropped."""
    lib = N.load()
    lengths = [5000, 300, 9000]
    speech = [speechlike(L, 700 + i) for i, L in enumerate(lengths)]
    nb = bank(20000, 70)
    sp, nz = torch.from_numpy(np.concatenate(speech)).cuda(), torch.from_numpy(nb).cuda()
    U, n_out = 3, 5056 + 320 + 9000
    tab = X.mix_tables(([0, 5000, 5300], lengths), ([0], [20000], [0, 0, 0]), [0, 6000, 11000], None, (14300, 20000))
    fac = X.snr_factors([0.0, 5.0, -5.0])
    good = prefilled_call(sp, nz, tab, fac, n_out)

    def call(table):
        outs = [torch.full((n_out,), 7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        stats = torch.zeros((U + 2, 6), dtype=torch.float64, device="cuda")
        ws = torch.empty(lib.dvae_mix_snr_workspace_bytes(int(table[U]), U), dtype=torch.uint8, device="cuda")
        t, f = torch.from_numpy(table).cuda(), torch.from_numpy(fac).cuda()
        N.check(lib.dvae_mix_snr_batch(N.ptr(sp), sp.numel(), 1, N.ptr(nz), nz.numel(), 1, U, N.ptr(t), int(table[U]), N.ptr(f), 1, N.ptr(outs[0]),
                                       N.ptr(outs[1]), N.ptr(outs[2]), n_out, 1, N.ptr(stats[1:]), N.ptr(ws), N.stream()), "dvae_mix_snr_batch")
        torch.cuda.synchronize()
        assert bool((stats[0] == 0).all()) and bool((stats[-1] == 0).all())           # the rows around the stats: untouched
        return outs, stats[1:-1]

    entries = {"noise0": (2 * U + 1 + 1, 20000 - 100),                      # utterance 1: 300 samples from 100 before the bank's end
               "speech0": (U + 1 + 1, -1),
               "len": (4 * U + 1 + 1, 300 + 4096),                          # a length that disagrees with the item count
               "out0": (3 * U + 1 + 1, n_out - 299),
               "out_extent": (5 * U + 1 + 1, 299)}                          # shorter than the length
    for name, (pos, value) in entries.items():
        bad = tab.copy()
        bad[pos] = value
        outs, stats = call(bad)
        assert torch.isnan(stats[1]).all(), name
        assert torch.equal(stats[[0, 2]], good[3][[0, 2]]), name
        for o, g in zip(outs, good[:3]):
            assert bool((o[5056:5056 + 320] == 7.0).all()), name            # utterance 1's outputs: unwritten
            assert torch.equal(o[:5000], g[:5000]) and torch.equal(o[5376:], g[5376:]), name
            assert bool((o == 7.0).sum() == (g == 7.0).sum() + 300), name
    rc = lib.dvae_mix_snr_batch(N.ptr(sp), sp.numel(), 1, N.ptr(nz), nz.numel(), 1, U, None, 7, None, 1, None, None, None, n_out, 1, None, None, None)
    assert rc != 0 and b"mix_snr_batch" in lib.dvae_last_error()


# ---- the enhancement example ------------------------------------------------------------------------------------------------------------

def test_enhance_mcem_example_scores_sir_and_sar_with_the_mixers_noise(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "enhance_mcem.py"), "--synthetic", "3", "--snr", "0", "--niter", "2",
                        "--score", "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr, sep="\n")
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    table = next(i for i, line in enumerate(lines) if "SI-SIR" in line)                 # the table of the mixer's conditions
    rows = [line.split() for line in lines[table + 1:] if line.startswith("synthetic_")]
    assert len(rows) == 3
    for row in rows:
        snr, sdr, sir, sar = (float(v) for v in row[1:5])
        assert abs(snr) < 1e-6 and all(np.isfinite(v) for v in (sdr, sir, sar)), row
    assert len(list(tmp_path.glob("*_s_est.wav"))) == 3
