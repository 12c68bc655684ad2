"""The batched scorer on the MI355X (dvae_si_ratios_batch; metrics.energy_ratios_batch / si_sdr_batch, the packages.metrics drop-ins
on CUDA tensors, McemBatch.score): the reference's recorded values, the sums against long double at every loop bound, bit-identity
across batches and runs, IEEE degenerate cases, packed buffers past 2^31 bytes.

Bounds are derived, not tuned: tests/metrics_bounds.py states them (u = 2^-53).  In short
  * a device sum of terms t_i over k work items: |err| <= (64 + 6 + k) u sum |t_i| (64 fma per lane, 6 butterfly levels, k partials);
  * a ratio in dB: (10 / ln 10) (eps_num + eps_den) + 2 ulp, where alpha enters through kappa = sum |sh_i s_i| / |sum sh_i s_i| (and
    likewise for n), computed from each test's inputs, and the per-sample rounding of a residual through |s_target| / |residual|;
  * against recorded reference values, the reference's own worst case (n u per sum, any order) is added.
Every fixture and random case keeps kappa <= 1e3 (asserted).  On the fixture the bound device + reference is 2.5e-13 dB (n = 2) ...
3.1e-9 dB (n = 16 000, kappa_n = 14, SI-SAR +38 dB); the device alone is held to 2.2e-13 ... 2.1e-11 dB of the long-double value.
Measured on an MI355X: every figure of this module within 4 % of its bound (the worst: |n|^2 at 4095 samples, 2.6e-16 relative).
"""
import importlib
import os

import numpy as np
import pytest
import torch

import metrics_bounds as MB
from packages import metrics as PM

pytestmark = pytest.mark.gpu
M = importlib.import_module("disentangled-vae_amd.metrics")
H = importlib.import_module("disentangled-vae_amd.stft")
FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics_golden.npz"))
NAMES = [str(n) for n in FIX["names"]]
COLS = {name: i for i, name in enumerate(M.SUMS)}


def fixture(name, dtype=np.float64):
    return tuple(FIX[f"{name}/{k}"].astype(dtype) for k in ("s_hat", "s", "n"))


def mixture(n, seed, snr_db=3.0, art_db=-12.0):
    """s_hat = 0.8 s + 0.3 n + artefact on speech-like s: kappa_s about 1, kappa_n a few units."""
    rng = np.random.default_rng(seed)
    env = np.repeat((rng.random(n // 800 + 1) > 0.4).astype(np.float64), 800)[:n] + 0.05
    s = env * rng.standard_normal(n) * 0.1
    noise = rng.standard_normal(n) * 0.05 * 10 ** (-snr_db / 20)
    art = rng.standard_normal(n) * 0.05 * 10 ** (art_db / 20)
    return 0.8 * s + 0.3 * noise + art, s, noise


def check_ratios(got, q, extra=None, what=""):
    """got: three dB values (or one without n) against the exact q within the device bound (+ extra by ratio name)."""
    MB.check_kappa(q)
    b = MB.bound_db(q)
    for i, (ratio, _) in enumerate(MB.RATIOS):
        if ratio not in q:
            continue
        tol = b[ratio] + (extra[ratio] if extra else 0.0)
        print(what, ratio, "got - expected", float(got[i]) - q[ratio], "bound", tol)
        assert abs(float(got[i]) - q[ratio]) <= tol, (what, ratio)


def check_sums(row, q, what=""):
    """One row of the [U, 8] sums against long double within the device's relative bounds."""
    MB.check_kappa(q)
    e = MB.relative(q, MB.gamma_dev(MB.items(q["len"])))
    for key, col in COLS.items():
        if key not in q:
            assert np.isnan(row[col]), (what, key)
            continue
        err, tol = abs(np.longdouble(row[col]) - q[key]), e[key] * abs(q[key])
        print(what, key, "relative error", float(err / abs(q[key])), "bound", e[key])
        assert err <= tol, (what, key)


# ---- the reference's recorded values -------------------------------------------------------------------------------------------------

def test_fixture_cases_in_one_batch():
    cases = [fixture(n) for n in NAMES]
    sh, s, n = ([c[k] for c in cases] for k in range(3))
    ratios = M.energy_ratios_batch(sh, s, n)
    leroux = M.si_sdr_batch(sh, s)
    assert ratios.shape == (len(NAMES), 3) and ratios.dtype == torch.float64 and ratios.is_cuda
    assert leroux.shape == (len(NAMES),) and leroux.dtype == torch.float64 and leroux.is_cuda
    ratios, leroux = ratios.cpu().numpy(), leroux.cpu().numpy()
    for u, name in enumerate(NAMES):
        q = MB.exact(*cases[u])
        check_ratios(ratios[u], q, what=name)                                             # the device against the exact value
        ref = MB.ref_db(q)
        rec = FIX[name + "/energy_ratios"]
        dev = MB.bound_db(q)
        for i, (ratio, _) in enumerate(MB.RATIOS):                                        # and against the recorded reference
            print(name, ratio, "got - recorded", ratios[u, i] - rec[i], "bound", dev[ratio] + ref[ratio])
            assert abs(ratios[u, i] - rec[i]) <= dev[ratio] + ref[ratio], (name, ratio)
        assert abs(leroux[u] - float(FIX[name + "/si_sdr_leroux"])) <= dev["si_sdr"] + ref["si_sdr"], name
        check_ratios([leroux[u]], MB.exact(cases[u][0], cases[u][1]), what=name + " (no n)")


@pytest.mark.parametrize("name", NAMES)
def test_dropin_functions_on_cuda_tensors(name):
    host = fixture(name)
    sh, s, n = (torch.from_numpy(a).cuda() for a in host)
    got = PM.energy_ratios(sh, s, n)
    assert len(got) == 3 and all(g.is_cuda and g.dim() == 0 and g.dtype == torch.float64 for g in got)
    q = MB.exact(*host)
    ref, dev = MB.ref_db(q), MB.bound_db(q)
    rec = FIX[name + "/energy_ratios"]
    for i, (ratio, _) in enumerate(MB.RATIOS):
        assert abs(float(got[i]) - rec[i]) <= dev[ratio] + ref[ratio], (name, ratio)
    leroux = PM.si_sdr_leroux(sh, s)
    assert leroux.is_cuda and abs(float(leroux) - float(FIX[name + "/si_sdr_leroux"])) <= dev["si_sdr"] + ref["si_sdr"]
    # float32 device tensors hold the fixture's values exactly: the same bits as from their float64 images
    sh32, s32, n32 = (torch.from_numpy(a).cuda() for a in fixture(name, np.float32))
    assert [float(g) for g in PM.energy_ratios(sh32, s32, n32)] == [float(g) for g in got]


def test_dropin_refuses_what_has_no_device_form():
    sh, s, n = (torch.from_numpy(a).cuda() for a in fixture("n63"))
    with pytest.raises(TypeError, match="host path only"):
        PM.si_sdr_components(sh, s, n)
    with pytest.raises(TypeError, match="mixed"):
        PM.energy_ratios(sh, s.cpu(), n)


# ---- the sums at every loop bound ------------------------------------------------------------------------------------------------------

LENGTHS = [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 1, 80000]


def packed_batch(lengths, dtypes, seed, gap=(1, 37)):
    """Utterances at unaligned offsets of three NaN-filled buffers (different offsets per buffer) -> host cases, WaveBatches."""
    rng = np.random.default_rng(seed)
    cases = []
    for i, L in enumerate(lengths):
        c = mixture(L, seed * 100 + i)
        cases.append(tuple(a.astype(dt).astype(np.float64) for a, dt in zip(c, dtypes)))      # what the device buffer will hold
    batches = []
    for k, dt in enumerate(dtypes):
        offs, pos = [], int(rng.integers(*gap))
        for L in lengths:
            offs.append(pos)
            pos += L + int(rng.integers(*gap))
        buf = np.full(pos, np.nan, dt)
        for c, o, L in zip(cases, offs, lengths):
            buf[o:o + L] = c[k]
        batches.append(H.WaveBatch(torch.from_numpy(buf).cuda(), offs, lengths))
    return cases, batches


@pytest.mark.parametrize("dtypes", [(np.float32, np.float64, np.float64), (np.float64, np.float32, np.float32),
                                    (np.float32, np.float32, np.float64), (np.float64, np.float64, np.float32)],
                         ids=["f32-f64-f64", "f64-f32-f32", "f32-f32-f64", "f64-f64-f32"])
def test_sums_against_long_double_at_every_loop_bound(dtypes):
    cases, (bh, bs, bn) = packed_batch(LENGTHS, dtypes, seed=3)
    ratios, sums = M.energy_ratios_batch(bh, bs, bn, return_sums=True)
    assert sums.shape == (len(LENGTHS), 8)
    ratios, sums = ratios.cpu().numpy(), sums.cpu().numpy()
    assert np.all(np.isfinite(sums[1:])) and np.all(np.isfinite(ratios[1:]))                 # no NaN sentinel leaked into a sum
    for u, L in enumerate(LENGTHS):
        if L == 1:
            # one sample: s_hat = alpha_s s up to a rounding, so the residuals are rounding noise (no relative bound exists); the
            # sums that do not cancel are exact products
            sh, s, n = (c[0] for c in cases[u])
            assert sums[u, COLS["dot_s"]] == sh * s and sums[u, COLS["ss"]] == s * s and sums[u, COLS["nn"]] == n * n
            assert abs(sums[u, COLS["e_noise_art"]]) <= (8 * MB.U * abs(sh)) ** 2
            continue
        q = MB.exact(*cases[u])
        check_sums(sums[u], q, what=f"len {L}")
        check_ratios(ratios[u], q, what=f"len {L}")
        # alpha is the IEEE quotient of the sums that are returned
        a_s = sums[u, COLS["dot_s"]] / sums[u, COLS["ss"]]
        assert sums[u, COLS["s_target"]] == a_s * a_s * sums[u, COLS["ss"]]


def test_without_noise_and_into_poisoned_outputs():
    cases, (bh, bs, _) = packed_batch(LENGTHS[1:], (np.float32, np.float64, np.float64), seed=5)
    sdr, sums = M.si_sdr_batch(bh, bs, return_sums=True)
    sdr, sums = sdr.cpu().numpy(), sums.cpu().numpy()
    for u, c in enumerate(cases):
        q = MB.exact(c[0], c[1])
        check_sums(sums[u], q, what=f"len {q['len']} (no n)")                              # the n columns must be NaN
        check_ratios([sdr[u]], q, what=f"len {q['len']} (no n)")
    # the C entry point on NaN-filled outputs with a guard row on either side: every row written, nothing outside
    tab = M.ratio_tables([(bh.offsets, bh.lengths), (bs.offsets, bs.lengths)], [bh.y.numel(), bs.y.numel()])
    U = len(cases)
    N = importlib.import_module("disentangled-vae_amd.native")
    lib = N.load()
    ratios = torch.full((U + 2, 3), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((U + 2, 8), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.dvae_si_ratios_workspace_bytes(int(tab[U])), dtype=torch.uint8, device="cuda")
    tab_dev = torch.from_numpy(tab).cuda()
    N.check(lib.dvae_si_ratios_batch(N.ptr(bh.y), bh.y.numel(), 0, N.ptr(bs.y), bs.y.numel(), 1, None, 0, 0, U, N.ptr(tab_dev), int(tab[U]),
                                     N.ptr(ratios[1:]), N.ptr(out[1:]), N.ptr(ws), N.stream()), "dvae_si_ratios_batch")
    assert torch.isnan(ratios[0]).all() and torch.isnan(ratios[-1]).all() and torch.isnan(out[0]).all() and torch.isnan(out[-1]).all()
    assert np.array_equal(ratios[1:-1, 0].cpu().numpy(), sdr) and torch.isnan(ratios[1:-1, 1:]).all()
    assert np.array_equal(out[1:-1].cpu().numpy(), sums, equal_nan=True)


def test_trim_scores_the_inner_samples():
    cases, (bh, bs, bn) = packed_batch([1601, 2000, 80000], (np.float32, np.float64, np.float64), seed=7)
    got = M.energy_ratios_batch(bh, bs, bn, trim=800).cpu().numpy()
    for u, c in enumerate(cases):
        if len(c[0]) - 1600 == 1:
            continue                                                                       # one sample: no relative bound (see above)
        check_ratios(got[u], MB.exact(*(a[800:-800] for a in c)), what=f"trimmed {len(c[0])}")
    lists = M.energy_ratios_batch(*([c[k][800:-800] for c in cases] for k in range(3))).cpu().numpy()
    assert np.array_equal(got, lists, equal_nan=True)                                      # offsets moved == arrays cut


def test_a_bad_table_entry_leaves_nan_and_spares_the_others():
    """The kernels recheck the table: an utterance whose entry leaves its buffer (the host check bypassed) is dropped."""
    cases, (bh, bs, bn) = packed_batch([5000, 300, 9000], (np.float32, np.float64, np.float64), seed=9)
    views = [(b.offsets, b.lengths) for b in (bh, bs, bn)]
    totals = [b.y.numel() for b in (bh, bs, bn)]
    tab = M.ratio_tables(views, totals)
    good, _ = M.si_ratios_packed([bh.y, bs.y, bn.y], tab)
    U = 3
    bad = tab.copy()
    bad[2 * U + 1 + 1] = totals[1] - 100                                                   # utterance 1 of s: 300 samples from 100 before the end
    ratios, sums = M.si_ratios_packed([bh.y, bs.y, bn.y], bad, True, True)
    assert torch.isnan(ratios[1]).all() and torch.isnan(sums[1]).all()
    assert torch.equal(ratios[[0, 2]], good[[0, 2]])
    bad = tab.copy()
    bad[4 * U + 1 + 2] = 9000 + 4096                                                       # a length that disagrees with the item count
    ratios, _ = M.si_ratios_packed([bh.y, bs.y, bn.y], bad)
    assert torch.isnan(ratios[2]).all() and torch.equal(ratios[:2], good[:2])


# ---- bit-identity ----------------------------------------------------------------------------------------------------------------------

def test_alone_and_inside_256_utterances_and_twice():
    rng = np.random.default_rng(11)
    lengths = [int(x) for x in rng.integers(100, 30000, 256)]
    lengths[100] = 80000
    cases = [tuple(a.astype(np.float32) if k == 0 else a for k, a in enumerate(mixture(L, 1000 + i))) for i, L in enumerate(lengths)]
    sh, s, n = ([c[k] for c in cases] for k in range(3))
    r1, s1 = M.energy_ratios_batch(sh, s, n, return_sums=True)
    r2, s2 = M.energy_ratios_batch(sh, s, n, return_sums=True)
    assert torch.equal(r1, r2) and torch.equal(s1, s2)
    for u in (0, 17, 100, 255):
        ra, sa = M.energy_ratios_batch([sh[u]], [s[u]], [n[u]], return_sums=True)
        assert torch.equal(ra[0], r1[u]) and torch.equal(sa[0], s1[u]), u
    check_ratios(r1[100].cpu().numpy(), MB.exact(*cases[100]), what="utterance 100 of 256")


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------------

def test_degenerate_inputs_follow_numpy():
    _, s, n = mixture(5000, 21)
    z = np.zeros(5000)
    e0, e1 = np.array([1.0, -2.0, 0.5]), np.array([3.0, 1.0, -1.0])
    cases = [(2.0 * e0, e0, e1),       # a perfect estimate (alpha_s = 10.5 / 5.25 = 2 and the residual 0 in any summation order): +inf
             (s, z, n),                # all-zero s: alpha_s = 0 / 0
             (s + n, s, z),            # all-zero n: alpha_n = 0 / 0, which numpy carries into e_noise + e_art as well
             (z, s, n),                # all-zero estimate: 0 / 0 in every ratio
             (z[:3], e0, z[:3])]
    got = M.energy_ratios_batch(*([c[k] for c in cases] for k in range(3))).cpu().numpy()
    with np.errstate(all="ignore"):
        want = np.array([PM.energy_ratios(*c) for c in cases])
    print(got, want, sep="\n")
    for name, pred in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(pred(got), pred(want)), name
    assert np.isposinf(got[0, 0]) and np.isfinite(got[0, 1:]).all() and np.isnan(got[1:]).all()
    assert torch.isposinf(M.si_sdr_batch([2.0 * e0], [e0])).all() and torch.isnan(M.si_sdr_batch([s], [z])).all()


# ---- past 2^31 bytes -------------------------------------------------------------------------------------------------------------------

def test_packed_buffers_past_two_gib():
    U, L = 6800, 80000                                                                        # 6 800 x 5 s: 2.18e9 bytes per float32 buffer
    total = U * L
    assert total * 4 > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(5)
    s = torch.empty(total, dtype=torch.float32, device="cuda").normal_(0, 0.1, generator=g)
    n = torch.empty(total, dtype=torch.float32, device="cuda").normal_(0, 0.05, generator=g)
    sh = torch.empty(total, dtype=torch.float32, device="cuda").normal_(0, 0.02, generator=g)
    sh.add_(s, alpha=0.8).add_(n, alpha=0.3)
    offs, lens = [u * L for u in range(U)], [L] * U
    ratios, sums = M.energy_ratios_batch(H.WaveBatch(sh, offs, lens), H.WaveBatch(s, offs, lens), H.WaveBatch(n, offs, lens), return_sums=True)
    assert bool(torch.isfinite(ratios).all())
    mark = 2 ** 31 // (4 * L)                                                                 # the utterance that straddles the 2^31-byte mark
    k = MB.items(L)
    for u in (0, mark - 1, mark, mark + 1, U - 1):
        a, b, c = (t[u * L:(u + 1) * L].double() for t in (sh, s, n))
        row = sums[u].cpu().numpy()
        # torch.float64 dot products (their own error at most L u sum |t_i| in any order) against the device's (70 + k) u sum |t_i|
        for key, x, y in (("dot_s", a, b), ("ss", b, b), ("dot_n", a, c), ("nn", c, c)):
            ref, mag = float(torch.dot(x, y)), float(torch.dot(x.abs(), y.abs()))
            tol = MB.SLACK * (L + 70 + k) * MB.U * mag
            print(u, key, "difference", row[COLS[key]] - ref, "bound", tol)
            assert abs(row[COLS[key]] - ref) <= tol, (u, key)
        if u in (mark, U - 1):
            check_ratios(ratios[u].cpu().numpy(), MB.exact(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()), what=f"utterance {u}")


# ---- McemBatch.score -------------------------------------------------------------------------------------------------------------------

def test_mcem_batch_score_equals_the_scores_of_its_waveforms():
    from packages.models.models import DeepGenerativeModel
    McemBatch = importlib.import_module("disentangled-vae_amd.mcem").McemBatch
    torch.manual_seed(0)
    vae = DeepGenerativeModel([513, 1, 16, [128, 128]], None).cuda().eval()
    for p in vae.parameters():
        p.requires_grad = False
    lengths = [16000, 20000, 12345]
    parts = [mixture(L, 40 + i, snr_db=5.0) for i, L in enumerate(lengths)]
    speech, noise = [p[1] for p in parts], [0.3 * p[2] for p in parts]
    waves = [a + b for a, b in zip(speech, noise)]
    X = H.stft_batch(waves, center=False, pad_at_end=True)
    Y = [np.ones((1, T), np.float32) for T in X.counts]
    mb = McemBatch(vae, niter=2, nsamples_E_step=2, burnin_E_step=2, nsamples_WF=2, burnin_WF=2)
    mb.init_parameters(X, Y)
    mb.run()
    got = mb.score(speech, noise, max_len=lengths, trim=800)
    assert got.shape == (3, 3) and got.is_cuda and got.dtype == torch.float64
    leroux = mb.score(speech, max_len=lengths, trim=800).cpu().numpy()
    assert leroux.shape == (3,)
    s_hat, _ = mb.enhance(max_len=lengths)
    got = got.cpu().numpy()
    for u, w in enumerate(s_hat.numpy()):
        c = (w.astype(np.float64)[800:-800], speech[u][800:-800], noise[u][800:-800])
        q = MB.exact(*c)
        check_ratios(got[u], q, what=f"utterance {u}")
        check_ratios([leroux[u]], MB.exact(c[0], c[1]), what=f"utterance {u} (no n)")
        host = PM.energy_ratios(*c)                                                            # the path it replaces
        ref, dev = MB.ref_db(q), MB.bound_db(q)
        for i, (ratio, _) in enumerate(MB.RATIOS):
            assert abs(got[u, i] - host[i]) <= dev[ratio] + ref[ratio], (u, ratio)
