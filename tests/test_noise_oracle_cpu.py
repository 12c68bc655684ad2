"""Pins oracle/noise_oracle.py (the float64 restatement of the in-kernel reparametrisation noise) so that the GPU tests in
test_gpu_noise.py compare the device against something known to be right: the published Philox known answers, the counter layout,
the edges of the uniform quantisation, and the distribution / independence of the streams the trainer actually uses (fixed seeds:
deterministic; the device inherits these properties through the per-element comparison, without a statistical test on the GPU).

Wall time of this file: about 20 s on one core (the oracle costs ~0.25 us per Philox block)."""
import functools
import itertools

import numpy as np
import pytest

import noise_cases as nc
from oracle import noise_oracle as no

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox4x32_10_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    got = no.philox4x32_10(ctr, key)
    assert " ".join("%08x" % int(w) for w in got) == want


def test_philox_is_vectorised():
    c = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    k = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = np.stack(no.philox4x32_10(c, k), axis=-1)
    want = np.array([[int(w, 16) for w in k[2].split()] for k in KAT], dtype=np.uint64)
    assert np.array_equal(got, want)


# ---- counter layout ----
BASE = dict(seed=(0x13572468 << 32) | 0x9abcdef0, frame=(5 << 32) | 77, step=(3 << 32) | 1234, draw=1)
VARIANTS = {"seed lo": dict(seed=BASE["seed"] ^ 1), "seed hi": dict(seed=BASE["seed"] ^ (1 << 32)), "seed top bit": dict(seed=BASE["seed"] ^ (1 << 63)),
            "frame lo": dict(frame=BASE["frame"] + 1), "frame hi": dict(frame=BASE["frame"] + (1 << 32)),
            "step lo": dict(step=BASE["step"] + 1), "step hi": dict(step=BASE["step"] + (1 << 32)), "step bit 55": dict(step=BASE["step"] ^ (1 << 55)),
            "draw": dict(draw=2), "draw 0": dict(draw=0), "draw 3": dict(draw=3)}


def _w(seed, frame, step, draw):
    return no.words(seed, frame, step, draw).reshape(4)


@pytest.mark.parametrize("which", list(VARIANTS))
def test_every_field_of_key_and_counter_reaches_all_four_words(which):
    a, b = _w(**BASE), _w(**{**BASE, **VARIANTS[which]})
    assert np.all(a != b), (which, a, b)
    # and it is a different STREAM, not a shifted one: the normals differ in every element too
    assert np.all(no.box_muller(no.uniforms(a)) != no.box_muller(no.uniforms(b)))


def test_counter_words_are_the_documented_slots():
    seed, frame, step = (0xAAAA5555 << 32) | 0x12345678, (0x00000009 << 32) | 0x80000001, (0x00ABCDEF << 32) | 0xFEDCBA98
    c = [int(v) for v in no.counter(frame, step, 3)]
    assert c == [0x80000001, 0x00000009, 0xFEDCBA98, (0x00ABCDEF << 8) | 3]
    assert [int(v) for v in no.key(seed)] == [0x12345678, 0xAAAA5555]
    # the words are what Philox gets, in this order
    assert np.array_equal(_w(seed, frame, step, 3), np.array([int(v) for v in no.philox4x32_10(c, no.key(seed))], dtype=np.uint64))


def test_step_high_word_and_draw_never_collide():
    """c3 = (step hi << 8) | draw is one-to-one on step hi < 2^24, draw < 4 (all 2^26 pairs), and stays inside 32 bits."""
    for lo in range(0, 1 << 24, 1 << 22):
        s = np.arange(lo, lo + (1 << 22), dtype=np.uint64)
        for d in range(4):
            c3 = no.counter(0, s << np.uint64(32), d)[3]
            assert np.array_equal(c3 >> np.uint64(8), s) and np.all((c3 & np.uint64(0xff)) == np.uint64(d))


def test_evaluation_steps_are_disjoint_from_training_steps():
    assert no.EVAL_BASE == 1 << 40
    for k in (1, 2, 3, 1 << 20, (1 << 40) - 1):
        e = no.eval_step(k)
        assert e == (1 << 40) + k and e >= 1 << 40                     # above every training step < 2^40 ...
        c_eval = [int(v) for v in no.counter(0, e, 0)]
        c_train = [int(v) for v in no.counter(0, k, 0)]
        assert c_eval[2] == c_train[2] and c_eval[3] != c_train[3]     # ... and the difference sits in the step-hi slot
        assert c_eval[3] == ((e >> 32) << 8)
    # all training steps < 2^40 have step hi < 2^8; evaluation steps 2^40 + k (k < 2^40) have step hi in [2^8, 2^9)
    assert ((1 << 40) - 1) >> 32 < 1 << 8 <= no.eval_step(1) >> 32


def test_rank_seed():
    assert no.rank_seed(5, 0) == 5
    assert no.rank_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert no.rank_seed((1 << 64) - 1, 1) == 0x9E3779B97F4A7C14         # wraps mod 2^64
    assert len({no.rank_seed(0, r) for r in range(8)}) == 8
    assert all(no.rank_seed(0, r) >> 32 != 0 for r in range(1, 8))        # ranks differ in the HIGH key word as well


# ---- quantisation edges ----
def test_uniform_quantisation_edges():
    w = np.array([0x00000000, 0x000000ff, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint64)
    u = no.uniforms(w)
    assert u.dtype == np.float32
    assert np.all(np.isfinite(u)) and np.all(u > 0) and np.all(u <= 1)
    assert u[0] == u[1] == np.float32(2.0 ** -25)                        # the minimum; the low 8 bits are not used
    assert u[4] == np.float32(1.0)                                       # 2^24 - 1 + 0.5 rounds to 2^24
    assert u[2] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24) and u[3] == np.float32(0.5)      # 2^23 - 1 + 0.5 is exact; 2^23 + 0.5 is a tie -> 2^23
    # float32 arithmetic, not exact: on the upper half of the range the + 0.5 rounds away
    k = np.array([(1 << 23) + 1, (1 << 23) + 2, (1 << 24) - 2], dtype=np.uint64)
    assert np.array_equal(no.uniforms(k << np.uint64(8)), np.array([(1 << 23) + 2, (1 << 23) + 2, (1 << 24) - 2], dtype=np.float32) * np.float32(2.0 ** -24))
    z = no.box_muller(no.uniforms(np.array([[0, 0, 0xffffffff, 0x40000000]], dtype=np.uint64)))[0]
    rmax = np.sqrt(50 * np.log(2))
    assert np.all(np.isfinite(z)) and abs(z[0] - rmax) < 1e-12 and abs(z[1] - rmax * 2 * np.pi * 2.0 ** -25) < 1e-12 and z[2] == 0.0 and z[3] == 0.0
    allw = no.box_muller(no.uniforms(np.random.default_rng(0).integers(0, 1 << 32, (1 << 16, 4), dtype=np.uint64)))
    assert np.abs(allw).max() <= rmax


@pytest.mark.parametrize("kind", list(nc.EXTREME))
def test_committed_extreme_counters_are_extreme(kind):
    """The (seed, step, frame, draw, pair) the device test asks for really hold the edge words (found by noise_cases.find_extremes)."""
    assert len(nc.EXTREME[kind]) >= 2
    for seed, step, frame, draw, pair in nc.EXTREME[kind]:
        assert frame < nc.SEARCH_FRAMES
        k = _w(seed, frame, step, draw) >> np.uint64(8)
        z = no.normals(seed, [frame], step)[0]
        c0, c1 = nc.element_columns(draw, pair)
        assert np.all(np.isfinite(z))
        if kind == "radius_min":
            assert int(k[2 * pair]) == 0
            assert abs(np.hypot(z[c0], z[c1]) - np.sqrt(50 * np.log(2))) < 1e-12
        elif kind == "radius_one":
            assert int(k[2 * pair]) == nc.TOP
            assert z[c0] == 0.0 and z[c1] == 0.0
        else:
            assert int(k[2 * pair + 1]) == nc.TOP
            u = no.uniforms(_w(seed, frame, step, draw))
            assert u[2 * pair + 1] == np.float32(1.0)
            r = np.sqrt(-2 * np.log(np.float64(u[2 * pair])))
            assert abs(z[c0] - r) < 1e-12 and abs(z[c1]) < 1e-14      # angle 2 pi: (cos, sin) = (1, 0) to float64 rounding


def test_search_finds_the_committed_counters():
    """The search function next to the constants, on the one step of the first hit of each kind."""
    for kind, hits in nc.EXTREME.items():
        seed, step = hits[0][0], hits[0][1]
        found = nc.find_extremes(seed=seed, steps=[step], per_kind=1)
        assert found[kind] == [hits[0]], (kind, found)


# ---- feature layout ----
def test_feature_layout_of_the_four_draws():
    seed, step, frames = 99, 5, np.arange(64)
    z = no.normals(seed, frames, step)
    assert z.shape == (64, 16) and z.dtype == np.float64
    for draw, f0 in enumerate((0, 8, 4, 12)):
        assert np.array_equal(z[:, f0:f0 + 4], no.box_muller(no.uniforms(no.words(seed, frames, step, draw))))
    u = no.uniforms(no.words(seed, frames, step, 2)).astype(np.float64)
    np.testing.assert_allclose(z[:, 4], np.sqrt(-2 * np.log(u[:, 0])) * np.cos(2 * np.pi * u[:, 1]), rtol=0, atol=1e-15)
    np.testing.assert_allclose(z[:, 7], np.sqrt(-2 * np.log(u[:, 2])) * np.sin(2 * np.pi * u[:, 3]), rtol=0, atol=1e-15)
    # a frame's row does not depend on which other frames are asked for
    assert np.array_equal(no.normals(seed, [63, 0, 17], step), z[[63, 0, 17]])


# ---- distribution of the streams the trainer uses ----
SEED_A = 0x0123456789ABCDEF
STEP_A = 1
NF = 1 << 20              # frames of the moment / KS tests: 2^24 elements
NC = 1 << 18              # frames of the correlation streams: 2^22 elements each


@functools.lru_cache(maxsize=None)
def _stream(seed, step, n):
    return no.normals(seed, np.arange(n, dtype=np.uint64), step)


def _moments_and_ks(z, what):
    from scipy import stats
    z = np.asarray(z).ravel()
    n = z.size
    mean, var = z.mean(), z.var()
    p = stats.kstest(z, "norm").pvalue
    print(f"{what}: n {n} mean {mean:+.3e} (bound {5 / np.sqrt(n):.3e}) var-1 {var - 1:+.3e} (bound {5 * np.sqrt(2 / n):.3e}) KS p {p:.3f}")
    assert abs(mean) <= 5 / np.sqrt(n), (what, mean)
    assert abs(var - 1) <= 5 * np.sqrt(2 / n), (what, var)
    assert p > 1e-3, (what, p)


def _corr(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def _assert_uncorrelated(a, b, what):
    n = np.asarray(a).size
    c = _corr(a, b)
    print(f"{what}: n {n} corr {c:+.3e} (bound {5 / np.sqrt(n):.3e})")
    assert abs(c) <= 5 / np.sqrt(n), (what, c)


def test_oracle_stream_is_standard_normal():
    _moments_and_ks(_stream(SEED_A, STEP_A, NF), "all 2^24 elements")


@pytest.mark.parametrize("col", range(16))
def test_each_latent_feature_is_standard_normal(col):
    _moments_and_ks(_stream(SEED_A, STEP_A, NF)[:, col], f"feature {col}")


def test_latent_features_are_pairwise_uncorrelated():
    """Two features sharing a draw or an output (features 4..7 = features 8..11, feature j + 1 = feature j) would show as correlation 1."""
    z = _stream(SEED_A, STEP_A, NF)
    c = np.corrcoef(z.T)
    off = np.abs(c - np.eye(16)).max()
    print(f"largest off-diagonal feature correlation {off:.3e} (bound {5 / np.sqrt(NF):.3e})")
    assert off <= 5 / np.sqrt(NF)
    assert not any(np.array_equal(z[:, i], z[:, j]) for i, j in itertools.combinations(range(16), 2))


def test_cos_and_sin_halves_of_a_draw_are_uncorrelated():
    z = _stream(SEED_A, STEP_A, NF)
    _assert_uncorrelated(z[:, 0::2], z[:, 1::2], "cos vs sin")


def test_adjacent_frames_are_uncorrelated():
    z = _stream(SEED_A, STEP_A, NF)
    _assert_uncorrelated(z[:-1], z[1:], "frame b vs b + 1")
    _assert_uncorrelated(z[:-32], z[32:], "frame b vs b + 32 (the next tile)")


def test_adjacent_steps_are_uncorrelated():
    _assert_uncorrelated(_stream(SEED_A, STEP_A, NC), _stream(SEED_A, STEP_A + 1, NC), "step 1 vs 2")
    _assert_uncorrelated(_stream(SEED_A, (1 << 32) - 1, NC), _stream(SEED_A, 1 << 32, NC), "step 2^32 - 1 vs 2^32")


def test_training_and_evaluation_steps_are_uncorrelated():
    for s in (1, 2):
        _assert_uncorrelated(_stream(SEED_A, s, NC), _stream(SEED_A, no.eval_step(s), NC), f"step {s} vs 2^40 + {s}")


def test_seeds_differing_in_the_high_word_are_uncorrelated():
    _assert_uncorrelated(_stream(SEED_A, STEP_A, NC), _stream(SEED_A ^ (1 << 32), STEP_A, NC), "seed vs seed ^ 2^32")
    _assert_uncorrelated(_stream(7, STEP_A, NC), _stream(7 + (1 << 63), STEP_A, NC), "seed 7 vs 7 + 2^63")


def test_rank_streams_are_pairwise_uncorrelated():
    base = 1234
    z = [_stream(no.rank_seed(base, r), STEP_A, NC) for r in range(8)]
    for i, j in itertools.combinations(range(8), 2):
        _assert_uncorrelated(z[i], z[j], f"rank {i} vs {j}")
