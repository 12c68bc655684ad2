"""tests/grad_columns.py on the CPU: the restatements against float64, the gap the per-column measure closes (seeded faults that the
tensor-level figure of the other tests cannot see), the zero-column rule, and the oracle's operand hook at its default."""
import numpy as np
import pytest

import golden_util as gu
import grad_columns as gc
from oracle import vae_oracle as vo

W1 = "encoder.hidden.0.weight"
TENSOR_TOL = 5e-5                    # X3_TOL of tests/test_gpu_fused.py: the tightest tensor-level bound in force
CASES = [(f, m, y, 1000) for f in ("bench", "speech") for m, y in (("M1", 0), ("M2", 1), ("M2", 513))]


def _ids(case):
    return "{}-{}-y{}-B{}".format(*case) if isinstance(case, tuple) else None


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_restatements_stay_inside_their_own_bound(case):
    """A second draw of every restatement -- the same step on the frames in another order, i.e. other sums of the same terms -- stays
    inside the bound made from the first; no column that is zero in float64 is anything else in a restatement; and the conditions the
    inputs were chosen for hold."""
    r = gc.reference(*case)
    perm = np.random.default_rng(5).permutation(r.B)
    x, e = r.x[perm], r.e[perm]
    y = None if r.y is None else r.y[perm]
    again = {"fp32": gc.oracle_grads(r.model, r.params, x, y, e, dtype=np.float32)}
    for name, make in gc.POLICIES.items():
        again[name] = gc.oracle_grads(r.model, r.params, x, y, e, hook=make())
    for precision, g in again.items():
        fails, top = gc.check(g, r, precision, label=f"{precision:6s}")
        assert not fails, fails
    for precision in r.figures:
        assert all(f["zero_ok"] for f in r.figures[precision].values())
    top = np.abs(r.truth[W1]).max(axis=0)
    quiet = float(np.mean(top < TENSOR_TOL * top.max()))
    worst32 = max(f["worst"] for f in r.figures["fp32"].values())
    print(f"columns of {W1} below 5e-5 of the tensor's maximum: {100 * quiet:.1f} %; float32 restatement, worst column of any tensor: {worst32:.2e}")
    if r.family == "speech":
        assert 0.2 <= quiet <= 0.5 and worst32 <= 3.5e-5


def _exceeds(r, g, precisions=("fp32", "bf16x3")):
    """the figures of the faulty tensor g (encoder layer 1's weight) and whether they break the per-column bound of every given policy"""
    f = gc.column_figures(g, r.truth[W1])
    out = []
    for p in precisions:
        bw, bm = gc.bound(r.figures["fp32"][W1], None if p == "fp32" else r.figures[p][W1])
        out.append(f["worst"] > bw or f["median"] > bm)
    return f, all(out)


def _layer1_terms(r):
    """float64 dpre and input of encoder layer 1 (through the hook, products left exact)"""
    class Capture:
        fwd = staticmethod(lambda name, x, W: x @ W.T)
        bias = staticmethod(lambda name, dpre: dpre.sum(axis=0))
        bwd = staticmethod(lambda name, dpre, W: dpre @ W)

        def wgrad(self, name, dpre, inp):
            if name == "encoder.hidden.0":
                self.got = (dpre, inp)
            return dpre.T @ inp
    cap = Capture()
    gc.oracle_grads(r.model, r.params, r.x, r.y, r.e, hook=cap)
    return cap.got


@pytest.mark.parametrize("case", [("bench", "M2", 513, 33), ("bench", "M2", 513, 1000)], ids=_ids)
def test_label_columns_off_by_one_percent_pass_the_tensor_level_bound_only(case):
    r = gc.reference(*case)
    g = r.truth[W1].copy()
    g[:, gc.XD:] *= 1.01
    f, caught = _exceeds(r, g)
    print(f"label columns x 1.01: worst column {f['worst']:.2e}, median {f['median']:.2e}, tensor-level {f['tensor']:.2e}")
    assert f["tensor"] < TENSOR_TOL and caught and f["worst"] > 9e-3


@pytest.mark.parametrize("case", [("bench", "M2", 513, 33), ("bench", "M2", 513, 1000), ("speech", "M2", 513, 33), ("speech", "M1", 0, 1000)], ids=_ids)
def test_an_unwritten_quiet_column_passes_the_tensor_level_bound_only(case):
    r = gc.reference(*case)
    g = r.truth[W1].copy()
    q = int(np.argmin(np.abs(g[:, :gc.XD]).max(axis=0)))
    g[:, q] = 0.0
    f, caught = _exceeds(r, g)
    print(f"column {q} zeroed: worst column {f['worst']:.2e}, tensor-level {f['tensor']:.2e}")
    assert f["tensor"] < TENSOR_TOL and caught and f["worst"] == 1.0 and f["arg"] == q


@pytest.mark.parametrize("case", [("speech", "M2", 513, 1000), ("speech", "M1", 0, 1000)], ids=_ids)
@pytest.mark.parametrize("fault", ["bf16", "f16"])
def test_a_coarser_weight_gradient_x_operand_shows_per_column(case, fault):
    """The x operand of the layer-1 weight gradient without its lo plane (one bf16), or rebuilt from the forward's fixed-scale fp16 planes
    (which flush quiet bins).  On the upper half of the spectrum (bins 256 ..., 30 dB and more below the first) either one stays under the
    tensor-level bound and breaks the per-column one.  On every bin, the missing lo plane reaches 3.1e-3 ... 3.4e-3 of the tensor's maximum
    (the loud columns carry it: the tensor-level tests see that one), the fp16 planes still stay under it."""
    r = gc.reference(*case)
    for k0 in (256, 0):
        hook = gc.OperandPolicy(2, True, wgrad_x=fault, wgrad_x_from=k0)
        g = gc.oracle_grads(r.model, r.params, r.x, r.y, r.e, hook=hook)[W1]
        f, caught = _exceeds(r, g, ("bf16x3",))
        print(f"{fault} planes from bin {k0}: worst column {f['worst']:.2e} at {f['arg']}, median {f['median']:.2e}, tensor-level {f['tensor']:.2e}")
        assert caught
        if k0 or fault == "f16":
            assert f["tensor"] < TENSOR_TOL


@pytest.mark.parametrize("case", [("bench", "M2", 513, 33), ("speech", "M2", 513, 33)], ids=_ids)
def test_a_frame_missing_from_one_column_block_passes_the_tensor_level_bound_only(case):
    """33 frames: the last one is alone in the second 32-frame tile.  Left out of the sums of bins 480 .. 511 (one 32-column block)."""
    r = gc.reference(*case)
    dpre, inp = _layer1_terms(r)
    g = r.truth[W1].copy()
    g[:, 480:512] -= np.outer(dpre[-1], inp[-1, 480:512])
    f, caught = _exceeds(r, g)
    print(f"last frame left out of bins 480 .. 511: worst column {f['worst']:.2e} at {f['arg']}, tensor-level {f['tensor']:.2e}")
    assert f["tensor"] < TENSOR_TOL and caught and 480 <= f["arg"] < 512


def test_zero_columns_must_be_exactly_zero():
    """One frame of M2 y 513: the columns of the labels that are 0 in that frame have an identically zero gradient (about 70 % of the label
    columns); every restatement leaves them exactly zero, and a gradient that does not is refused whatever its size."""
    r = gc.reference("bench", "M2", 513, 1)
    G = r.truth[W1]
    zero = np.flatnonzero(np.abs(G).max(axis=0) == 0)
    assert np.array_equal(zero, gc.XD + np.flatnonzero(r.y[0] == 0)) and zero.size > 300
    for p, figs in r.figures.items():
        assert figs[W1]["zero_ok"] and abs(figs[W1]["zero_share"] - zero.size / G.shape[1]) < 1e-12, p
    g = {k: v.copy() for k, v in r.truth.items()}
    fails, _ = gc.check(g, r, "fp32")
    assert not fails
    g[W1][5, zero[0]] = 1e-30
    fails, _ = gc.check(g, r, "bf16")
    assert [k for k, _ in fails] == [W1] and "identically zero" in fails[0][1]


@pytest.mark.parametrize("model,y_dim", [("M1", 0), ("M2", 513), ("M2_info", 1)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_operand_hook_at_its_default_changes_no_bit(model, y_dim, dtype):
    """No hook (the default), and a hook that forms the four products as the oracle writes them, against the products written out here:
    the same bits in every gradient."""
    dims = gc.dims_of(y_dim)
    params = {k: v.astype(dtype) for k, v in gu.make_params(model, dims, 3).items()}
    x, y, e = (None if a is None else a.astype(dtype) for a in gu.make_batch(dims, 50, 4))

    class Plain:
        fwd = staticmethod(lambda name, x, W: x @ W.T)
        wgrad = staticmethod(lambda name, dpre, inp: dpre.T @ inp)
        bias = staticmethod(lambda name, dpre: dpre.sum(axis=0))
        bwd = staticmethod(lambda name, dpre, W: dpre @ W)

    def run():
        if model == "M2_info":
            out, g1, g2 = vo.m2info_losses_and_grads(params, x, y, e, 0.5, 10.0, 1.0)
            return dict(g1, **{"second." + k: v for k, v in g2.items()}), out["enc_loss"]
        out, g = vo.vae_loss_and_grads(model, params, x, y, e)
        return g, out["loss"]

    assert vo._GEMM_HOOK is None
    g0, l0 = run()
    with vo.gemm_hook(Plain()):
        g1, l1 = run()
    assert vo._GEMM_HOOK is None
    # the layer written out: what linear() and linear_bwd() computed before they had a hook
    W, b = params["encoder.hidden.0.weight" if model != "M2_info" else "enc_dec_clf.encoder.hidden.0.weight"], params["encoder.hidden.0.bias" if model != "M2_info" else "enc_dec_clf.encoder.hidden.0.bias"]
    inp = x if model != "M2" else np.concatenate([x, y], axis=1)
    assert np.array_equal(vo.linear(inp, W, b), inp @ W.T + b)
    grads = {}
    d = np.ones((50, 128), dtype) * dtype(0.25)
    dx = vo.linear_bwd({"l.weight": W}, grads, "l", inp, d)
    assert np.array_equal(grads["l.weight"], d.T @ inp) and np.array_equal(grads["l.bias"], d.sum(axis=0)) and np.array_equal(dx, d @ W)
    assert l0 == l1 and g0.keys() == g1.keys()
    for k in g0:
        assert np.array_equal(g0[k], g1[k]) and g0[k].dtype == dtype, k
