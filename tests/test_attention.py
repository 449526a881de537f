"""CPU: the host model of the fused attention (tests/_attention_ref.py) against the reference's float64 records, the keep
rates of the restated dropout draw, the tolerance of the GPU tests (measured here from the torch composition, never from
the kernel), and three faults that must leave that tolerance on the GPU test's inputs."""
import numpy as np
import pytest

import _paths  # noqa: F401
import _attention_ref as R
import _bert4rec_golden as G
from fbgemm_gpu import _lib

# 8 x the worst float32-vs-float64 error of the torch composition over the GPU ABI test's inputs, as first measured
# (BERT4Rec); the measurement must stay within a factor 2 of it on any host.
DOCUMENTED_TOLERANCE = 9.0e-5


def _supported(L, d):
    return bool(_lib.load().tbe_attention_supported(L, d))


def _extra():
    return ((1, 1, R.max_L(_supported, 128), 128),)


def test_support_rule_covers_the_documented_range():
    assert _supported(100, 128) and _supported(200, 64)
    for d in range(4, 129, 4):
        assert _supported(1, d) and _supported(64, d), d
    for L, d in ((0, 8), (8, 0), (8, 6), (8, 132), (257, 4), (-1, 8), (200, 128)):
        assert not _supported(L, d), (L, d)
    assert 128 <= R.max_L(_supported, 128) < 200


@pytest.mark.parametrize("case", G.cases("mha"))
def test_host_model_agrees_with_the_reference_float64_records(case):
    z, pre = G.load(), f"mha|{case}|"
    xq, xk, xv, g, rows = (np.asarray(a, np.float64) if i < 4 else a for i, a in enumerate(G.mha_inputs(case)))
    P = {n: v.astype(np.float64) for n, v in G.params("mha", case).items()}
    valid = z[pre + "valid"]
    B, L, dim = xq.shape
    H = int(case.split("h")[-1])
    proj = [x @ P[f"linear_layers.{i}.weight"].T + P[f"linear_layers.{i}.bias"] for i, x in enumerate((xq, xk, xv))]
    q, k, v = (t.reshape(B, L, H, dim // H) for t in proj)
    att, _, _ = R.forward(q, k, v, valid)
    out = att.reshape(B, L, dim) @ P["output_linear.weight"].T + P["output_linear.bias"]
    np.testing.assert_allclose(out[:, rows], z[pre + "f64|out"], rtol=1e-9, atol=1e-11)
    datt = (g @ P["output_linear.weight"]).reshape(B, L, H, dim // H)
    grads = [t.reshape(B, L, dim) for t in R.backward(datt, q, k, v, valid)]
    for i, (n, x) in enumerate(zip(("gxq", "gxk", "gxv"), (xq, xk, xv))):
        np.testing.assert_allclose((grads[i] @ P[f"linear_layers.{i}.weight"])[:, rows], z[pre + "f64|" + n], rtol=1e-9,
                                   atol=1e-11)
        gw = np.einsum("blo,bli->oi", grads[i], x)
        np.testing.assert_allclose(G.stored_grad(gw), z[pre + f"f64|grad|linear_layers.{i}.weight"], rtol=1e-9, atol=1e-10)


def test_keep_rate_of_the_restated_draw():
    """|rate - (1 - p)| <= 5 sqrt(p (1 - p) / n) for every (p, seed, call, shape) the GPU tests draw with."""
    shapes = [(3, 2, 7, 8), (2, 2, 65, 64), (1, 2, 100, 128)]
    for p, seed, call in R.DROPOUT:
        for B, H, L, d in shapes:
            for c in (call, call + 1):
                kept = R.dropout_draws(seed, c, B, H, L) >= np.uint32(R.dropout_threshold(p))
                n = kept.size
                assert abs(kept.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (p, seed, c, (B, H, L), kept.mean())
    assert R.dropout_threshold(0.0) == 0 and R.dropout_threshold(0.1) == 429496736
    assert int(R.fmix32(np.uint32(1))) == 0x514E28B7  # murmur3's finalizer


def test_tolerance_of_the_gpu_tests_is_measured_from_the_torch_composition():
    tol = R.measured_tolerance(_extra())
    print(f"measured tolerance (8 x worst float32 error of the torch composition): {tol:.3e}")
    assert DOCUMENTED_TOLERANCE / 2 <= tol <= DOCUMENTED_TOLERANCE * 2, tol


def _outputs(q, k, v, g, valid, **fault):
    fwd = {n: fault[n] for n in ("masked_value", "subtract_max", "dtype") if n in fault}
    bwd = {n: fault[n] for n in ("cut_masked",) if n in fault}
    out = R.forward(q, k, v, valid, None, **fwd)[0]
    return (out, *R.backward(g, q, k, v, valid, None, **bwd))


def _leaves(right, wrong, tol):
    with np.errstate(invalid="ignore"):
        return any(not (np.abs(w - r).max() / R.scale_of(r) <= tol) for r, w in zip(right, wrong))


def test_three_faults_leave_the_tolerance_on_the_gpu_tests_inputs():
    tol = R.measured_tolerance(_extra())
    B, H, L, d = 3, 2, 7, 8
    q, k, v, g = R.make_inputs(B, H, L, d)
    valid = R.key_valid("per_sample", B, L)
    right = _outputs(q, k, v, g, valid)
    # the -1e9 rule dropped: -inf for the sample with no valid key (NaN), or zero weight (O = 0 instead of the mean of V)
    assert _leaves(right, _outputs(q, k, v, g, valid, masked_value=-np.inf), tol)
    zero_weight = [a.copy() for a in right]
    zero_weight[0][0] = 0
    assert _leaves(right, zero_weight, tol)
    # dS let through at masked keys: shows where masked keys carry weight, the sample with no valid key
    assert _leaves(right, _outputs(q, k, v, g, valid, cut_masked=False), tol)
    # no row-maximum subtraction: float32 exp overflows once a score passes 88.7
    qh, kh, vh, gh = R.make_inputs(*R.HOT, 6.0)
    assert np.abs(np.einsum("bihc,bjhc->bhij", qh.astype(np.float64), kh) / np.sqrt(R.HOT[3])).max() > 100
    hot_right = _outputs(qh, kh, vh, gh, None)
    assert not _leaves(hot_right, _outputs(qh, kh, vh, gh, None, dtype=np.float32), 1e-3)  # float32 with the maximum: fine
    assert _leaves(hot_right, _outputs(qh, kh, vh, gh, None, dtype=np.float32, subtract_max=False), tol)
