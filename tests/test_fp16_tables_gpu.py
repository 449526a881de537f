"""GPU parity of the FP16-table kernels (tbe_*_f16w) against the CPU oracle run on the up-cast tables.

Forward: the arithmetic is the FP32 kernels' (sequential fmaf in bag order on float(w16)), so the output is bit-identical
to the oracle wherever the FP32 kernels are.  Backward: the update is computed in FP32 and only the final store converts,
so with nearest-even rounding a stored weight is within half an FP16 ulp of the FP32 result (plus the FP32 backward's own
tolerance), and with stochastic rounding it is one of the two FP16 neighbours of the FP32 result."""
import math

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
from _util import make_inputs, oracle_forward_mixed, to_dev
from oracle import oracle

pytestmark = pytest.mark.gpu

# the shapes of tests/test_tbe_gpu.py CASES
CASES = [
    # rows, dims, ftm, B, max_len, fixed_len, weighted, pooling
    dict(rows=[100, 7, 3000], dims=[128, 128, 128], ftm=None, B=300, max_len=1, fixed_len=1, weighted=False, pooling=0),
    dict(rows=[50, 9], dims=[64, 32], ftm=[0, 1, 0], B=65, max_len=5, fixed_len=None, weighted=False, pooling=0),
    dict(rows=[50, 9, 11], dims=[16, 256, 8], ftm=None, B=130, max_len=4, fixed_len=None, weighted=True, pooling=0),
    dict(rows=[33, 200], dims=[512, 40], ftm=None, B=70, max_len=3, fixed_len=None, weighted=False, pooling=1),
    dict(rows=[20, 15], dims=[1024, 12], ftm=None, B=19, max_len=2, fixed_len=None, weighted=True, pooling=1),
    dict(rows=[12, 40], dims=[7, 13], ftm=None, B=37, max_len=4, fixed_len=None, weighted=False, pooling=0),  # D % 4 != 0
    dict(rows=[64], dims=[2048], ftm=None, B=5, max_len=3, fixed_len=None, weighted=False, pooling=0),
    dict(rows=[500, 30], dims=[128, 64], ftm=None, B=33, max_len=60, fixed_len=None, weighted=False, pooling=0),  # long-bag kernel
    dict(rows=[500, 30], dims=[32, 256], ftm=None, B=17, max_len=70, fixed_len=None, weighted=True, pooling=1),  # long-bag, weighted mean
]

OPTS = [
    ("EXACT_SGD", {}),
    ("EXACT_ROWWISE_ADAGRAD", dict(eps=1e-3)),
    ("EXACT_ROWWISE_ADAGRAD", dict(eps=1e-3, weight_decay=0.01, weight_decay_mode=1)),  # WeightDecayMode.L2
    ("EXACT_ADAGRAD", dict(eps=1e-3)),
    ("ADAM", dict(eps=1e-3, weight_decay=0.02)),
]


def _opt(name):
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    return getattr(EmbOptimType, name)


def build_pair16(rows, dims, ftm, pooling, optimizer=None, rng=None, locations=None, **kw):
    """(FP16-table module on cuda:0, oracle Tables holding the same values up-cast to float32)."""
    from fbgemm_gpu.split_embedding_configs import EmbOptimType, SparseType
    from fbgemm_gpu.split_table_batched_embeddings_ops import (
        ComputeDevice, EmbeddingLocation, PoolingMode, SplitTableBatchedEmbeddingBagsCodegen)

    pm = {0: PoolingMode.SUM, 1: PoolingMode.MEAN, 2: PoolingMode.NONE}[pooling]
    locations = locations or [EmbeddingLocation.DEVICE] * len(rows)
    kw.setdefault("stochastic_rounding", False)
    mod = SplitTableBatchedEmbeddingBagsCodegen(
        [(r, d, loc, ComputeDevice.CUDA) for r, d, loc in zip(rows, dims, locations)],
        feature_table_map=ftm, pooling_mode=pm, device=torch.device("cuda", 0), weights_precision=SparseType.FP16,
        optimizer=optimizer if optimizer is not None else EmbOptimType.EXACT_SGD, **kw)
    tabs = oracle.Tables(rows, dims, ftm)
    rng = rng if rng is not None else np.random.default_rng(0)
    for t, w in enumerate(mod.split_embedding_weights()):
        assert w.dtype == torch.float16
        w16 = rng.standard_normal((rows[t], dims[t])).astype(np.float16)
        tabs.weights[t][...] = w16.astype(np.float32)
        w.copy_(torch.from_numpy(w16))
    return mod, tabs


def weights_f32(mod):
    return [w.float().cpu().numpy() for w in mod.split_embedding_weights()]


def assert_within_half_ulp(w16_as_f32, w32_oracle, what=""):
    """|float(w16_gpu) - w32_oracle| <= 2^-11 |w32| + 2^-25 (half an FP16 ulp, normal and subnormal) + the FP32 backward
    tolerance of tests/test_tbe_gpu.py (2e-5 |w32| + 2e-5)."""
    a = np.abs(w32_oracle.astype(np.float64))
    bound = 2.0 ** -11 * a + 2.0 ** -25 + (2e-5 * a + 2e-5)
    err = np.abs(w16_as_f32.astype(np.float64) - w32_oracle.astype(np.float64))
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"{what} max |err| / bound = {worst:.4f}")
    assert worst <= 1.0, f"{what}: {worst:.4f} of the bound"


# ---- 1. forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_forward_vs_oracle_on_upcast_tables(case):
    rng = np.random.default_rng(11)
    mod, tabs = build_pair16(case["rows"], case["dims"], case["ftm"], case["pooling"], rng=rng)
    indices, offsets, psw = make_inputs(rng, case["rows"], case["B"], case["max_len"], case["ftm"],
                                        case["fixed_len"], case["weighted"])
    out = mod(to_dev(indices), to_dev(offsets), to_dev(psw))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32
    out = out.detach().cpu().numpy()
    ref, bad = oracle.tbe_forward(tabs, indices, offsets, psw, case["pooling"])
    assert bad == 0 and mod.bounds_check_errors() == 0
    long_bags = indices.size / max(1, (offsets.size - 1)) >= 3.5
    if not long_bags:
        np.testing.assert_array_equal(out, ref)  # same accumulation order as the oracle (sequential fmaf)
    else:
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-4)  # different (fixed) association


def test_nobag_forward_is_a_bit_exact_gather():
    rng = np.random.default_rng(6)
    rows, dims, ftm = [30, 17], [64, 64], [0, 1, 0]
    mod, tabs = build_pair16(rows, dims, ftm, 2, rng=rng)
    indices, offsets, _ = make_inputs(rng, rows, 12, 5, ftm)
    out = mod(to_dev(indices), to_dev(offsets))
    ref, _ = oracle.tbe_forward(tabs, indices, offsets, None, oracle.POOL_NONE)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    # odd dim: the element-wise path
    mod, tabs = build_pair16([30, 17], [7, 7], ftm, 2, rng=rng)
    out = mod(to_dev(indices), to_dev(offsets))
    ref, _ = oracle.tbe_forward(tabs, indices, offsets, None, oracle.POOL_NONE)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    grad = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_EXACT_SGD, 0.01, None, oracle.POOL_NONE)
    for t, w in enumerate(weights_f32(mod)):
        assert_within_half_ulp(w, tabs.weights[t], f"nobag table {t}")


# ---- 2. backward, nearest-even ------------------------------------------------------------------------------------------
def _zero_states(tabs, code):
    s0 = s1 = None
    if code == oracle.OPT_EXACT_ROWWISE_ADAGRAD:
        s0 = [np.zeros(r, dtype=np.float32) for r in tabs.rows]
    elif code in (oracle.OPT_ADAM, oracle.OPT_EXACT_ADAGRAD):
        s0 = [np.zeros((r, d), dtype=np.float32) for r, d in zip(tabs.rows, tabs.dims)]
        if code == oracle.OPT_ADAM:
            s1 = [np.zeros((r, d), dtype=np.float32) for r, d in zip(tabs.rows, tabs.dims)]
    return s0, s1


@pytest.mark.parametrize("optname,kw", OPTS, ids=[f"{o[0]}{i}" for i, o in enumerate(OPTS)])
@pytest.mark.parametrize("case", CASES[:7], ids=[str(i) for i in range(7)])
def test_backward_nearest_even_vs_oracle(case, optname, kw):
    """Each of two steps on its own: the oracle starts the step from the GPU's tables (up-cast) and FP32 state, so a
    one-ulp difference of step 1 is not charged to step 2."""
    rng = np.random.default_rng(5)
    code = {"EXACT_SGD": 0, "EXACT_ROWWISE_ADAGRAD": 1, "ADAM": 2, "EXACT_ADAGRAD": 3}[optname]
    lr = 0.05
    mod, tabs = build_pair16(case["rows"], case["dims"], case["ftm"], case["pooling"], _opt(optname), rng,
                             learning_rate=lr, **kw)
    s0, s1 = _zero_states(tabs, code)
    for step in range(2):
        for t, w in enumerate(weights_f32(mod)):
            tabs.weights[t][...] = w
        for t, st in enumerate(mod.split_optimizer_states()):
            assert all(s.dtype == torch.float32 for s in st)
            if s0 is not None:
                s0[t][...] = st[0].cpu().numpy()
            if s1 is not None:
                s1[t][...] = st[1].cpu().numpy()
        indices, offsets, psw = make_inputs(rng, case["rows"], case["B"], case["max_len"], case["ftm"],
                                            case["fixed_len"], case["weighted"])
        out = mod(to_dev(indices), to_dev(offsets), to_dev(psw))
        grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        out.backward(to_dev(grad))
        torch.cuda.synchronize()
        oracle.tbe_backward(tabs, indices, offsets, grad, code, lr, psw, case["pooling"],
                            eps=kw.get("eps", 1e-8), weight_decay=kw.get("weight_decay", 0.0),
                            iteration=step + 1, state0=s0, state1=s1)
        for t, w in enumerate(weights_f32(mod)):
            assert_within_half_ulp(w, tabs.weights[t], f"step {step} table {t}")
        states = mod.split_optimizer_states()
        for t in range(len(tabs.rows)):
            if s0 is not None:
                np.testing.assert_allclose(states[t][0].cpu().numpy(), s0[t], rtol=2e-5, atol=2e-5)
            if s1 is not None:
                np.testing.assert_allclose(states[t][1].cpu().numpy(), s1[t], rtol=2e-5, atol=2e-5)
            if code == 0:
                assert states[t] == ()
    assert mod.bounds_check_errors() == 0


# ---- 3. duplicate-free SGD, nearest-even ----------------------------------------------------------------------------------
def _duplicate_free(rng, rows, B):
    indices = np.concatenate([rng.permutation(r)[:B] for r in rows]).astype(np.int64)
    offsets = np.arange(len(rows) * B + 1, dtype=np.int64)
    return indices, offsets


def test_backward_sgd_duplicate_free_nearest_even_is_bit_exact():
    """With unique ids every row gets one contribution: w16' = float16(fmaf(-lr, g, float(w16))) exactly."""
    rng = np.random.default_rng(2)
    rows, dims, B = [5000, 3000], [128, 128], 512
    mod, tabs = build_pair16(rows, dims, None, 0, rng=rng, learning_rate=0.3)
    indices, offsets = _duplicate_free(rng, rows, B)
    out = mod(to_dev(indices), to_dev(offsets))
    grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_EXACT_SGD, 0.3)  # x = fmaf(-lr, g, w) exactly
    for t, w in enumerate(mod.split_embedding_weights()):
        np.testing.assert_array_equal(w.cpu().numpy(), tabs.weights[t].astype(np.float16))


# ---- 4. stochastic rounding ------------------------------------------------------------------------------------------------
def _neighbours(x):
    """The FP16 values lo <= x <= hi adjacent to float32 x (equal when x is representable)."""
    h = x.astype(np.float16)
    hf = h.astype(np.float32)
    lo = np.where(hf <= x, h, np.nextafter(h, np.float16(-np.inf)))
    hi = np.where(hf >= x, h, np.nextafter(h, np.float16(np.inf)))
    return lo.astype(np.float16), hi.astype(np.float16)


def test_stochastic_rounding_stores_a_neighbour_of_the_exact_result():
    rng = np.random.default_rng(3)
    rows, dims, B = [4000, 600], [128, 20], 512  # a vector-path table and an element-wise one (D % 4 == 0, base unaligned or not)
    torch.manual_seed(7)
    mod, tabs = build_pair16(rows, dims, None, 0, rng=rng, learning_rate=0.3, stochastic_rounding=True)
    indices, offsets = _duplicate_free(rng, rows, B)
    # the rows the first half of table 1's bags address hold tiny values and get tiny gradients: results around and
    # below 2^-14, where halves are subnormal
    ws = mod.split_embedding_weights()
    tiny = torch.from_numpy(indices[B:B + B // 2]).cuda()
    ws[1][tiny] = ws[1][tiny] * 2.0 ** -14
    tabs.weights[1][...] = ws[1].float().cpu().numpy()
    out = mod(to_dev(indices), to_dev(offsets))
    grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    grad[:, :8] = 0.0  # x == w16: representable, must be stored exactly
    grad[: B // 2, 128:] *= 2.0 ** -14
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, indices, offsets, grad, oracle.OPT_EXACT_SGD, 0.3)
    n_inexact = n_up = 0
    for t, w in enumerate(mod.split_embedding_weights()):
        got = w.cpu().numpy()
        x = tabs.weights[t]
        lo, hi = _neighbours(x)
        assert np.all((got == lo) | (got == hi)), f"table {t}: a stored value is not a neighbour of the FP32 result"
        exact = lo == hi
        np.testing.assert_array_equal(got[exact].astype(np.float32), x[exact])
        n_inexact += int((~exact).sum())
        n_up += int(((got == hi) & ~exact).sum())
    assert n_inexact > 50000 and 0.4 < n_up / n_inexact < 0.6, (n_inexact, n_up)  # both neighbours occur


def _quarter_step(mod, rows, iteration=None):
    """All weights 1.0, lr 0.5, every gradient -2^-11: x = 1 + 2^-12, a quarter of the way from 1 to 1 + 2^-10."""
    w = mod.split_embedding_weights()[0]
    w.fill_(1.0)
    assert float(np.float32(1.0) + np.float32(0.5) * np.float32(2.0 ** -11)) == 1.0 + 2.0 ** -12
    idx = torch.randperm(rows, generator=torch.Generator().manual_seed(1)).cuda()
    off = torch.arange(rows + 1, dtype=torch.int64, device="cuda")
    out = mod(idx, off)
    out.backward(torch.full_like(out, -(2.0 ** -11)))
    torch.cuda.synchronize()
    got = mod.split_embedding_weights()[0].cpu().numpy()
    up = got == np.float16(1.0 + 2.0 ** -10)
    assert np.all(up | (got == np.float16(1.0)))
    return got, up


def test_stochastic_rounding_probability_determinism_and_iteration():
    rows, D = 4096, 128
    n = rows * D
    sigma = math.sqrt(0.25 * 0.75 / n)
    assert abs(6 * sigma - 0.0036) < 1e-4

    def make(seed):
        torch.manual_seed(seed)
        mod, _ = build_pair16([rows], [D], None, 0, learning_rate=0.5, stochastic_rounding=True)
        return mod

    mod = make(123)
    got1, up1 = _quarter_step(mod, rows)
    share = up1.mean()
    print(f"share rounded up: {share:.5f} (iteration 1)")
    assert abs(share - 0.25) <= 0.0036 + 2.0 ** -13
    # (d) the second iteration draws other bits: agreement with the first is p^2 + (1 - p)^2 = 0.625
    got2, up2 = _quarter_step(mod, rows)
    agree = (up1 == up2).mean()
    print(f"share rounded up: {up2.mean():.5f} (iteration 2), agreement {agree:.5f}")
    assert abs(up2.mean() - 0.25) <= 0.0036 + 2.0 ** -13
    assert abs(agree - 0.625) <= 6 * math.sqrt(0.625 * 0.375 / n)
    # (c) the same seed gives the same table, another seed another one
    got1b, _ = _quarter_step(make(123), rows)
    np.testing.assert_array_equal(got1, got1b)
    got1c, up1c = _quarter_step(make(124), rows)
    assert abs((up1 == up1c).mean() - 0.625) <= 6 * math.sqrt(0.625 * 0.375 / n)


@pytest.mark.parametrize("optname", ["EXACT_SGD", "EXACT_ROWWISE_ADAGRAD"])
def test_stochastic_rounding_is_independent_of_the_path_that_finishes_a_row(optname):
    """A 3-row table hit by every bag: its rows are finished by the fix-up kernel, the big table's by the update kernel.
    Same seed and iteration: the fused call and prepare + apply (the side-stream sort, TBE_OVERLAP_SORT) store the same
    bits; so do two batch sizes' worth of chunking for the rows they share (checked through determinism of each)."""
    rows, dims, B = [3, 100000], [128, 128], 4096
    results = []
    for overlap in ("0", "1", "0"):
        rng = np.random.default_rng(9)
        torch.manual_seed(99)
        mod, _ = build_pair16(rows, dims, None, 0, _opt(optname), rng, learning_rate=0.01, eps=1e-3, stochastic_rounding=True)
        mod.overlap_backward_sort = overlap
        indices, offsets, _ = make_inputs(rng, rows, B, 1, fixed_len=1)
        out = mod(to_dev(indices), to_dev(offsets))
        grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        out.backward(to_dev(grad))
        torch.cuda.synchronize()
        results.append([w.cpu().numpy().copy() for w in mod.split_embedding_weights()])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            np.testing.assert_array_equal(a, b)


# ---- 5. plumbing shared with FP32 --------------------------------------------------------------------------------------------
def test_a2a_ready_layout_with_row_windows_matches_standard_layout():
    rng = np.random.default_rng(12)
    rows, dims = [300, 5, 77], [128, 64, 32]
    W, Bl = 4, 50
    ftm = [0, 1, 2] * W
    mod_a, _ = build_pair16(rows, dims, ftm, 0, rng=np.random.default_rng(1), learning_rate=0.1)
    mod_b, _ = build_pair16(rows, dims, ftm, 0, rng=np.random.default_rng(1), learning_rate=0.1)
    mod_b.set_a2a_output_layout(W)
    for m in (mod_a, mod_b):  # table 0 is a shard holding global rows [100, 400) of a 1000-row table
        m.set_row_windows([100, 0, 0] * W, [1000, 5, 77] * W)
    indices, offsets, psw = make_inputs(rng, [1000, 5, 77], Bl, 3, ftm, weighted=True)
    oa = mod_a(to_dev(indices), to_dev(offsets), to_dev(psw))          # [Bl, W*Dl]
    ob = mod_b(to_dev(indices), to_dev(offsets), to_dev(psw))          # [W*Bl, Dl]
    Dl = sum(dims)
    assert ob.shape == (W * Bl, Dl) and float(oa.detach().abs().sum()) > 0
    assert torch.equal(ob, oa.view(Bl, W, Dl).permute(1, 0, 2).reshape(W * Bl, Dl))
    g = torch.from_numpy(rng.standard_normal((Bl, W * Dl)).astype(np.float32)).cuda()
    oa.backward(g)
    ob.backward(g.view(Bl, W, Dl).permute(1, 0, 2).reshape(W * Bl, Dl).contiguous())
    torch.cuda.synchronize()
    for wa, wb in zip(mod_a.split_embedding_weights(), mod_b.split_embedding_weights()):
        assert torch.equal(wa, wb)
    assert mod_a.bounds_check_errors() == 0 and mod_b.bounds_check_errors() == 0  # rows of other shards are no errors


def test_sum_and_mean_tables_in_one_module():
    from _util import oracle_backward_mixed
    from fbgemm_gpu.split_table_batched_embeddings_ops import PoolingMode

    rng = np.random.default_rng(21)
    rows, dims, ftm = [60, 9, 200, 31], [32, 64, 16, 128], [0, 1, 2, 2, 3]
    feat_mean = [False, True, True, True, False]
    mod, tabs = build_pair16(rows, dims, ftm, 0, rng=rng, learning_rate=0.1)
    mod.set_feature_pooling([PoolingMode.MEAN if m else PoolingMode.SUM for m in feat_mean])
    indices, offsets, psw = make_inputs(rng, rows, 19, 6, ftm, None, True)
    out = mod(to_dev(indices), to_dev(offsets), to_dev(psw))
    ref = oracle_forward_mixed(tabs, indices, offsets, psw, feat_mean)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    grad = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(to_dev(grad))
    torch.cuda.synchronize()
    oracle_backward_mixed(tabs, indices, offsets, grad, oracle.OPT_EXACT_SGD, 0.1, psw, feat_mean)
    for t, w in enumerate(weights_f32(mod)):
        assert_within_half_ulp(w, tabs.weights[t], f"table {t}")


@pytest.mark.parametrize("optname", ["EXACT_SGD", "EXACT_ROWWISE_ADAGRAD"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=["0", "3", "5"])
def test_lookup_without_autograd_is_the_autograd_path(case, optname):
    def run(explicit):
        rng = np.random.default_rng(11)
        mod, _ = build_pair16(case["rows"], case["dims"], case["ftm"], case["pooling"], _opt(optname), rng, learning_rate=0.05)
        outs = []
        for _ in range(2):
            indices, offsets, psw = make_inputs(rng, case["rows"], case["B"], case["max_len"], case["ftm"],
                                                case["fixed_len"], case["weighted"])
            i, o, w = to_dev(indices), to_dev(offsets), to_dev(psw)
            if explicit:
                out, rec = mod.lookup_no_autograd(i, o, w)
            else:
                out = mod(i, o, w)
            grad = to_dev(rng.standard_normal(tuple(out.shape)).astype(np.float32))
            outs.append(out.detach().clone())
            if explicit:
                mod.backward_no_autograd(rec, grad)
            else:
                out.backward(grad)
        torch.cuda.synchronize()
        state = [tuple(s.clone() for s in st) for st in mod.split_optimizer_states()]
        return outs, [w.clone() for w in mod.split_embedding_weights()], state

    a, b = run(False), run(True)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x, y)
    for sa, sb in zip(a[2], b[2]):
        for x, y in zip(sa, sb):
            assert torch.equal(x, y)


def test_out_of_range_indices_are_counted_and_contribute_zero():
    rng = np.random.default_rng(8)
    rows, dims = [10, 20], [32, 32]
    mod, tabs = build_pair16(rows, dims, None, 0, rng=rng)
    B = 8
    indices = rng.integers(0, 10, size=2 * B).astype(np.int64)
    indices[3] = 10      # == rows -> invalid
    indices[B + 1] = -1  # negative -> invalid
    offsets = np.arange(2 * B + 1, dtype=np.int64)
    out = mod(to_dev(indices), to_dev(offsets))
    ref, bad = oracle.tbe_forward(tabs, indices, offsets)
    assert bad == 2
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, indices, offsets, np.ones(tuple(out.shape), np.float32), 0, 0.01)
    for t, w in enumerate(weights_f32(mod)):
        assert_within_half_ulp(w, tabs.weights[t], f"table {t}")
    assert mod.bounds_check_errors() == 4  # 2 in forward + 2 in backward


def test_managed_tables_match_device_tables_bit_for_bit():
    from fbgemm_gpu.split_table_batched_embeddings_ops import EmbeddingLocation

    rows, dims = [300, 41, 7], [128, 128, 128]
    results = []
    for locs in ([EmbeddingLocation.DEVICE] * 3, [EmbeddingLocation.MANAGED, EmbeddingLocation.DEVICE, EmbeddingLocation.MANAGED]):
        rng = np.random.default_rng(21)
        torch.manual_seed(5)
        mod, _ = build_pair16(rows, dims, None, 0, _opt("EXACT_ROWWISE_ADAGRAD"), rng, locations=locs, learning_rate=0.1, eps=1e-3,
                              stochastic_rounding=True)
        ws = mod.split_embedding_weights()
        assert ws[1].is_cuda and ws[0].is_cuda == (locs[0] == EmbeddingLocation.DEVICE) and ws[0].dtype == torch.float16
        indices, offsets, _ = make_inputs(rng, rows, 64, 3)
        out = mod(to_dev(indices), to_dev(offsets))
        grad = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        out.backward(to_dev(grad))
        torch.cuda.synchronize()
        results.append((out.detach().cpu(), [w.cpu().clone() for w in mod.split_embedding_weights()],
                        [s[0].cpu().clone() for s in mod.split_optimizer_states()]))
    assert torch.equal(results[0][0], results[1][0])
    for a, b in zip(results[0][1] + results[0][2], results[1][1] + results[1][2]):
        assert torch.equal(a, b)


# ---- 6. sharded, world 1 -----------------------------------------------------------------------------------------------------
def test_sharded_ebc_world1_fp16_tables_forward_step_and_checkpoint():
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, Topology
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.modules.embedding_configs import DataType, EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    rng = np.random.default_rng(33)
    rows, D, B, lr = [5000, 700], 128, 300, 0.1
    keys = ["c0", "c1"]
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=D, num_embeddings=rows[i], feature_names=[keys[i]],
                                 data_type=DataType.FP16) for i in range(2)]
    # (row-wise features come first in a rank's local feature order: t0, so that the output columns are in table order)
    plan = EmbeddingShardingPlanner(Topology(1), constraints={"t0": ["row_wise"], "t1": ["table_wise"]}).plan_tables(tables)
    assert plan["t0"].sharding_type == "row_wise" and plan["t1"].sharding_type == "table_wise"
    dev = torch.device("cuda", 0)

    def make():
        return ShardedEmbeddingBagCollection(EmbeddingBagCollection(tables, device=torch.device("meta")), plan,
                                             ShardingEnv.from_local(1, 0), {"learning_rate": lr, "stochastic_rounding": False}, dev)

    sebc = make()
    assert sebc._emb_module.weights_dev.dtype == torch.float16
    tabs = oracle.Tables(rows, [D] * 2)
    for name, (w, _) in sebc.local_shards().items():
        assert w.dtype == torch.float16 and float(w.float().abs().sum()) > 0  # initialised in half
        t = int(name[1:])
        w16 = rng.standard_normal((rows[t], D)).astype(np.float16)
        tabs.weights[t][...] = w16.astype(np.float32)
        w.copy_(torch.from_numpy(w16))
    values = np.concatenate([rng.integers(0, r, size=B) for r in rows]).astype(np.int64)
    kjt = KeyedJaggedTensor.from_fixed_lengths(keys, torch.from_numpy(values).to(dev), [1] * 2)
    out = sebc(kjt).wait().values()
    offsets = np.arange(2 * B + 1, dtype=np.int64)
    ref, _ = oracle.tbe_forward(tabs, values, offsets)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    grad = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(torch.from_numpy(grad).to(dev))
    torch.cuda.synchronize()
    oracle.tbe_backward(tabs, values, offsets, grad, oracle.OPT_EXACT_SGD, lr)
    for name, (w, _) in sebc.local_shards().items():
        assert_within_half_ulp(w.float().cpu().numpy(), tabs.weights[int(name[1:])], name)
    sd = sebc.state_dict()
    assert sorted(sd) == ["embedding_bags.t0.weight", "embedding_bags.t1.weight"]
    assert all(v.dtype == torch.float16 for v in sd.values())
    saved = {k: v.detach().clone() for k, v in sd.items()}
    fresh = make()
    holder = torch.nn.Module()
    holder.add_module("m", fresh)
    res = holder.load_state_dict({f"m.{k}": v for k, v in saved.items()})
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in fresh.state_dict().items():
        assert v.dtype == torch.float16 and torch.equal(v, saved[k])
    # an FP32 checkpoint tensor is cast on load
    res = holder.load_state_dict({f"m.{k}": v.float() for k, v in saved.items()})
    for k, v in fresh.state_dict().items():
        assert v.dtype == torch.float16 and torch.equal(v, saved[k])


# ---- 7. DLRM end to end -----------------------------------------------------------------------------------------------------
def _small_dlrm(data_type):
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from torchrec_amd.distributed.embeddingbag import ShardedEmbeddingBagCollection
    from torchrec_amd.distributed.planner import EmbeddingShardingPlanner, Topology
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.dlrm import DLRM
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection

    dev = torch.device("cuda", 0)
    rows, D = [3000, 50, 700], 64
    keys = [f"f{i}" for i in range(3)]
    tables = [EmbeddingBagConfig(name=f"t{i}", embedding_dim=D, num_embeddings=rows[i], feature_names=[keys[i]],
                                 data_type=data_type) for i in range(3)]
    plan = EmbeddingShardingPlanner(Topology(1)).plan_tables(tables)
    torch.manual_seed(4)
    sebc = ShardedEmbeddingBagCollection(EmbeddingBagCollection(tables, device=torch.device("meta")), plan,
                                         ShardingEnv.from_local(1, 0), {"learning_rate": 0.1, "optimizer": EmbOptimType.EXACT_SGD}, dev)
    sebc.reset_parameters_sharding_invariant(9)
    model = DLRM(sebc, 13, [32, D], [16, 1], dense_device=dev)
    model.fused_lookup = True
    return model, sebc, keys, rows


def test_dlrm_trains_with_fp16_tables_on_the_two_kernel_path():
    from torchrec_amd.modules.embedding_configs import DataType
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    B, steps = 96, 3
    for data_type in (DataType.FP16, DataType.FP32):
        model, sebc, keys, rows = _small_dlrm(data_type)
        half = data_type == DataType.FP16
        assert (sebc._emb_module.gather_layout() is None) == half
        assert sebc._emb_module.weights_dev.dtype == (torch.float16 if half else torch.float32)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        before = {k: w.clone() for k, (w, _) in sebc.local_shards().items()}
        g = torch.Generator().manual_seed(0)
        for _ in range(steps):
            vals = torch.cat([torch.randint(0, r, (B,), generator=g) for r in rows]).to(torch.int64).cuda()
            dense = torch.randn(B, 13, generator=g).cuda()
            labels = torch.randint(0, 2, (B,), generator=g).float().cuda()
            logits = model(dense, KeyedJaggedTensor.from_fixed_lengths(keys, vals, [1] * 3))
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), labels)
            assert math.isfinite(float(loss.detach()))
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        # the path taken, not a timing: FP16 tables are served by lookup + interaction, FP32 ones by the gather kernels
        assert model.fused_lookup_steps == (0 if half else steps)
        after = {k: w for k, (w, _) in sebc.local_shards().items()}
        assert all(w.dtype == (torch.float16 if half else torch.float32) for w in after.values())
        assert any(not torch.equal(after[k], before[k]) for k in after)  # the tables were trained
        assert all(bool(torch.isfinite(w.float()).all()) for w in after.values())
        assert sebc._emb_module.bounds_check_errors() == 0
