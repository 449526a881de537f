"""Shared by the variable-batch tests (CPU over gloo with the oracle lookup, GPU with the real kernels): the recorded
vectors of tests/golden/vb_dist_data.npz, per-rank batches of DIFFERENT sizes for a sharded collection, and the unsharded
oracle run on the concatenated batch that it must equal (the check of tests/_cw_sharded.py / tests/test_multirank_gpu.py
`_check_against_oracle` with one batch size per rank)."""
import json
import os

import numpy as np
import torch

import _paths  # noqa: F401

from _cw_sharded import LR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vb_dist_data.npz")


def golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def golden_kjt(z, case, rank, tag, device="cpu"):
    """(lengths, values, weights | None) of rank `rank`'s input (`tag` "in") or expected output ("out") as tensors."""
    pre = f"kjt/{case['name']}/r{rank}/{tag}_"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return t(z[pre + "lengths"]), t(z[pre + "values"]), (t(z[pre + "weights"]) if case["weighted"] else None)


def run_golden_exchanges(z, meta, W, rank, pg, device):
    """Every recorded W-rank case through KJTAllToAll(variable_batch_size=True) and PooledEmbeddingsAllToAll with
    batch_size_per_rank (forward and backward) on `device`; returns what the rank got, as numpy."""
    from torchrec_amd.distributed.dist_data import KJTAllToAll, PooledEmbeddingsAllToAll
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    got = {}
    for case in meta["kjt"]:
        if len(case["splits"]) != W:
            continue
        lengths, values, weights = golden_kjt(z, case, rank, "in", device)
        kjt = KeyedJaggedTensor.from_lengths_sync(case["keys"], values, lengths, weights=weights)
        assert kjt.stride() == case["batch_size_per_rank"][rank]
        out = KJTAllToAll(pg, case["splits"], device, variable_batch_size=True)(kjt).wait().wait()
        got["kjt/" + case["name"]] = (out.keys(), out.stride(), out.lengths().cpu().numpy(), out.values().cpu().numpy(),
                                      out.weights().cpu().numpy() if case["weighted"] else None)
    for case in meta["pooled"]:
        if len(case["splits"]) != W:
            continue
        pre = f"pooled/{case['name']}/r{rank}/"
        x = torch.from_numpy(z[pre + "in"]).to(device).requires_grad_(True)
        a2a = PooledEmbeddingsAllToAll(pg, case["dim_sum_per_rank"], device)
        res = a2a(x, case["batch_size_per_rank"]).wait()
        res.backward(torch.from_numpy(z[pre + "grad_out"]).to(device))
        got["pooled/" + case["name"]] = (res.detach().cpu().numpy(), x.grad.cpu().numpy())
    return got


def check_golden_exchanges(z, meta, W, ret):
    """Integers and forward floats match exactly: the exchange only copies.  The gradient is scaled by 1 / W: exact at W = 2."""
    n = 0
    for case in meta["kjt"]:
        if len(case["splits"]) != W:
            continue
        for r in range(W):
            keys, stride, lengths, values, weights = ret[r]["kjt/" + case["name"]]
            pre = f"kjt/{case['name']}/r{r}/out_"
            assert keys == case["out_keys"][r] and stride == sum(case["batch_size_per_rank"])
            np.testing.assert_array_equal(lengths, z[pre + "lengths"])
            np.testing.assert_array_equal(values, z[pre + "values"])
            if case["weighted"]:
                np.testing.assert_array_equal(weights, z[pre + "weights"])
            n += 1
    for case in meta["pooled"]:
        if len(case["splits"]) != W:
            continue
        for r in range(W):
            out, grad_in = ret[r]["pooled/" + case["name"]]
            pre = f"pooled/{case['name']}/r{r}/"
            assert out.shape == z[pre + "out"].shape and grad_in.shape == z[pre + "in"].shape
            np.testing.assert_array_equal(out, z[pre + "out"])
            # the kernels scale by the float 1 / W, the recorded gradient is x / W: the same number when W is a power of
            # two; otherwise fl(1 / W), the product and the quotient each round once (2^-24 relative each)
            np.testing.assert_allclose(grad_in, z[pre + "grad_in"], rtol=3 * 2.0 ** -24 if W & (W - 1) else 0, atol=0)
            n += 1
    assert n > 0
    return n


def data(bpr, rows, dims, fixed_len, weighted, seed=11, max_len=3):
    """per rank (lengths [F * B_r], ids, weights | None, output gradient [B_r, sum D]) + the initial tables."""
    rng = np.random.default_rng(seed)
    F = len(rows)
    per_rank = []
    for B in bpr:
        lengths = (np.full(F * B, fixed_len) if fixed_len else rng.integers(0, max_len + 1, size=F * B)).astype(np.int32)
        vals = np.concatenate([rng.integers(0, rows[f], size=int(lengths[f * B:(f + 1) * B].sum()))
                               for f in range(F)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        wts = (rng.random(vals.size).astype(np.float32) + 0.5) if weighted else None
        grad = rng.standard_normal((B, sum(dims))).astype(np.float32)
        per_rank.append((lengths, vals, wts, grad))
    init = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    return per_rank, init


def global_batch(per_rank, bpr, F, weighted):
    """The ranks' batches as ONE batch of sum(B_r): rank-major concatenation per feature; gradients / W."""
    W = len(bpr)
    g_len = np.concatenate([np.concatenate([per_rank[r][0][f * bpr[r]:(f + 1) * bpr[r]] for r in range(W)]) for f in range(F)])
    pos = [np.concatenate([[0], np.cumsum(per_rank[r][0])]) for r in range(W)]
    cat = lambda i: np.concatenate([np.concatenate([per_rank[r][i][pos[r][f * bpr[r]]:pos[r][(f + 1) * bpr[r]]]  # noqa: E731
                                                    for r in range(W)]) for f in range(F)])
    g_vals, g_w = cat(1), (cat(2) if weighted else None)
    g_grad = np.ascontiguousarray(np.concatenate([per_rank[r][3] for r in range(W)], axis=0) / W, dtype=np.float32)
    g_offs = np.concatenate([[0], np.cumsum(g_len)]).astype(np.int64)
    return g_vals, g_offs, g_w, g_grad


def check_against_unsharded(ret, bpr, rows, dims, per_rank, init, fixed_len, weighted, kinds, mean_tables=(), adagrad_eps=None,
                            bit_exact=None):
    """ret[r] = (output, pieces, replicas[, states]).  Every rank's forward against the unsharded oracle on ITS batch;
    the tables after one step against the oracle on the concatenated batch with gradients / W.  The oracle's backward
    runs on the split model — one table [rows, w] per piece, the feature duplicated — which for SGD is the unsharded
    table and for row-wise Adagrad is fbgemm's per-column-shard state; replicated tables are dense parameters stepped by
    plain SGD.  outputs rtol = atol = 1e-5 (bit-exact for fixed length 1, unweighted, SUM); tables and state 3e-5."""
    from _util import oracle_backward_mixed, oracle_forward_mixed
    from oracle import oracle

    W, F, Bg = len(bpr), len(rows), sum(bpr)
    feat_mean = [i in mean_tables for i in range(F)]
    tabs = oracle.Tables(rows, dims)
    for t in range(F):
        tabs.weights[t][...] = init[t]
    if bit_exact is None:
        bit_exact = fixed_len == 1 and not weighted and not mean_tables
    for r in range(W):
        lengths, vals, wts, _ = per_rank[r]
        assert ret[r][0].shape == (bpr[r], sum(dims))
        if bpr[r] == 0:
            continue
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ref = oracle_forward_mixed(tabs, vals, offs, wts, feat_mean)
        if bit_exact:
            np.testing.assert_array_equal(ret[r][0], ref)  # pure gather: bit-exact through the whole exchange
        else:
            np.testing.assert_allclose(ret[r][0], ref, rtol=1e-5, atol=1e-5)
    g_vals, g_offs, g_w, g_grad = global_batch(per_rank, bpr, F, weighted)
    held = sorted({(int(n[1:]), c0, w.shape[1]) for r in range(W) for n, w, _, c0 in ret[r][1]}
                  | {(int(n[1:]), 0, dims[int(n[1:])]) for n in ret[0][2]})
    assert [sum(w for t, _, w in held if t == tt) for tt in range(F)] == list(dims), "the pieces tile every table's columns"
    split = oracle.Tables([rows[t] for t, _, _ in held], [w for _, _, w in held])
    for i, (t, c0, w) in enumerate(held):
        split.weights[i][...] = init[t][:, c0:c0 + w]
    seg = lambda a: np.concatenate([a[g_offs[t * Bg]:g_offs[(t + 1) * Bg]] for t, _, _ in held])  # noqa: E731
    ids, psw = seg(g_vals), (seg(g_w) if weighted else None)
    lens = np.concatenate([np.diff(g_offs[t * Bg:(t + 1) * Bg + 1]) for t, _, _ in held])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    piece_mean = [t in mean_tables for t, _, _ in held]
    index = {(t, c0): i for i, (t, c0, _) in enumerate(held)}
    s0 = None
    if adagrad_eps is None:
        oracle_backward_mixed(split, ids, offs, g_grad, oracle.OPT_EXACT_SGD, LR, psw, piece_mean)
        sgd = split
    else:
        assert not mean_tables
        sgd = oracle.Tables(split.rows, split.dims)
        for i in range(len(held)):
            sgd.weights[i][...] = split.weights[i]
        s0 = [np.zeros(rows[t], dtype=np.float32) for t, _, _ in held]
        oracle.tbe_backward(sgd, ids, offs, g_grad, oracle.OPT_EXACT_SGD, LR, psw)
        oracle.tbe_backward(split, ids, offs, g_grad, oracle.OPT_EXACT_ROWWISE_ADAGRAD, LR, psw, eps=adagrad_eps, state0=s0)
    seen = {t: np.zeros((rows[t], dims[t]), dtype=np.int32) for t in range(F)}
    for r in range(W):
        for name, w, row0, c0 in ret[r][1]:
            t = int(name[1:])
            np.testing.assert_allclose(w, split.weights[index[(t, c0)]][row0:row0 + w.shape[0]], rtol=3e-5, atol=3e-5)
            seen[t][row0:row0 + w.shape[0], c0:c0 + w.shape[1]] += 1
        for name, w in ret[r][2].items():
            np.testing.assert_allclose(w, sgd.weights[index[(int(name[1:]), 0)]], rtol=3e-5, atol=3e-5)
        if adagrad_eps is not None:
            assert len(ret[r][3]) == len(ret[r][1])
            for name, c0, m1 in ret[r][3]:
                np.testing.assert_allclose(m1, s0[index[(int(name[1:]), c0)]], rtol=3e-5, atol=3e-5)
    for t in range(F):
        if kinds[f"t{t}"] == "data_parallel":
            assert all(f"t{t}" in ret[r][2] for r in range(W)) and not seen[t].any()
        else:
            assert (seen[t] == 1).all(), f"t{t}: every element of a sharded table lives in exactly one piece"
