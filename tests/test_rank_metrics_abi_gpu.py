"""GPU: csrc/rank_metrics.hip straight through the C ABI (include/tbe_hip.h), the outputs and the workspace between guard
elements that must stay untouched, the inputs checked to come back unmodified.  Per-row values are compared with the float64
restatement (tests/_rank_metrics_ref.py) at 8 x the reference's measured float32 error, hit counts exactly; every case runs
twice, bit for bit the same."""
import ctypes

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _rank_metrics_ref as rr
from _guarded import Buf
from fbgemm_gpu import _lib
from torchrec_amd.metrics import ranking

pytestmark = pytest.mark.gpu

OK, INVALID, WORKSPACE = 0, -1, -3
COUNT_COLS = 10  # row_counts [B, 10]: bad candidates, bad labels, hits of k_0 .. k_7


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw_buf(a):
    """Any array's bytes in a guarded float32 buffer (padded to whole elements)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    raw = np.concatenate([raw, np.zeros(-len(raw) % 4, dtype=np.uint8)])
    return Buf(len(raw) // 4, raw.view(np.float32))


def _run(lib, scores, labels, ks, candidates=None, stride=None):
    """One call through the ABI.  scores rows sit `stride` elements apart, NaN between them."""
    B, C = labels.shape
    width = scores.shape[1]
    stride = width if stride is None else stride
    sin = np.full(max(B, 1) * stride, np.nan, dtype=np.float32)
    for b in range(B):
        sin[b * stride:b * stride + width] = scores[b]
    nk = len(ks)
    bs, bl = Buf(len(sin), sin), _raw_buf(labels)
    bc = None if candidates is None else _raw_buf(np.asarray(candidates, dtype=np.int64))
    w = ranking.dcg_weights(ks[-1]).numpy()
    bw, bm, bcnt = Buf(len(w), w), Buf(2 * nk), _raw_buf(np.full(2, -7, dtype=np.int64))
    wbytes = lib.tbe_rank_metrics_workspace_bytes(B, nk)
    assert wbytes > 0 and wbytes % 256 == 0
    bws = Buf(wbytes // 4)
    rc = lib.tbe_rank_metrics_f32(bs.ptr, stride, None if bc is None else bc.ptr, width, bl.ptr, labels.dtype.itemsize, B, C,
                                  (ctypes.c_int32 * nk)(*ks), nk, bw.ptr, bm.ptr, bcnt.ptr, bws.ptr, wbytes, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bs.get().view(np.uint32), sin.view(np.uint32))  # inputs are not modified
    np.testing.assert_array_equal(bl.get().view(np.uint8)[:labels.nbytes], np.ascontiguousarray(labels).view(np.uint8).reshape(-1))
    if bc is not None:
        np.testing.assert_array_equal(bc.get().view(np.int64), np.asarray(candidates, dtype=np.int64).reshape(-1))
    np.testing.assert_array_equal(bw.get(), w)
    ws = bws.get()
    off = -(-(B * 2 * nk * 4) // 256) * 256 // 4 if B else 256 // 4
    return {"metrics": bm.get(), "counts": bcnt.get().view(np.int64).copy(),
            "row_values": ws[:B * 2 * nk].reshape(B, 2 * nk).copy(),
            "row_counts": ws[off:off + B * COUNT_COLS].view(np.int32).reshape(B, COUNT_COLS).copy()}


def _same_bits(a, b, nk):
    np.testing.assert_array_equal(a["metrics"].view(np.uint32), b["metrics"].view(np.uint32))
    np.testing.assert_array_equal(a["row_values"].view(np.uint32), b["row_values"].view(np.uint32))
    np.testing.assert_array_equal(a["row_counts"][:, :2 + nk], b["row_counts"][:, :2 + nk])
    np.testing.assert_array_equal(a["counts"], b["counts"])


def _check(lib, label, scores, labels, ks, candidates=None, stride=None):
    got = _run(lib, scores, labels, ks, candidates, stride)
    vals, hits = rr.per_row(scores, labels, ks, candidates)
    tol = rr.tolerance()
    nk = len(ks)
    assert (np.isnan(got["row_values"]) == np.isnan(vals)).all()
    fin = np.isfinite(vals)
    err = float(np.abs(got["row_values"][fin] - vals[fin]).max()) if fin.any() else 0.0
    np.testing.assert_array_equal(got["row_counts"][:, 2:2 + nk], hits)      # exact
    assert not got["row_counts"][:, :2].any() and not got["counts"].any()
    want = vals.mean(0)
    assert (np.isnan(got["metrics"]) == np.isnan(want)).all()
    fin = np.isfinite(want)
    merr = float(np.abs(got["metrics"][fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"{label}: tolerance {tol:.3e}, per-row error {err:.2e}, mean error {merr:.2e}")
    assert err <= tol and merr <= tol
    _same_bits(got, _run(lib, scores, labels, ks, candidates, stride), nk)
    return got


def _labels(rng, B, C, kind):
    y = np.zeros((B, C), dtype=np.int64)
    if kind == "one":
        y[np.arange(B), rng.integers(0, C, size=B)] = 1
    elif kind == "all":
        y[:] = 1
    elif kind == "last":
        y[:, -1] = 1
    else:  # ~30 % and at least one
        y = (rng.random((B, C)) < 0.3).astype(np.int64)
        y[np.arange(B), rng.integers(0, C, size=B)] = 1
    return y


@pytest.mark.parametrize("kind", ["one", "all", "last", "some"])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 63), (3, 64), (3, 65), (17, 101), (3, 256), (257, 257), (1, 101)])
def test_kernel_matches_the_float64_restatement_and_repeats_bit_for_bit(B, C, kind):
    """C: 1, both sides of a wave (63 | 64 | 65), 101, both sides of a workgroup's trip (256 | 257).  B: 1, 3, 17 (one past
    the finishing launch's 16 row lanes), 257 (one past its 256 threads)."""
    rng = np.random.default_rng([B, C, len(kind)])
    scores = rng.standard_normal((B, C)).astype(np.float32)
    _check(_lib.load(), f"rank_metrics {B}x{C} {kind}", scores, _labels(rng, B, C, kind), rr.ks_for(C))


@pytest.mark.parametrize("kind", ["one", "some"])
def test_the_widest_list(kind):
    """C = 8192, the limit, at B = 2, with k up to C."""
    rng = np.random.default_rng(8192)
    scores = rng.standard_normal((2, 8192)).astype(np.float32)
    _check(_lib.load(), f"rank_metrics 2x8192 {kind}", scores, _labels(rng, 2, 8192, kind), [1, 10, 4096, 8192])


def test_k_boundaries_ties_nan_and_signed_zero():
    lib = _lib.load()
    for C, k in ((12, 1), (12, 5), (12, 12), (300, 64), (300, 65)):
        s, y = rr.k_boundary_rows(C, k)
        got = _check(lib, f"k boundary C={C} k={k}", s, y, [k])
        assert got["row_counts"][0, 2] == 1 and got["row_counts"][1, 2] == (1 if k == C else 0)
    s, y = rr.edge_rows()
    ks = [1, 2, 3, 5, 8]
    got = _check(lib, "edge rows", s, y, ks)
    np.testing.assert_array_equal(got["row_counts"][:, 2:7], [[sum(p < k for p in row) for k in ks] for row in rr.EDGE_POSITIONS])
    y0 = y.copy()
    y0[2] = 0  # a row without a positive: NaN in its row and in the mean
    got = _check(lib, "edge rows, one without a positive", s, y0, ks)
    assert np.isnan(got["row_values"][2]).all() and np.isnan(got["metrics"]).all()
    for dtype in (np.float32, np.bool_):
        other = _run(lib, s, y.astype(dtype), ks)
        _same_bits(_run(lib, s, y, ks), other, len(ks))


def test_candidates_with_repeats_and_strided_scores():
    lib = _lib.load()
    rng = np.random.default_rng(11)
    B, C, V = 9, 101, 500
    scores = rng.standard_normal((B, V)).astype(np.float32)
    cand = rng.integers(0, V, size=(B, C)).astype(np.int64)
    cand[:, 50] = cand[:, 3]          # a repeated item: a tie, to the lower index
    cand[0, :] = cand[0, 0]           # one row of one item only
    y = _labels(rng, B, C, "some")
    a = _check(lib, "candidates", scores, y, rr.ks_for(C), candidates=cand)
    b = _check(lib, "candidates, row stride 3 V", scores, y, rr.ks_for(C), candidates=cand, stride=3 * V)  # scores[:, -1, :]
    _same_bits(a, b, 4)
    gathered = np.take_along_axis(scores, cand, axis=1)
    _same_bits(a, _run(lib, gathered, y, rr.ks_for(C)), 4)


def test_bad_candidates_and_labels_are_counted_and_never_used():
    lib = _lib.load()
    rng = np.random.default_rng(12)
    B, C, V = 5, 65, 90
    scores = rng.standard_normal((B, V)).astype(np.float32)
    cand = np.stack([rng.permutation(V)[:C] for _ in range(B)]).astype(np.int64)
    y = _labels(rng, B, C, "some")
    bad_c = cand.copy()
    bad_c[0, 1], bad_c[0, 2], bad_c[3, 64], bad_c[4, 0] = V, -1, 1 << 40, -(1 << 62)
    got = _run(lib, scores, y, [1, 10], candidates=bad_c)
    np.testing.assert_array_equal(got["counts"], [4, 0])
    np.testing.assert_array_equal(got["row_counts"][:, 0], [2, 0, 0, 1, 1])
    # such an entry ranks as a NaN score does
    as_nan = np.take_along_axis(scores, np.clip(bad_c, 0, V - 1), axis=1)
    as_nan[(bad_c < 0) | (bad_c >= V)] = np.nan
    np.testing.assert_array_equal(got["row_counts"][:, 2:4], rr.per_row(as_nan, y, [1, 10])[1])
    bad_y = y.copy()
    bad_y[1, 0], bad_y[1, 7], bad_y[2, 64] = 2, -1, 1 << 33
    got = _run(lib, scores, bad_y, [1, 10], candidates=cand)
    np.testing.assert_array_equal(got["counts"], [0, 3])
    np.testing.assert_array_equal(got["row_counts"][:, 1], [0, 2, 1, 0, 0])
    np.testing.assert_array_equal(got["row_counts"][:, 2:4], rr.per_row(scores, np.where(bad_y == 1, 1, 0), [1, 10], cand)[1])
    fl = bad_y.astype(np.float32)
    fl[4, 4] = 0.5
    np.testing.assert_array_equal(_run(lib, scores, fl, [1, 10], candidates=cand)["counts"], [0, 4])


def test_argument_errors_and_the_empty_batch_change_no_byte():
    lib = _lib.load()
    s, y = rr.edge_rows()
    B, C = y.shape
    ks = [1, 5]
    wbytes = lib.tbe_rank_metrics_workspace_bytes(B, 2)
    ones = lambda n: np.ones(n, dtype=np.float32)  # noqa: E731
    bufs = {"s": Buf(B * C, s), "y": _raw_buf(y), "c": _raw_buf(np.zeros((B, C), dtype=np.int64)),
            "w": Buf(5, ranking.dcg_weights(5).numpy()), "m": Buf(4, ones(4)), "cnt": _raw_buf(np.full(2, -7, dtype=np.int64)),
            "ws": Buf(wbytes // 4, ones(wbytes // 4))}
    before = {k: b.all().copy() for k, b in bufs.items()}
    P = {k: b.ptr for k, b in bufs.items()}

    def call(B=B, C=C, ks=ks, stride=C, V=C, cand=None, esize=8, ws_bytes=wbytes, **kw):
        p = dict(P, **kw)
        arr = (ctypes.c_int32 * max(len(ks), 1))(*ks)
        rc = lib.tbe_rank_metrics_f32(p["s"], stride, cand, V, p["y"], esize, B, C, arr, len(ks), p["w"], p["m"], p["cnt"],
                                      p["ws"], ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    for kw, text in (({"C": 0}, "C=0"), ({"C": 8193}, "C=8193"), ({"ks": [0, 5]}, "k=0"), ({"ks": [1, 9]}, "k=9"),
                     ({"ks": [5, 1]}, "ascending"), ({"ks": [1, 1]}, "ascending"), ({"ks": []}, "nk=0"),
                     ({"ks": list(range(1, 10)), "C": 12, "stride": 12}, "nk=9"), ({"esize": 2}, "labels must be"),
                     ({"stride": C - 1}, "score_row_stride"), ({"cand": P["c"], "V": 0}, "V=0"),
                     ({"cand": P["c"], "V": C + 1}, "score_row_stride"), ({"B": -1}, "B=-1"), ({"s": None}, "null"),
                     ({"y": None}, "null"), ({"w": None}, "null"), ({"m": None}, "null"), ({"cnt": None}, "null"),
                     ({"ws": None}, "null"), ({"s": P["s"] + 2}, "aligned"), ({"y": P["y"] + 4}, "aligned"),
                     ({"cnt": P["cnt"] + 4}, "aligned"), ({"ws": P["ws"] + 16}, "256-B")):
        rc, msg = call(**kw)
        assert rc == INVALID and text in msg and "tbe_rank_metrics_f32" in msg, (kw, rc, msg)
    rc, msg = call(ws_bytes=wbytes - 256)
    assert rc == WORKSPACE and "workspace" in msg
    assert lib.tbe_rank_metrics_workspace_bytes(-1, 2) == 0 and lib.tbe_rank_metrics_workspace_bytes(4, 9) == 0
    for k, b in bufs.items():
        np.testing.assert_array_equal(b.all().view(np.uint32), before[k].view(np.uint32), err_msg=k)
    # B == 0: the mean of nothing is NaN, the counts are 0, nothing else is touched
    rc, msg = call(B=0)
    assert rc == OK, msg
    assert np.isnan(bufs["m"].get()).all()
    np.testing.assert_array_equal(bufs["cnt"].get().view(np.int64), [0, 0])
    for k in ("s", "y", "c", "w", "ws"):
        np.testing.assert_array_equal(bufs[k].all().view(np.uint32), before[k].view(np.uint32), err_msg=k)
