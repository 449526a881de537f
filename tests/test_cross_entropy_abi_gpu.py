"""GPU: csrc/cross_entropy.hip straight through the C ABI (include/tbe_hip.h), every output and the workspace between guard
elements that must stay untouched, the inputs checked to come back unmodified.  Results are compared with the float64
restatement (tests/_cross_entropy_ref.py) at 8 x the float32 error torch's own cross_entropy shows on these very inputs
(tests/test_cross_entropy.py prints it), and every case runs twice: the second run repeats the first bit for bit."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _cross_entropy_ref as cr
from _guarded import Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
CODE = {"mean": 0, "sum": 1, "none": 2}
GAP = np.float32(7.0)  # what the gradient buffer holds between the rows before the call


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i64_buf(values):
    """int64 values in a guarded float32 buffer (two elements each; the bits travel unchanged)."""
    a = np.ascontiguousarray(values, dtype=np.int64)
    return Buf(2 * a.size, a.view(np.float32))


def _run(lib, x, target, reduction, g, ignore=cr.IGNORE, off=0, stride=None):
    """One forward and one backward through the ABI.  The rows sit `off` bytes behind a 16-B aligned base, `stride` elements
    apart; the elements between them are NaN in the input (never to be read) and GAP in the gradient (never to be written)."""
    R, V = x.shape
    stride = V if stride is None else stride
    e = off // 4
    span = e + (max(R, 1) - 1) * stride + V
    xin = np.full(span, np.nan, dtype=np.float32)
    for r in range(R):
        xin[e + r * stride:e + r * stride + V] = x[r]
    n_out = R if reduction == "none" else 1
    bx, bt, bg = Buf(span, xin), _i64_buf(target), Buf(max(n_out, 1), np.resize(np.asarray(g, dtype=np.float32), max(n_out, 1)))
    bstats, bloss, bn, bgrad = Buf(2 * R), Buf(max(n_out, 1)), _i64_buf([-1]), Buf(span, np.full(span, GAP))
    wbytes = lib.tbe_cross_entropy_workspace_bytes(R)
    assert wbytes >= 4 * R and wbytes % 256 == 0
    bws = Buf(wbytes // 4)
    code = CODE[reduction]
    rc = lib.tbe_cross_entropy_forward_f32(bx.ptr + off, stride, bt.ptr, R, V, ignore, code, bstats.ptr, bloss.ptr, bn.ptr,
                                           bws.ptr, wbytes, _stream())
    assert rc == OK, lib.tbe_last_error()
    rc = lib.tbe_cross_entropy_backward_f32(bg.ptr, bx.ptr + off, stride, bt.ptr, bstats.ptr, bn.ptr, R, V, ignore, code,
                                            bgrad.ptr + off, stride, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    bws.get()  # guards round the workspace
    np.testing.assert_array_equal(bx.get().view(np.uint32), xin.view(np.uint32))  # inputs are not modified
    np.testing.assert_array_equal(bt.get().view(np.int64), np.asarray(target, dtype=np.int64))
    garr = bgrad.get()
    grad = np.stack([garr[e + r * stride:e + r * stride + V] for r in range(R)]) if R else np.zeros((0, V), np.float32)
    written = np.zeros(span, dtype=bool)
    for r in range(R):
        written[e + r * stride:e + r * stride + V] = True
    assert (garr[~written] == GAP).all(), "the gradient's gaps were written"
    loss = bloss.get()
    return {"loss": loss[:R] if reduction == "none" else loss[0], "grad": grad, "stats": bstats.get((2, R)),
            "n_valid": int(bn.get().view(np.int64)[0])}


def _same_bits(a, b):
    for k in ("loss", "grad", "stats"):
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg=k)
    assert a["n_valid"] == b["n_valid"]


def _check(lib, label, x, target, ignore=cr.IGNORE):
    tol = cr.gpu_tolerance()
    out = {}
    for red in cr.REDUCTIONS:
        g = cr.grad_out_for(x.shape[0], red)
        got = _run(lib, x, target, red, g, ignore)
        want = cr.run(x, target, ignore, red, g)
        errs = cr.result_errors(got, want)
        print(f"{label} {red}: tolerance loss {tol['loss']:.3e} grad {tol['grad']:.3e}, errors loss {errs['loss']:.2e} "
              f"grad {errs['grad']:.2e}")
        assert got["n_valid"] == want["n_valid"]
        assert errs["loss"] <= tol["loss"] and errs["grad"] <= tol["grad"], (red, errs, tol)
        _same_bits(got, _run(lib, x, target, red, g, ignore))
        out[red] = got
    # the three reductions share the rows' statistics and losses
    np.testing.assert_array_equal(out["mean"]["stats"], out["none"]["stats"])
    return out


@pytest.mark.parametrize("R,V,share", cr.abi_shapes())
def test_kernels_match_the_float64_restatement_and_repeat_bit_for_bit(R, V, share):
    """Widths (tests/_cross_entropy_ref.py ABI_WIDTHS): 1, the float4 edges 3 | 4 | 5, a wave's 63 | 64 | 65, both sides of
    the rule's edges 256 | 257 and 4096 | 4097, 1023 | 1024 | 1025 round one float4 trip of 256 threads, 2049, 3708, and
    26 746 at R = 5.  Rows: one, and three row blocks with a ragged last one at each geometry; 300 rows with 85 % ignored."""
    rpb = cr.rows_per_block(V)
    if share == 1.0 and R > 1 and V != 26746:
        assert -(-R // rpb) == 3 and (rpb == 1 or R % rpb != 0)
    x, target = cr.gpu_case(R, V, share)
    out = _check(_lib.load(), f"cross_entropy {R}x{V}@{share}", x, target)
    ignored = target == cr.IGNORE
    assert not out["none"]["loss"][ignored].any() and not out["mean"]["grad"][ignored].any()


@pytest.mark.parametrize("V", [5, 65, 1026, 4099, 4100])
def test_bits_do_not_depend_on_base_alignment_or_row_stride(V):
    """V % 4 = 1, 1, 2, 3, 0: a row then starts 0, 4, 8 or 12 bytes off the 16-byte grid, differently from row to row."""
    lib = _lib.load()
    R = cr.ragged_rows(V)
    x, target = cr.gpu_case(R, V, 0.7, seed=5)
    for red in ("mean", "none"):
        g = cr.grad_out_for(R, red)
        base = _run(lib, x, target, red, g)
        for off in (0, 4, 8, 12):
            for stride in (V, V + 1, V + 3):
                _same_bits(base, _run(lib, x, target, red, g, off=off, stride=stride))


@pytest.mark.parametrize("name,x,target", cr.label_cases(), ids=[c[0] for c in cr.label_cases()])
def test_label_and_value_cases(name, x, target):
    """Label 0 with ignore_index = -100, label V - 1, the label on the row maximum, logits of +-1e4, -inf entries."""
    out = _check(_lib.load(), name, x, target)
    assert np.isfinite(out["none"]["loss"]).all() and np.isfinite(out["mean"]["grad"]).all()
    if name.startswith("neg_inf"):
        assert not out["mean"]["grad"][np.isneginf(x)].any()  # a masked logit: probability 0, gradient 0
    if name.startswith("label_on_max"):
        assert (out["none"]["loss"] >= 0).all()


@pytest.mark.parametrize("V", [65, 1025, 4099])
def test_ignored_rows_are_never_read_and_bad_labels_stay_in_their_row(V):
    lib = _lib.load()
    R = cr.ragged_rows(V) + 2
    x, target = cr.gpu_case(R, V, 0.5, seed=9)
    clean = _run(lib, x, target, "mean", np.float32(1.0))
    ignored = target == cr.IGNORE
    assert ignored.any() and not ignored.all()
    poisoned = x.copy()
    poisoned[ignored] = np.nan
    poisoned[np.flatnonzero(ignored)[0], ::2] = np.inf
    got = _run(lib, poisoned, target, "mean", np.float32(1.0))
    _same_bits(clean, got)  # NaN / Inf inside an ignored row reaches nothing
    assert np.isfinite(got["loss"])
    zeros = got["grad"][ignored]
    assert not zeros.any() and not np.signbit(zeros).any()  # exact +0
    # a label of V and of -1 (ignore_index = -100): NaN in that row only, no address formed, no abort
    valid_rows = np.flatnonzero(~ignored)
    bad = target.copy()
    bad[valid_rows[0]], bad[valid_rows[-1]] = V, -1
    is_bad = np.isin(np.arange(R), [valid_rows[0], valid_rows[-1]])
    rows = _run(lib, x, bad, "none", cr.grad_out_for(R, "none"))
    want = _run(lib, x, target, "none", cr.grad_out_for(R, "none"))
    assert np.isnan(rows["loss"][is_bad]).all() and np.isnan(rows["grad"][is_bad]).all()
    assert np.isnan(rows["stats"][:, is_bad]).all()
    np.testing.assert_array_equal(rows["loss"][~is_bad], want["loss"][~is_bad])
    np.testing.assert_array_equal(rows["grad"][~is_bad], want["grad"][~is_bad])
    assert rows["n_valid"] == want["n_valid"]  # a bad label counts as valid
    for red in ("mean", "sum"):
        assert np.isnan(_run(lib, x, bad, red, np.float32(1.0))["loss"])


def test_no_valid_row_and_no_row():
    lib = _lib.load()
    x, _ = cr.gpu_case(20, 65)
    target = np.full(20, 3, dtype=np.int64)
    for rows in (20, 0):
        got = _run(lib, x[:rows], target[:rows], "mean", np.float32(1.0), ignore=3)
        assert np.isnan(got["loss"]) and got["n_valid"] == 0 and not got["grad"].any()
        got = _run(lib, x[:rows], target[:rows], "sum", np.float32(1.0), ignore=3)
        assert got["loss"] == 0.0 and got["n_valid"] == 0
        got = _run(lib, x[:rows], target[:rows], "none", cr.grad_out_for(rows, "none"), ignore=3)
        assert got["loss"].shape == (rows,) and not got["loss"].any() and got["n_valid"] == 0


def test_argument_errors_change_no_byte():
    lib = _lib.load()
    R, V = 9, 68
    x, target = cr.gpu_case(R, V)
    wbytes = lib.tbe_cross_entropy_workspace_bytes(R)
    ones = lambda n: np.ones(n, dtype=np.float32)  # noqa: E731
    bufs = {"x": Buf(R * V, x), "t": _i64_buf(target), "g": Buf(1, ones(1)), "stats": Buf(2 * R, ones(2 * R)),
            "loss": Buf(1, ones(1)), "n": _i64_buf([5]), "grad": Buf(R * V, ones(R * V)), "ws": Buf(wbytes // 4, ones(wbytes // 4))}
    before = {k: b.all().copy() for k, b in bufs.items()}
    P = {k: b.ptr for k, b in bufs.items()}

    def fwd(R=R, V=V, stride=V, red=0, ws_bytes=wbytes, **kw):
        p = dict(P, **kw)
        rc = lib.tbe_cross_entropy_forward_f32(p["x"], stride, p["t"], R, V, cr.IGNORE, red, p["stats"], p["loss"], p["n"],
                                               p["ws"], ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    def bwd(R=R, V=V, stride=V, gstride=V, red=0, **kw):
        p = dict(P, **kw)
        rc = lib.tbe_cross_entropy_backward_f32(p["g"], p["x"], stride, p["t"], p["stats"], p["n"], R, V, cr.IGNORE, red,
                                                p["grad"], gstride, _stream())
        torch.cuda.synchronize()
        return rc, lib.tbe_last_error().decode()

    for call in (fwd, bwd):
        for kw, text in (({"x": None}, "null"), ({"t": None}, "null"), ({"stats": None}, "null"), ({"stride": V - 1}, "row_stride"),
                         ({"V": 0}, "V=0"), ({"R": -1}, "R=-1"), ({"red": 3}, "reduction"), ({"x": P["x"] + 2}, "aligned"),
                         ({"t": P["t"] + 4}, "aligned")):
            rc, msg = call(**kw)
            assert rc == INVALID and text in msg and "tbe_cross_entropy" in msg, (kw, msg)
    for kw, text in (({"ws_bytes": wbytes - 256}, "workspace"), ({"ws": None}, "null"), ({"loss": None}, "null"),
                     ({"n": None}, "null")):
        rc, msg = fwd(**kw)
        assert rc == INVALID and text in msg, (kw, msg)
    for kw, text in (({"gstride": V - 1}, "grad_row_stride"), ({"grad": None}, "null"), ({"g": None}, "null")):
        rc, msg = bwd(**kw)
        assert rc == INVALID and text in msg, (kw, msg)
    assert lib.tbe_cross_entropy_workspace_bytes(-1) == 0
    for k, b in bufs.items():
        np.testing.assert_array_equal(b.all().view(np.uint32), before[k].view(np.uint32), err_msg=k)
