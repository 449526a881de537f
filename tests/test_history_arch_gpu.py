"""GPU: tbe_history_forward_f32 / tbe_history_backward_f32 (csrc/history_arch.hip) through the C ABI between guard elements,
against a float64 restatement of include/tbe_hip.h written here, and HistoryArch's kernel path against its torch expression.

Tolerance, per case: 8 x the worst float32-vs-float64 error of torch's own composition (index_select, add, F.layer_norm,
multiply by the same keep multipliers, autograd) on the same inputs, measured here and printed — the project's rule for its
row kernels; the factor covers another summation order.  The mean's error is taken in units of the sample's standard
deviation, which is how it enters y: a mean near zero has no relative error worth the name.  Measured (MI355X; torch's side depends a
little on the host's torch build): torch's worst error per case 4.7e-8 (all-empty batch) ... 3.5e-7 (1030 samples of (3, 4)), so
tolerances of 3.7e-7 ... 2.8e-6; the kernels' worst 6.2e-7 at the 1030-sample case (grad beta), at most 1.8e-7 at every other."""
import functools

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
from _crossnet_ref import rel_err  # max |a - ref| / max |ref|
from _guarded import CANARY, Buf, TypedBuf
from _residual_layernorm_ref import keep

pytestmark = pytest.mark.gpu
EPS, SITE, SEED, CALL = 1e-5, 4, 20240917, 7
ROWS, LO, GLOBAL = 40, 16, 64  # the shard holds the global rows [16, 56) of a table of 64

# (L, E, B, p): fewer elements than threads; a second sample per workgroup at 256 threads (B > 1024); one shape per slot
# class of 256 threads (1, 2, 4, 8 float4 per thread) and of 1024 threads (4, 8); an odd L with ragged slots and a second
# sample per workgroup at 1024 threads (B > 256); the reference's default; L * E exactly at the cap
SHAPES = [(3, 4, 1, 0.0), (3, 4, 1030, 0.1), (8, 16, 5, 0.1), (20, 64, 5, 0.0), (40, 64, 5, 0.1), (100, 64, 5, 0.0),
          (100, 128, 5, 0.1), (137, 128, 260, 0.1), (100, 256, 5, 0.0), (100, 256, 5, 0.1), (128, 256, 1, 0.1)]
# (L, E, B, p, want, window, all_empty): every shape with all three sums, then (8, 16) with each sum switched off, with
# none, without a row window, and as an all-empty batch
CASES = ([s + (7, True, False) for s in SHAPES] + [(8, 16, 5, 0.1, w, True, False) for w in (6, 5, 3, 0)]
         + [(8, 16, 5, 0.0, 7, False, False), (8, 16, 5, 0.1, 7, True, True)])


@functools.lru_cache(maxsize=None)
def inputs(L, E, B, p, window, all_empty):
    """Lengths 0, 1, L - 1, L, L + 3 in turn from sample 0 on (a batch of one: L), ids over the whole table — most of them
    another shard's under the window — and one bad id at the first kept position."""
    rng = np.random.default_rng([L, E, B, int(window)])
    pattern = [0, 1, L - 1, L, L + 3] if B > 1 else [L]
    lengths = np.array([0 if all_empty else pattern[b % 5] for b in range(B)], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    N = int(offsets[-1])
    lo, top = (LO, GLOBAL) if window else (0, ROWS)
    ids = rng.integers(0, top, size=N).astype(np.int64)
    if N:
        ids[0] = top + 5
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    return {"table": f(ROWS, E), "pos": f(L, E), "gamma": f(L, E), "beta": f(L, E), "gy": f(B, L, E), "ids": ids,
            "offsets": offsets, "lo": lo, "top": top, "keep": keep(p, SEED, CALL, SITE, B, L * E).reshape(B, L, E)}


def gathered(c, L):
    """(rows [B, L] of the table or -1, the float mask of the kept positions with a local row) — jagged_2d_to_dense's rule."""
    B = len(c["offsets"]) - 1
    rows = np.full((B, L), -1, dtype=np.int64)
    for b in range(B):
        seg = c["ids"][c["offsets"][b]:c["offsets"][b + 1]][:L] - c["lo"]
        rows[b, :len(seg)] = np.where((seg >= 0) & (seg < ROWS), seg, -1)
    return rows, (rows >= 0)[..., None]


def restate(c, L, E, dtype):
    """float64: the formulas of the header with numpy.  float32: torch's composition of the same operations."""
    rows, has = gathered(c, L)
    if dtype == np.float64:
        t, pos, gamma, beta, gy, k = (c[n].astype(np.float64) for n in ("table", "pos", "gamma", "beta", "gy", "keep"))
        x = np.where(has, t[np.maximum(rows, 0)], 0.0) + pos
        mean = x.mean(axis=(1, 2), keepdims=True)
        rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=(1, 2), keepdims=True) + EPS)
        xh, g = (x - mean) * rstd, gy * k
        d = g * gamma
        gx = rstd * (d - d.mean(axis=(1, 2), keepdims=True) - xh * (d * xh).mean(axis=(1, 2), keepdims=True))
        out = {"y": (xh * gamma + beta) * k, "mean": mean.ravel(), "rstd": rstd.ravel(), "gx": gx * has,
               "gp": np.stack([gx.sum(0), (g * xh).sum(0), g.sum(0)])}
    else:
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()  # noqa: E731
        emb = (T(c["table"])[torch.from_numpy(np.maximum(rows, 0))] * T(has)).requires_grad_()
        pos, gamma, beta = (T(c[n]).requires_grad_() for n in ("pos", "gamma", "beta"))
        x = emb + pos
        y = torch.nn.functional.layer_norm(x, (L, E), gamma, beta, EPS) * T(c["keep"])
        (y * T(c["gy"])).sum().backward()
        out = {"y": y, "mean": x.mean(dim=(1, 2)), "rstd": 1.0 / torch.sqrt(x.var(dim=(1, 2), unbiased=False) + EPS),
               "gx": emb.grad * T(has), "gp": torch.stack([pos.grad, gamma.grad, beta.grad])}
        out = {n: v.detach().double().numpy() for n, v in out.items()}
    return out


def errors(got, ref, names):
    e = {n: rel_err(got[n], ref[n]) for n in names if n != "mean"}
    e["mean"] = float(np.abs(got["mean"] - ref["mean"]).max() * ref["rstd"].min())
    return e


@functools.lru_cache(maxsize=None)
def reference(L, E, B, p, window, empty):
    """(the float64 restatement of the case, its tolerance): computed once, shared by the cases that differ in `want` only."""
    c = inputs(L, E, B, p, window, empty)
    ref = restate(c, L, E, np.float64)
    worst = max(errors(restate(c, L, E, np.float32), ref, list(ref)).values())
    print(f"({L}, {E}, {B}, {p}): torch float32 composition vs float64: worst {worst:.3g}; tolerance {8 * worst:.3g}")
    return ref, 8.0 * worst


def run(lib, c, L, E, p, want, window):
    """One forward and one backward between guards: the outputs, the counter and the inputs as read back."""
    B, N = len(c["offsets"]) - 1, len(c["ids"])
    fw = TypedBuf(1, np.int64, [0])
    fr, fwin = TypedBuf(1, np.int64, [ROWS]), TypedBuf(2, np.int64, [c["lo"], c["top"]])
    ids, offs, err = TypedBuf(N, np.int64, c["ids"]), TypedBuf(B + 1, np.int64, c["offsets"]), TypedBuf(1, np.int32, [0])
    table, pos, gamma, beta, gy = (Buf(c[n].size, c[n]) for n in ("table", "pos", "gamma", "beta", "gy"))
    fw.t[fw.guard] = table.ptr
    y, stats, gemb, gp = Buf(B * L * E), Buf(2 * B), Buf(N * E), Buf(3 * L * E)
    wbytes = lib.tbe_history_backward_workspace_bytes(B, L, E, want)
    ws = Buf(wbytes // 4)
    common = (fw.ptr, fr.ptr, fwin.ptr if window else None, ids.ptr, N, offs.ptr, B, L, E)
    rc = lib.tbe_history_forward_f32(*common, pos.ptr, gamma.ptr, beta.ptr, EPS, p, SITE, SEED, CALL, y.ptr, stats.ptr,
                                     err.ptr, None)
    assert rc == 0, lib.tbe_last_error()
    rc = lib.tbe_history_backward_f32(gy.ptr, *common, pos.ptr, gamma.ptr, stats.ptr, p, SITE, SEED, CALL, gemb.ptr,
                                      gp.ptr if want else None, want, ws.ptr if want else None, wbytes, None)
    assert rc == 0, lib.tbe_last_error()
    torch.cuda.synchronize()
    ws.get()
    for n, b in (("table", table), ("pos", pos), ("gamma", gamma), ("beta", beta), ("gy", gy), ("ids", ids), ("offsets", offs)):
        np.testing.assert_array_equal(b.get(), c[n].reshape(-1), err_msg=f"input {n} changed")
    return {"y": y.get((B, L, E)), "stats": stats.get((B, 2)), "gemb": gemb.get((N, E)), "gp": gp.get((3, L, E)),
            "errors": int(err.get()[0])}


@pytest.mark.parametrize("L,E,B,p,want,window,empty", CASES)
def test_kernels_match_the_float64_restatement(L, E, B, p, want, window, empty):
    from fbgemm_gpu import _lib

    lib, c = _lib.load(), inputs(L, E, B, p, window, empty)
    assert lib.tbe_history_supported(L, E) == 1
    got, again = run(lib, c, L, E, p, want, window), run(lib, c, L, E, p, want, window)
    for n in ("y", "stats", "gemb", "gp"):
        np.testing.assert_array_equal(got[n].view(np.uint32), again[n].view(np.uint32), err_msg=f"{n}: two runs differ")
    ref, tol = reference(L, E, B, p, window, empty)
    # the jagged gradient: row offsets[b] + l is position l of sample b; everything else is +0.0, bit for bit
    rows, has = gathered(c, L)
    lengths = np.diff(c["offsets"])
    ref_emb, live = np.zeros((len(c["ids"]), E)), np.zeros(len(c["ids"]), dtype=bool)
    for b in range(B):
        n = min(int(lengths[b]), L)
        ref_emb[c["offsets"][b]:c["offsets"][b] + n] = ref["gx"][b, :n]
        live[c["offsets"][b]:c["offsets"][b] + n] = rows[b, :n] >= 0
    assert (got["gemb"][~live].view(np.uint32) == 0).all(), "a truncated, foreign or bad position is not +0.0"
    got.update(mean=got["stats"][:, 0], rstd=got["stats"][:, 1])
    errs = errors(got, ref, ["y", "mean", "rstd"])
    if live.any():
        errs["gemb"] = rel_err(got["gemb"], ref_emb)
    for i, name in enumerate(("gpos", "ggamma", "gbeta")):
        if want >> i & 1:
            errs[name] = rel_err(got["gp"][i], ref["gp"][i])
        else:
            assert (got["gp"][i] == CANARY).all(), f"{name} was switched off and written"
    print(f"(L, E, B, p, want) = ({L}, {E}, {B}, {p}, {want}): {errs}; tolerance {tol:.3g}")
    assert max(errs.values()) <= tol, errs
    assert got["errors"] == (1 if len(c["ids"]) else 0)


def test_a_shape_past_the_cap_and_bad_arguments_are_refused_with_nothing_written():
    from fbgemm_gpu import _lib

    lib = _lib.load()
    assert lib.tbe_history_supported(128, 256) == 1 and lib.tbe_history_supported(129, 256) == 0
    L, E, B = 129, 256, 1
    i64, out, prm = TypedBuf(4, np.int64, [0, ROWS, 0, 0]), Buf(B * L * E), Buf(3 * L * E)
    fwd = lambda L, E, p, eps, y: lib.tbe_history_forward_f32(  # noqa: E731
        i64.ptr, i64.ptr + 8, None, i64.ptr, 0, i64.ptr + 16, B, L, E, prm.ptr, prm.ptr, prm.ptr, eps, p, SITE, SEED, CALL, y,
        out.ptr, None, None)
    bwd = lambda L, E, want, ws, wbytes: lib.tbe_history_backward_f32(  # noqa: E731
        out.ptr, i64.ptr, i64.ptr + 8, None, i64.ptr, 0, i64.ptr + 16, B, L, E, prm.ptr, prm.ptr, out.ptr, 0.0, SITE, SEED,
        CALL, None, prm.ptr, want, ws, wbytes, None)
    assert fwd(129, 256, 0.0, EPS, out.ptr) == -1 and b"unsupported" in lib.tbe_last_error()
    assert fwd(8, 16, 1.0, EPS, out.ptr) == -1 and fwd(8, 16, 0.0, -1.0, out.ptr) == -1
    assert fwd(8, 16, 0.0, EPS, out.ptr + 4) == -1 and fwd(8, 16, 0.0, EPS, None) == -1
    assert bwd(129, 256, 7, out.ptr, 1 << 20) == -1 and bwd(8, 16, 8, out.ptr, 1 << 20) == -1
    assert bwd(8, 16, 7, out.ptr, 16) == -1 and b"workspace" in lib.tbe_last_error()
    assert bwd(8, 16, 7, None, 1 << 20) == -1
    torch.cuda.synchronize()
    assert (out.get() == CANARY).all() and (prm.get() == CANARY).all()


def test_an_empty_batch_launches_nothing_forward_and_zeroes_the_wanted_sums():
    from fbgemm_gpu import _lib

    lib, L, E = _lib.load(), 8, 16
    gp = Buf(3 * L * E)
    assert lib.tbe_history_forward_f32(None, None, None, None, 0, None, 0, L, E, None, None, None, EPS, 0.0, SITE, SEED, CALL,
                                       None, None, None, None) == 0
    assert lib.tbe_history_backward_f32(None, None, None, None, None, 0, None, 0, L, E, None, None, None, 0.0, SITE, SEED, CALL,
                                        None, gp.ptr, 5, None, 0, None) == 0
    torch.cuda.synchronize()
    got = gp.get((3, L * E))
    assert (got[0].view(np.uint32) == 0).all() and (got[1] == CANARY).all() and (got[2].view(np.uint32) == 0).all()


# ---- the module: HistoryArch on the kernel path against kernel_path = False on the same weights.  Each path is within the
# tolerance of the (8, 16) case of five samples without dropout — the module tests' shape — of the exact result, so the two
# are within twice that of each other.
def module_tolerance():
    return 2 * reference(8, 16, 5, 0.0, False, False)[1]


def build_pair(fused, L=8, E=16, vocab=50, dropout=0.0, **more):
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from torchrec_amd.models import bert4rec as M

    params = ({"optimizer": EmbOptimType.ADAM, "learning_rate": 1e-2, "eps": 1e-8, "beta1": 0.9, "beta2": 0.999,
               "weight_decay": 0.0, **more} if fused else None)
    pair = []
    for _ in range(2):
        torch.manual_seed(5)
        pair.append(M.HistoryArch(vocab, L, E, dropout=dropout, device=torch.device("cuda", 0), fused_params=params))
    with torch.no_grad():
        pair[1].load_state_dict(pair[0].state_dict())
        pair[1].ec.table_weights()["item_embedding"].copy_(pair[0].ec.table_weights()["item_embedding"])
        for m in pair:  # away from the initial ones and zeros
            m.layernorm.weight.copy_(pair[0].positional * 0.5 + 1.0)
            m.layernorm.bias.copy_(pair[0].positional * 0.25)
    pair[1].kernel_path = False
    return pair


def batch(L, vocab=50, keys=("item",)):
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    rng = np.random.default_rng(3)
    lengths = np.array([0, 1, L - 1, L, L + 3, 4] * len(keys), dtype=np.int32)
    ids = rng.integers(0, vocab, size=int(lengths.sum())).astype(np.int64)
    return KeyedJaggedTensor.from_lengths_sync(list(keys), torch.from_numpy(ids).cuda(), torch.from_numpy(lengths).cuda())


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "dense"])
def test_history_arch_kernel_path_matches_its_torch_expression(fused):
    L, E = 8, 16
    pair, kjt, tol = build_pair(fused), batch(8), module_tolerance()
    g = torch.from_numpy(np.random.default_rng(4).standard_normal((6, L, E)).astype(np.float32)).cuda()
    outs = []
    for m in pair:
        y = m(kjt)
        y.backward(g)
        outs.append(y.detach())
    torch.cuda.synchronize()
    assert [m.last_path for m in pair] == ["kernel", "torch"]
    num = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    assert rel_err(num(outs[0]), num(outs[1])) <= tol
    for name in ("positional", "layernorm.weight", "layernorm.bias"):
        a, b = (num(m.get_parameter(name).grad) for m in pair)
        assert rel_err(a, b) <= tol, name
    if fused:  # one fused-ADAM step has run inside each backward
        a, b = (num(m.ec.table_weights()["item_embedding"]) for m in pair)
        assert pair[0].ec._tbe.iter == pair[1].ec._tbe.iter == 1
    else:
        a, b = (num(m.ec._tbe.weights.grad) for m in pair)
    assert rel_err(a, b) <= tol


def test_history_arch_falls_back_and_runs_without_autograd(monkeypatch):
    from fbgemm_gpu.split_embedding_configs import SparseType

    kernel, twin = build_pair(True)
    kjt = batch(8)
    with torch.no_grad():
        y = kernel(kjt)
    assert kernel.last_path == "kernel" and y.grad_fn is None and not y.requires_grad
    assert rel_err(y.double().cpu().numpy(), twin(kjt).detach().double().cpu().numpy()) <= module_tolerance()
    half = build_pair(True, weights_precision=SparseType.FP16)  # FP16 rows: the kernel would read halves as floats
    assert half[0].ec.table_weights()["item_embedding"].dtype == torch.float16
    assert torch.equal(half[0](kjt), half[1](kjt)) and half[0].last_path == "torch"
    raised = []  # keys beyond the collection's one feature: the torch expression's own error, on either switch
    for m in (kernel, twin):
        with pytest.raises(Exception) as info:
            m(batch(8, keys=("item", "other")))
        raised.append(info.type)
    assert raised[0] is raised[1] and kernel.last_path == "torch"
    assert kernel.eval()(kjt).shape == y.shape and kernel.last_path == "kernel"
    kernel.train()
    kernel.layernorm = torch.nn.LayerNorm([8, 16], elementwise_affine=False, device="cuda")
    kernel(kjt)
    assert kernel.last_path == "torch"
    for other in (build_pair(True, E=6)[0], build_pair(True, dropout=1.0)[0]):  # emb_dim % 4 != 0; p = 1 in training
        other(batch(8))
        assert other.last_path == "torch"
    drop = build_pair(True, dropout=0.5)[0]
    with monkeypatch.context() as mp:  # what a capturing stream answers: the call counter is host state
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        drop(kjt)
        assert drop.last_path == "torch" and drop._dropout_calls == 0
        drop.eval()(kjt)
        assert drop.last_path == "kernel"  # dropout inactive: nothing of the host's enters
        drop.train()
    # the draw is this kernel's: reproducible under the seed, moving between calls
    torch.manual_seed(1)
    a, b = drop(kjt).detach(), drop(kjt).detach()
    torch.manual_seed(1)
    drop._dropout_calls = 0
    assert drop.last_path == "kernel" and torch.equal(drop(kjt).detach(), a) and not torch.equal(a, b)
    assert 0.3 < float((a == 0).float().mean()) < 0.7


def test_a_backward_after_the_fused_update_of_another_forward_is_refused():
    """The backward recomputes xhat from the live table: once the table has moved, the saved (mean, rstd) are stale."""
    m, kjt = build_pair(True)[0], batch(8)
    y1, y2 = m(kjt), m(kjt)
    y2.sum().backward()
    with pytest.raises(RuntimeError, match="updated since"):
        y1.sum().backward()
