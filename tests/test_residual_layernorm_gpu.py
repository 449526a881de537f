"""GPU: csrc/residual_layernorm.hip through the C ABI between guard elements, against the float64 restatement
(tests/_residual_layernorm_ref.py) within the tolerance measured there, and TransformerBlock / BERT4Rec on the fused path
against their torch path."""
import copy

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _attention_ref as A
import _bert4rec_golden as G
import _residual_layernorm_ref as rr
from _guarded import Buf
from fbgemm_gpu import _lib
from torchrec_amd.models import bert4rec as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, INVALID = 0, -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _abi_run(lib, c, variant):
    """Forward and backward of one case through the ABI; outputs laid out like rr.run's."""
    has_s, p_in, p_out, want_n, want_y, has_gy, want_pg = rr.VARIANTS[variant]
    R, N = c["x"].shape
    b = {k: Buf(c[k].size, c[k]) for k in ("x", "s", "gamma", "beta", "g_y", "g_n") if c[k] is not None}
    wbytes = lib.tbe_residual_layernorm_backward_workspace_bytes(R, N)
    o = {"y": Buf(R * N), "n": Buf(R * N), "stats": Buf(2 * R), "g_x": Buf(R * N), "g_s": Buf(R * N), "gp": Buf(2 * N),
         "ws": Buf(wbytes // 4)}
    P = lambda d, k, on=True: d[k].ptr if on and k in d else None  # noqa: E731
    drop = (p_in, rr.SITE_IN, p_out, rr.SITE_OUT, rr.SEED, rr.CALL)
    rc = lib.tbe_residual_layernorm_forward_f32(P(b, "x"), P(b, "s"), P(b, "gamma"), P(b, "beta"), rr.EPS, R, N, *drop,
                                                P(o, "y", want_y), P(o, "n", want_n), P(o, "stats", want_n), _stream())
    assert rc == OK, lib.tbe_last_error()
    rc = lib.tbe_residual_layernorm_backward_f32(
        P(b, "g_y", has_gy), P(b, "g_n", want_n), o["y"].ptr if want_y else b["x"].ptr, P(o, "stats", want_n), P(b, "gamma"), R,
        N, *drop, o["g_x"].ptr, P(o, "g_s", has_s), P(o, "gp", want_pg), P(o, "ws", want_pg), wbytes if want_pg else 0, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    for k, buf in b.items():
        np.testing.assert_array_equal(buf.get(), c[k].reshape(-1), err_msg=k)  # inputs are not modified
    raw = {k: buf.get() for k, buf in o.items()}  # guards round every output and the workspace
    wanted = {"y": want_y, "n": want_n, "stats": want_n, "g_x": True, "g_s": has_s, "gp": want_pg, "ws": want_pg}
    for k, w in wanted.items():
        assert w or (raw[k] == raw[k][0]).all() and raw[k][0] == np.float32(-12345.5), f"{k} written though not wanted"
    out = {k: raw[k].reshape(R, N) for k in ("y", "n", "g_x", "g_s") if wanted[k]}
    if want_n:
        out.update(mean=raw["stats"].reshape(R, 2)[:, 0], rstd=raw["stats"].reshape(R, 2)[:, 1])
    if want_pg:
        out.update(grad_gamma=raw["gp"][:N], grad_beta=raw["gp"][N:])
    return out


@pytest.mark.parametrize("R,N,variant", rr.cases())
def test_kernels_match_the_float64_restatement_and_repeat_bit_for_bit(R, N, variant):
    lib, c = _lib.load(), rr.inputs(R, N, variant)
    got, ref, tol = _abi_run(lib, c, variant), rr.run(c, variant), rr.tolerance()
    errs = rr.errors(got, ref)
    print(f"{R}x{N} {variant}: tolerance {tol:.3e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(np.isfinite(v).all() for v in got.values())
    if "y" in got:  # the keep decisions are the numpy draw's: y == 0 <=> dropped by drop_out, y == x * scale <=> s dropped
        kept_out = c["k_out"] != 0
        np.testing.assert_array_equal(got["y"] != 0, kept_out)
        if c["s"] is not None:
            bare = (c["x"].astype(np.float64) * c["k_out"]).astype(np.float32)
            np.testing.assert_array_equal((got["y"] == bare)[kept_out], (c["k_in"] == 0)[kept_out])
    if variant == "norm_only" and R > 1:
        assert got["mean"][-1] == np.float32(1.5) and got["rstd"][-1] == np.float32(1.0) / np.sqrt(np.float32(rr.EPS))
    assert max(errs.values()) <= tol, errs
    again = _abi_run(lib, c, variant)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.uint32), again[k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("n", [4, 1020, 1028])  # a workgroup spans 256 threads x 4 floats
def test_relu_dropout_matches_numpy_bit_for_bit(n, p):
    lib = _lib.load()
    rng = np.random.default_rng(n)
    a, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    a[::5] = 0.0
    k = rr.keep(p, rr.SEED, rr.CALL, 3, 1, n)[0].astype(np.float32)
    ba, bg, bh, bga = Buf(n, a), Buf(n, g), Buf(n), Buf(n)
    assert lib.tbe_relu_dropout_forward_f32(ba.ptr, n, p, 3, rr.SEED, rr.CALL, bh.ptr, _stream()) == OK, lib.tbe_last_error()
    assert lib.tbe_relu_dropout_backward_f32(bg.ptr, bh.ptr, n, p, bga.ptr, _stream()) == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    h = np.where(k != 0, np.maximum(a, np.float32(0)) * k, np.float32(0))
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    np.testing.assert_array_equal(bh.get().view(np.uint32), h.view(np.uint32))
    np.testing.assert_array_equal(bga.get().view(np.uint32), np.where(h > 0, g * scale, np.float32(0)).view(np.uint32))
    if p and n > 4:  # both kinds of element occur (four draws may all be kept)
        assert (k == 0).any() and (k != 0).any()


def test_bad_arguments_are_refused_and_change_no_byte():
    lib = _lib.load()
    R, N = 5, 8
    wbytes = lib.tbe_residual_layernorm_backward_workspace_bytes(R, N)
    bufs = {k: Buf(n, np.ones(n)) for k, n in (("x", R * N), ("s", R * N), ("gamma", N), ("beta", N), ("y", R * N), ("n", R * N),
                                              ("stats", 2 * R), ("g_x", R * N), ("g_s", R * N), ("gp", 2 * N), ("ws", wbytes // 4))}
    before = {k: b.all().copy() for k, b in bufs.items()}
    P = {k: b.ptr for k, b in bufs.items()}

    def fwd(N=N, p_in=0.0, p_out=0.0, **kw):
        p = dict(P, **kw)
        return lib.tbe_residual_layernorm_forward_f32(p["x"], p["s"], p["gamma"], p["beta"], rr.EPS, R, N, p_in, 0, p_out, 1, 7, 0,
                                                      p["y"], p["n"], p["stats"], _stream())

    def bwd(N=N, p_in=0.0, p_out=0.0, ws_bytes=wbytes, **kw):
        p = dict(P, **kw)
        return lib.tbe_residual_layernorm_backward_f32(p["y"], p["n"], p["x"], p["stats"], p["gamma"], R, N, p_in, 0, p_out, 1, 7,
                                                       0, p["g_x"], p["g_s"], p["gp"], p["ws"], ws_bytes, _stream())

    bad = [dict(N=0), dict(N=6), dict(N=4100), dict(p_in=1.0), dict(p_out=-0.1), dict(p_out=float("nan")), dict(x=None),
           dict(x=P["x"] + 4), dict(gamma=None), dict(stats=None)]
    for call, more in ((fwd, [dict(y=None, n=None), dict(y=None, p_out=0.5), dict(s=P["s"] + 4), dict(n=P["n"] + 8)]),
                       (bwd, [dict(y=None, n=None), dict(n=None), dict(g_x=None), dict(g_s=P["g_s"] + 4), dict(ws=None),
                              dict(ws_bytes=wbytes - 256), dict(g_s=P["g_x"], p_in=0.5)])):
        for kw in bad + more:
            assert call(**kw) == INVALID and b"tbe_residual_layernorm" in lib.tbe_last_error(), kw
    for kw in (dict(n=6), dict(n=-4), dict(p=1.0), dict(a=None), dict(a=P["x"] + 4)):
        a = dict(dict(a=P["x"], n=8, p=0.0), **kw)
        assert lib.tbe_relu_dropout_forward_f32(a["a"], a["n"], a["p"], 3, 7, 0, P["y"], _stream()) == INVALID, kw
        assert lib.tbe_relu_dropout_backward_f32(a["a"], P["s"], a["n"], a["p"], P["g_x"], _stream()) == INVALID, kw
    torch.cuda.synchronize()
    for k, b in bufs.items():
        np.testing.assert_array_equal(b.all(), before[k], err_msg=k)


# ---- module level

def _block(hidden=32, p=0.0, seed=3):
    torch.manual_seed(seed)
    return M.TransformerBlock(hidden, 2, 4 * hidden, p, device=torch.device(DEV))


def _model(p=0.0):
    torch.manual_seed(4)
    return M.BERT4Rec(vocab_size=40, max_len=17, emb_dim=32, nhead=2, num_layers=2, dropout=p, device=torch.device(DEV))


def _kjt(B=3, L=17):
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    rng = np.random.default_rng(5)
    lengths = np.array([L, 5, 11], dtype=np.int32)[:B]
    return KeyedJaggedTensor.from_lengths_sync(["item"], torch.from_numpy(rng.integers(1, 40, int(lengths.sum()))).to(DEV),
                                               torch.from_numpy(lengths).to(DEV))


def _run_block(m, x, mask, g):
    xr = x.detach().to(next(m.parameters()).dtype).requires_grad_()
    return dict(_run(m, g, xr, mask), gx=xr.grad)


def _run(m, g, *args):
    m.zero_grad()
    out = m(*args)
    out.backward(g.to(out.dtype))
    return {"out": out.detach(), **{n: p.grad for n, p in m.named_parameters() if p.grad is not None}}


@pytest.mark.parametrize("kind", ["block", "model"])
def test_fused_path_agrees_with_the_torch_path_in_eval_mode(kind):
    """The tolerance rule of the ABI test, measured here: 8 x the torch path's float32 error against a float64 copy of the
    module, relative to each result's scale (the key bias, whose gradient is exactly 0, at its weight's: see
    tests/test_bert4rec_model.py)."""
    if kind == "block":
        fused, (B, L) = _block().eval(), (3, 17)
        x, g = torch.randn(B, L, 32, device=DEV), torch.randn(B, L, 32, device=DEV)
        mask = G.mask_of(A.key_valid("per_sample", B, L), "expand", DEV)
        run, blocks = (lambda m: _run_block(m, x, mask, g)), (lambda m: [m])
    else:
        fused, kjt, g = _model().eval(), _kjt(), torch.randn(3, 17, 40, device=DEV)
        run, blocks = (lambda m: _run(m, g, kjt)), (lambda m: list(m.transformer_blocks))
    plain, exact = copy.deepcopy(fused), copy.deepcopy(fused)
    for b in blocks(plain):
        b.kernel_path = False
    if kind == "block":
        exact = exact.double()
    else:  # HistoryArch (the lookup kernel's float32, the same bits in all three) stays; everything above it is float64
        exact.history.register_forward_hook(lambda _m, _i, out: out.double())
        exact.transformer_blocks.double(), exact.out.double()
    got, ref, hi = run(fused), run(plain), run(exact)
    assert all(b.last_path == "kernel" for b in blocks(fused)) and all(b.last_path == "torch" for b in blocks(plain))

    def err(a, b, n):
        scale = A.scale_of(hi[n].cpu().numpy())
        if n.endswith("linear_layers.1.bias"):
            scale = max(scale, A.scale_of(hi[n[:-len("bias")] + "weight"].cpu().numpy()))
        return float((a[n].double() - b[n].double()).abs().max()) / scale

    assert set(got) == set(ref) == set(hi)
    tol = 8.0 * max(err(ref, hi, n) for n in hi)
    errs = {n: err(got, ref, n) for n in hi}
    print(f"{kind}: tolerance {tol:.3e}, worst error {max(errs.values()):.3e}")
    assert max(errs.values()) <= tol, {n: e for n, e in errs.items() if e > tol}


def test_seeded_training_mode_reproduces_and_the_draw_keeps_its_rate():
    p, (R, N) = 0.1, (4096, 64)
    sd = np.sqrt(p * (1 - p) / (R * N))
    dropped = float((rr.keep(p, 11, 2, 2, R, N) == 0).mean())  # the condition on the draw, on the CPU first
    assert abs(dropped - p) <= 5 * sd, dropped
    from torchrec_amd.distributed._device_ops import residual_layernorm_forward

    y = residual_layernorm_forward(torch.ones(R, N, device=DEV), None, None, None, 0.0, (0.0, 0, p, 2, 11, 2))[0]
    assert float((y == 0).float().mean()) == pytest.approx(dropped, abs=1e-7)
    base = _block(p=p).train()
    x = torch.randn(3, 17, 32, device=DEV)
    mask = G.mask_of(A.key_valid("per_sample", 3, 17), "expand", DEV)
    runs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        m = copy.deepcopy(base)
        runs.append((m(x, mask).detach(), m(x, mask).detach()))
        assert m.last_path == "kernel"
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], runs[0][1]) and not torch.equal(runs[0][0], runs[2][0])
    xr = x.clone().requires_grad_()
    out = m(xr, mask)
    (g1,) = torch.autograd.grad(out, xr, torch.ones_like(out), retain_graph=True)
    (g2,) = torch.autograd.grad(out, xr, torch.ones_like(out))
    assert torch.equal(g1, g2) and bool(torch.isfinite(g1).all())


def test_gradients_follow_needs_input_grad_and_no_grad_keeps_nothing():
    m = _block().eval()
    x, g = torch.randn(3, 17, 32, device=DEV), torch.randn(3, 17, 32, device=DEV)
    mask = G.mask_of(A.key_valid("per_sample", 3, 17), "expand", DEV)
    full = _run_block(m, x, mask, g)
    frozen = [m.input_sublayer.norm.weight, m.output_sublayer.norm.bias]
    for q in frozen:
        q.requires_grad_(False)
    m.zero_grad()
    out = m(x, mask)  # x itself wants no gradient
    out.backward(g)
    assert all(q.grad is None for q in frozen) and torch.equal(out.detach(), full["out"])
    for n, q in m.named_parameters():
        assert q.requires_grad == (q.grad is not None) and (q.grad is None or torch.equal(q.grad, full[n])), n
    with torch.no_grad():
        quiet = m(x, mask)
    assert m.last_path == "kernel" and quiet.grad_fn is None and torch.equal(quiet, full["out"])


def test_forward_and_backward_captured_into_a_hip_graph_replay_the_eager_bits():
    m = _block(64).eval()
    x, gout = torch.randn(4, 33, 64, device=DEV).requires_grad_(), torch.randn(4, 33, 64, device=DEV)
    mask = G.mask_of(A.key_valid("per_sample", 4, 33), "expand", DEV)
    params = list(m.parameters())

    def step():
        return (lambda out: (out, *torch.autograd.grad(out, [x] + params, gout)))(m(x, mask))

    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    assert m.last_path == "kernel"
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, captured))


@pytest.mark.parametrize("dev,hidden", [(DEV, 6), ("cpu", 32)])
def test_unsupported_inputs_silently_take_the_torch_expression(dev, hidden):
    torch.manual_seed(0)
    m = M.TransformerBlock(hidden, 2, 4 * hidden, 0.0, device=torch.device(dev)).eval()
    x, twin = torch.randn(2, 5, hidden, device=dev), copy.deepcopy(m)
    twin.kernel_path = False
    assert torch.equal(m(x, None), twin(x, None)) and m.last_path == "torch"
