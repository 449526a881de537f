"""GPU: tbe_attention_tiled_forward_f32 / _backward_f32 through the C ABI against the float64 host model of
tests/_attention_ref.py, with canaries round out, the log-sum-exp, the D workspace, dq, dk and dv; and MultiHeadedAttention on
the tiled kernels against a float64 copy of itself.  Every tolerance is 8 x the float32 error of the torch composition on the
same inputs (never the kernel's own): R.measured_tolerance(SHAPES) was 9.02e-5 when first measured, the kernels' worst error
against the model 9.0e-7 on the ordinary inputs and 5.4e-6 (dQ) on the hot case."""
import copy

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _attention_ref as R
from _guarded import CANARY, Buf
from fbgemm_gpu import _lib
from torchrec_amd.models import bert4rec as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every power-of-two block edge up to 128 in L; a partial, an odd and a full column tile in d
SHAPES = ((1, 1, 1, 4), (2, 2, 15, 8), (1, 2, 17, 20), (2, 1, 63, 64), (1, 1, 64, 128), (2, 2, 65, 64), (1, 2, 127, 32),
          (1, 1, 129, 128), (1, 2, 200, 128), (1, 1, 257, 4), (1, 1, 300, 64))


def _tol():
    tol = R.measured_tolerance(SHAPES)
    print(f"measured tolerance (8 x worst float32 error of the torch composition): {tol:.3e}")
    return tol


class Run:
    """One forward + backward through the C ABI.  packed: q, k, v are column slices of one [B, L, 3 H d] buffer."""

    def __init__(self, q, k, v, g, valid=None, p=0.0, seed=0, call=0, packed=True, need=(True, True, True)):
        lib = _lib.load()
        B, L, H, d = q.shape
        row = H * d
        if packed:
            self.src = [Buf(B * L * 3 * row, np.concatenate([a.reshape(B, L, row) for a in (q, k, v)], axis=2))]
            ptrs = [self.src[0].ptr + 4 * row * n for n in range(3)]
            strides = (L * 3 * row, 3 * row)
        else:
            self.src = [Buf(B * L * row, a) for a in (q, k, v)]
            ptrs = [b.ptr for b in self.src]
            strides = (L * row, row)
        self.g = Buf(B * L * row, g)
        self.kv = None if valid is None else torch.from_numpy(valid.astype(np.uint8)).cuda()
        self.out, self.lse, self.ws = Buf(B * L * row), Buf(B * H * L), Buf(B * H * L)
        self.grads = [Buf(B * L * row) if w else None for w in need]
        qkv = [x for ptr in ptrs for x in (ptr, *strides)]
        kvp = None if self.kv is None else self.kv.data_ptr()
        rc = lib.tbe_attention_tiled_forward_f32(*qkv, kvp, B, H, L, d, p, seed, call, self.out.ptr, self.lse.ptr, None)
        assert rc == 0, lib.tbe_last_error()
        rc = lib.tbe_attention_tiled_backward_f32(self.g.ptr, self.out.ptr, *qkv, kvp, self.lse.ptr, B, H, L, d, p, seed, call,
                                                  self.ws.ptr, *[b.ptr if b is not None else None for b in self.grads], None)
        assert rc == 0, lib.tbe_last_error()
        torch.cuda.synchronize()
        shape = (B, L, H, d)
        self.o, self.l, self.D = self.out.get(shape), self.lse.get((B, H, L)), self.ws.get((B, H, L))
        self.dq, self.dk, self.dv = [b.get(shape) if b is not None else None for b in self.grads]

    def bits(self):
        return [a.view(np.uint32) for a in (self.o, self.l, self.D, self.dq, self.dk, self.dv) if a is not None]


def _check(run, q, k, v, g, valid, keep, tol, what):
    out, lse, _ = R.forward(q, k, v, valid, keep)
    dq, dk, dv = R.backward(g, q, k, v, valid, keep)
    D = np.einsum("bihc,bihc->bhi", g.astype(np.float64), out)
    errs = {n: R.assert_close(got, want, tol, f"{what} {n}")
            for n, got, want in (("out", run.o, out), ("D", run.D, D), ("dq", run.dq, dq), ("dk", run.dk, dk), ("dv", run.dv, dv))}
    for b in range(q.shape[0]):
        R.assert_close(run.l[b], lse[b], tol, f"{what} lse of sample {b}")
    print(what, {n: f"{e:.2e}" for n, e in errs.items()}, f"tol {tol:.2e}")


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "separate"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_match_the_host_model(shape, packed):
    B, H, L, d = shape
    q, k, v, g = R.make_inputs(B, H, L, d)
    tol = _tol()
    for pat in R.PATTERNS:
        valid = R.key_valid(pat, B, L)
        run = Run(q, k, v, g, valid, packed=packed)
        _check(run, q, k, v, g, valid, None, tol, f"{shape} {pat}")
        if pat in ("empty", "per_sample"):  # the sample without a valid key: uniform weights, dQ = 0, nothing into dK
            np.testing.assert_allclose(run.o[0], np.broadcast_to(v[0].astype(np.float64).mean(axis=0), v[0].shape),
                                       rtol=0, atol=tol * R.scale_of(v[0]))
            assert (run.dq[0] == 0).all() and (run.dk[0] == 0).all()


@pytest.mark.parametrize("pat", ["none", "per_sample"])
def test_scores_above_100_do_not_overflow(pat):
    B, H, L, d = R.HOT
    q, k, v, g = R.make_inputs(B, H, L, d, 6.0)
    assert np.abs(np.einsum("bihc,bjhc->bhij", q.astype(np.float64), k) / np.sqrt(d)).max() > 100
    valid = R.key_valid(pat, B, L)
    _check(Run(q, k, v, g, valid), q, k, v, g, valid, None, _tol(), f"hot {pat}")


@pytest.mark.parametrize("p, seed, call", R.DROPOUT)
@pytest.mark.parametrize("shape", [(3, 2, 7, 8), (2, 2, 65, 64)], ids=lambda s: "x".join(map(str, s)))
def test_dropout_equals_the_model_fed_the_restated_mask(shape, p, seed, call):
    B, H, L, d = shape
    q, k, v, g = R.make_inputs(B, H, L, d)
    keep = R.dropout_keep(p, seed, call, B, H, L)
    for pat in ("none", "per_sample"):
        valid = R.key_valid(pat, B, L)
        _check(Run(q, k, v, g, valid, p, seed, call), q, k, v, g, valid, keep, _tol(), f"{shape} {pat} p={p}")


@pytest.mark.parametrize("p, seed, call", R.DROPOUT)
def test_dropout_mask_is_the_restated_draw_bit_for_bit(p, seed, call):
    """q = k = 0 makes P uniform and one-hot values put P~[i, j] into out[i, h, j]."""
    B, H, L, d = 1, 2, 128, 128
    q = k = np.zeros((B, L, H, d), np.float32)
    v = np.zeros((B, L, H, d), np.float32)
    v[:, np.arange(L), :, np.arange(L)] = 1.0
    run = Run(q, k, v, np.zeros_like(v), None, p, seed, call)
    kept = np.transpose(run.o, (0, 2, 1, 3)) != 0
    np.testing.assert_array_equal(kept, R.dropout_draws(seed, call, B, H, L) >= np.uint32(R.dropout_threshold(p)))


def test_p_zero_gives_the_bits_of_a_launch_without_dropout_and_two_runs_are_identical():
    B, H, L, d = 2, 2, 65, 64
    q, k, v, g = R.make_inputs(B, H, L, d)
    valid = R.key_valid("per_sample", B, L)
    plain = Run(q, k, v, g, valid).bits()
    for a, b in zip(plain, Run(q, k, v, g, valid, 0.0, 987654321, 55).bits()):
        np.testing.assert_array_equal(a, b)
    first, second = (Run(q, k, v, g, valid, 0.1, 5, 1).bits() for _ in range(2))
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    assert any((a != b).any() for a, b in zip(plain, first))


def test_unwanted_gradients_are_skipped_without_changing_the_others():
    B, H, L, d = 2, 2, 65, 64
    q, k, v, g = R.make_inputs(B, H, L, d)
    valid = R.key_valid("per_sample", B, L)
    full = Run(q, k, v, g, valid)
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        part = Run(q, k, v, g, valid, need=need)
        np.testing.assert_array_equal(part.D.view(np.uint32), full.D.view(np.uint32))  # written also without dq
        for got, want in zip((part.dq, part.dk, part.dv), (full.dq, full.dk, full.dv)):
            assert got is None or (got.view(np.uint32) == want.view(np.uint32)).all(), need


def test_every_argument_error_changes_no_byte():
    lib = _lib.load()
    B, H, L, d = 2, 2, 8, 8
    row = H * d
    src = Buf(B * L * row, np.ones(B * L * row, np.float32))
    outs = [Buf(B * L * row) for _ in range(4)] + [Buf(B * H * L) for _ in range(2)]  # out, dq, dk, dv, lse, D_ws
    good = dict(q=src.ptr, k=src.ptr, v=src.ptr, bs=L * row, rs=row, B=B, H=H, L=L, d=d, p=0.0, out=outs[0].ptr,
                lse=outs[4].ptr, g=src.ptr, o=src.ptr, ws=outs[5].ptr)
    bad = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(lse=None), dict(g=None), dict(o=None), dict(ws=None),
           dict(B=-1), dict(H=0), dict(L=0), dict(L=-3), dict(d=0), dict(d=6), dict(d=132), dict(L=4097), dict(rs=row - 4),
           dict(rs=row + 2), dict(bs=L * row - 4), dict(p=1.0), dict(p=-0.1), dict(p=float("nan")), dict(q=src.ptr + 4),
           dict(B=2 ** 30, H=1, L=200, bs=200 * row)]  # the last: 2^32 workgroups
    for change in bad:
        a = {**good, **change}
        qkv = [x for t in ("q", "k", "v") for x in (a[t], a["bs"], a["rs"])]
        if not {"g", "o", "ws"} & set(change):
            rc = lib.tbe_attention_tiled_forward_f32(*qkv, None, a["B"], a["H"], a["L"], a["d"], a["p"], 1, 2, a["out"], a["lse"],
                                                     None)
            assert rc == -1, (change, rc)
        if "out" not in change:
            rc = lib.tbe_attention_tiled_backward_f32(a["g"], a["o"], *qkv, None, a["lse"], a["B"], a["H"], a["L"], a["d"], a["p"],
                                                      1, 2, a["ws"], outs[1].ptr, outs[2].ptr, outs[3].ptr, None)
            assert rc == -1, (change, rc)
        assert lib.tbe_last_error()
    qkv = [src.ptr, L * row, row] * 3
    assert lib.tbe_attention_tiled_forward_f32(*qkv, None, 0, H, L, d, 0.0, 0, 0, outs[0].ptr, outs[4].ptr, None) == 0  # B == 0
    torch.cuda.synchronize()
    for b in outs:
        assert (b.all() == CANARY).all(), "an entry that launches nothing wrote something"


# ---- the module

def _step(m, x, g, mask):
    """(out, dx, parameter gradients) of one forward + backward."""
    out = m(x, x, x, mask=mask)
    return [out.detach(), *torch.autograd.grad(out, [x] + list(m.parameters()), g)]


def _module_case(L, dim=256, B=2):
    torch.manual_seed(L)
    m = M.MultiHeadedAttention(num_heads=2, dim_model=dim, dropout=0.0, device=torch.device(DEV))
    x = torch.randn(B, L, dim, device=DEV).requires_grad_()
    g = torch.randn(B, L, dim, device=DEV)
    mask = torch.from_numpy(R.key_valid("per_sample", B, L)).to(DEV)[:, None, None, :].expand(B, 1, L, L)
    m64 = copy.deepcopy(m).double()
    m64.kernel_path = False
    want = [t.detach() for t in _step(m64, x.detach().double().requires_grad_(), g.double(), mask)]
    twin = copy.deepcopy(m)
    twin.kernel_path = False
    # 8 x the float32 torch twin's own error against the float64 copy, per tensor, of that tensor's scale or a thousandth of
    # the largest (the key projection's bias has an exactly zero gradient: rounding residue on both sides)
    floor = 1e-3 * max(float(b.abs().max()) for b in want)
    scales = [max(float(b.abs().max()), floor) for b in want]
    tol = 8 * max(float((a.double() - b).abs().max()) / s for a, b, s in zip(_step(twin, x, g, mask), want, scales))
    return m, x, g, mask, want, scales, tol


def _assert_module(got, want, scales, tol, what):
    for n, (a, b, s) in enumerate(zip(got, want, scales)):
        err = float((a.double() - b).abs().max()) / s
        assert err <= tol, f"{what}: tensor {n} error {err:.3e}, tolerance {tol:.3e}"


def test_module_takes_the_tiled_kernels_at_200_by_128_and_matches_its_float64_copy():
    m, x, g, mask, want, scales, tol = _module_case(200)
    got = _step(m, x, g, mask)
    assert (m.last_path, m.last_kernel) == ("kernel", "tiled")
    print(f"module tolerance at L = 200: {tol:.3e}")
    _assert_module(got, want, scales, tol, "tiled (200, 128)")


def test_prefer_tiled_agrees_with_the_resident_kernels_at_100_by_128():
    m, x, g, mask, want, scales, tol = _module_case(100)
    resident = _step(m, x, g, mask)
    assert (m.last_path, m.last_kernel) == ("kernel", "resident")
    m.prefer_tiled = True
    tiled = _step(m, x, g, mask)
    assert (m.last_path, m.last_kernel) == ("kernel", "tiled")
    _assert_module(tiled, [t.double() for t in resident], scales, tol, "tiled against resident (100, 128)")
    _assert_module(tiled, want, scales, tol, "tiled (100, 128)")


def test_forward_and_backward_captured_into_a_hip_graph_replay_the_eager_bits():
    m, x, g, mask, _, _, _ = _module_case(200)
    eager = [t.detach().clone() for t in _step(m, x, g, mask)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(m, x, g, mask)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(m, x, g, mask)
    assert (m.last_path, m.last_kernel) == ("kernel", "tiled")
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)
