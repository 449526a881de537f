"""GPU: tbe_attention_forward_f32 / _backward_f32 through the C ABI against the float64 host model of
tests/_attention_ref.py, with canaries round out, the log-sum-exp, dq, dk and dv.  The tolerance is the one
tests/test_attention.py measures from the torch composition on these very inputs (never from the kernel)."""
import ctypes

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _attention_ref as R
from _guarded import CANARY, Buf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu


def _supported(L, d):
    return bool(_lib.load().tbe_attention_supported(L, d))


EXTRA = ((1, 1, R.max_L(_supported, 128), 128),)  # the LDS limit
ALL_SHAPES = list(R.SHAPES) + list(EXTRA)


def _tol():
    return R.measured_tolerance(EXTRA)


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
        self.out, self.lse = Buf(B * L * row), Buf(B * H * L)
        self.grads = [Buf(B * L * row) if w else None for w in need]
        qkv = [x for ptr in ptrs for x in (ptr, *strides)]
        kvp = None if self.kv is None else self.kv.data_ptr()
        self.rc_fwd = lib.tbe_attention_forward_f32(*qkv, kvp, B, H, L, d, p, seed, call, self.out.ptr, self.lse.ptr, None)
        assert self.rc_fwd == 0, lib.tbe_last_error()
        self.rc_bwd = lib.tbe_attention_backward_f32(self.g.ptr, *qkv, kvp, self.lse.ptr, B, H, L, d, p, seed, call,
                                                     *[b.ptr if b is not None else None for b in self.grads], None)
        assert self.rc_bwd == 0, lib.tbe_last_error()
        torch.cuda.synchronize()
        shape = (B, L, H, d)
        self.o, self.l = self.out.get(shape), self.lse.get((B, H, L))
        self.dq, self.dk, self.dv = [b.get(shape) if b is not None else None for b in self.grads]

    def bits(self):
        return [a.view(np.uint32) for a in (self.o, self.l, self.dq, self.dk, self.dv) if a is not None]


def _check(run, q, k, v, g, valid, keep, tol, what):
    out, lse, _ = R.forward(q, k, v, valid, keep)
    dq, dk, dv = R.backward(g, q, k, v, valid, keep)
    errs = {n: R.assert_close(got, want, tol, f"{what} {n}")
            for n, got, want in (("out", run.o, out), ("dq", run.dq, dq), ("dk", run.dk, dk), ("dv", run.dv, dv))}
    for b in range(q.shape[0]):
        R.assert_close(run.l[b], lse[b], tol, f"{what} lse of sample {b}")
    print(what, {n: f"{e:.2e}" for n, e in errs.items()}, f"tol {tol:.2e}")


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "separate"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_match_the_host_model(shape, packed):
    B, H, L, d = shape
    q, k, v, g = R.make_inputs(B, H, L, d)
    for pat in R.PATTERNS:
        valid = R.key_valid(pat, B, L)
        run = Run(q, k, v, g, valid, packed=packed)
        _check(run, q, k, v, g, valid, None, _tol(), f"{shape} {pat}")
        if pat in ("empty", "per_sample"):  # the sample without a valid key: uniform weights, dQ = 0, nothing into dK
            np.testing.assert_allclose(run.o[0], np.broadcast_to(v[0].astype(np.float64).mean(axis=0), v[0].shape),
                                       rtol=0, atol=_tol() * R.scale_of(v[0]))
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


def _mask_through_the_kernel(B, H, L, d, p, seed, call):
    """kept [B, H, L, L] read back exactly: q = k = 0 makes P uniform and one-hot values put P~[i, j] into out[i, h, j]."""
    assert L <= d
    q = k = np.zeros((B, L, H, d), np.float32)
    v = np.zeros((B, L, H, d), np.float32)
    v[:, np.arange(L), :, np.arange(L)] = 1.0
    run = Run(q, k, v, np.zeros_like(v), None, p, seed, call)
    return np.transpose(run.o[:, :, :, :L], (0, 2, 1, 3)) != 0


@pytest.mark.parametrize("p, seed, call", R.DROPOUT)
@pytest.mark.parametrize("shape", [(3, 2, 7, 8), (1, 2, 100, 128)], ids=lambda s: "x".join(map(str, s)))
def test_dropout_mask_is_the_restated_draw_bit_for_bit_and_moves_with_call(shape, p, seed, call):
    B, H, L, d = shape
    kept = _mask_through_the_kernel(B, H, L, d, p, seed, call)
    want = R.dropout_draws(seed, call, B, H, L) >= np.uint32(R.dropout_threshold(p))
    np.testing.assert_array_equal(kept, want)
    other = _mask_through_the_kernel(B, H, L, d, p, seed, call + 1)
    np.testing.assert_array_equal(other, R.dropout_draws(seed, call + 1, B, H, L) >= np.uint32(R.dropout_threshold(p)))
    assert (other != kept).any()


def test_p_zero_gives_the_bits_of_a_launch_without_dropout_and_two_runs_are_identical():
    B, H, L, d = 2, 2, 65, 64
    q, k, v, g = R.make_inputs(B, H, L, d)
    valid = R.key_valid("per_sample", B, L)
    plain = Run(q, k, v, g, valid).bits()
    for a, b in zip(plain, Run(q, k, v, g, valid, 0.0, 987654321, 55).bits()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(plain, Run(q, k, v, g, valid, packed=False).bits()):  # the layout changes no bit either
        np.testing.assert_array_equal(a, b)
    first, second = (Run(q, k, v, g, valid, 0.1, 5, 1).bits() for _ in range(2))
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    assert any((a != b).any() for a, b in zip(plain, first))


def test_unwanted_gradients_are_skipped_without_changing_the_others():
    B, H, L, d = 2, 2, 33, 32
    q, k, v, g = R.make_inputs(B, H, L, d)
    valid = R.key_valid("per_sample", B, L)
    full = Run(q, k, v, g, valid)
    only_q = Run(q, k, v, g, valid, need=(True, False, False))
    np.testing.assert_array_equal(only_q.dq.view(np.uint32), full.dq.view(np.uint32))
    kv = Run(q, k, v, g, valid, need=(False, True, True))
    np.testing.assert_array_equal(kv.dk.view(np.uint32), full.dk.view(np.uint32))
    np.testing.assert_array_equal(kv.dv.view(np.uint32), full.dv.view(np.uint32))


def test_every_argument_error_changes_no_byte():
    lib = _lib.load()
    B, H, L, d = 2, 2, 8, 8
    row = H * d
    src = Buf(B * L * row, np.ones(B * L * row, np.float32))
    outs = [Buf(B * L * row) for _ in range(4)]  # out, dq, dk, dv
    lse = Buf(B * H * L)
    good = dict(q=src.ptr, k=src.ptr, v=src.ptr, bs=L * row, rs=row, kv=None, B=B, H=H, L=L, d=d, p=0.0, out=outs[0].ptr,
                lse=lse.ptr, g=src.ptr)
    big_L = R.max_L(_supported, 128) + 1
    bad = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(lse=None), dict(g=None), dict(B=-1), dict(H=0),
           dict(L=0), dict(L=-3), dict(d=0), dict(d=6), dict(d=132), dict(L=big_L, d=128), dict(L=257, d=4), dict(rs=row - 4),
           dict(rs=row + 2), dict(bs=L * row - 4), dict(p=1.0), dict(p=-0.1), dict(p=float("nan")), dict(q=src.ptr + 4)]
    for change in bad:
        a = {**good, **change}
        qkv = [x for t in ("q", "k", "v") for x in (a[t], a["bs"], a["rs"])]
        if "g" not in change:
            rc = lib.tbe_attention_forward_f32(*qkv, a["kv"], a["B"], a["H"], a["L"], a["d"], a["p"], 1, 2, a["out"], a["lse"],
                                               None)
            assert rc == -1, (change, rc)
        if "out" not in change:
            rc = lib.tbe_attention_backward_f32(a["g"], *qkv, a["kv"], a["lse"], a["B"], a["H"], a["L"], a["d"], a["p"], 1, 2,
                                                outs[1].ptr, outs[2].ptr, outs[3].ptr, None)
            assert rc == -1, (change, rc)
        assert lib.tbe_last_error()
    torch.cuda.synchronize()
    for b in outs + [lse]:
        assert (b.all() == CANARY).all(), "an entry that reported an error wrote something"
    assert ctypes.c_int(lib.tbe_attention_forward_f32(src.ptr, L * row, row, src.ptr, L * row, row, src.ptr, L * row, row, None,
                                                      0, H, L, d, 0.0, 0, 0, outs[0].ptr, lse.ptr, None)).value == 0  # B == 0
    torch.cuda.synchronize()
    assert (outs[0].all() == CANARY).all()
