"""GPU: csrc/deepfm.hip straight through the C ABI (include/tbe_hip.h), bit for bit against the int64 model of
tests/_deepfm_ref.py.  The inputs make float32 exact in any summation order: x in {-1, 0, 1}, grad_fm an integer in
[-4, 4], grad_cat an integer in [-8, 8], N <= 3456, so s^2 <= 3456^2 < 2^24 and every product and sum is an integer or
half-integer below 2^24.  A dropped, repeated or misplaced column changes the result.

Every buffer lies between guard elements, the gaps of strided buffers and the columns of an unwanted gradient segment hold
canaries, and all of them must come back unchanged."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _deepfm_ref as dr
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

GUARD = 64  # float32 elements before and after every buffer (256 B: the payload keeps the allocation's alignment)
CANARY = np.float32(-12345.5)
OK = 0


class Strided:
    """A device [B, w] float32 block with row stride `stride`, starting `off` elements behind a 256-B aligned address, in a
    buffer that is canaries wherever it is not payload (guards, the offset, the gaps between rows)."""

    def __init__(self, B, w, stride=None, off=0, init=None):
        self.B, self.w, self.stride, self.off = B, w, stride or w, off
        n = off + (B - 1) * self.stride + w if B else off
        self.host = np.full(n + 2 * GUARD, CANARY, dtype=np.float32)
        if init is not None:
            self._payload(self.host)[...] = init
        self.t = torch.from_numpy(self.host).cuda()
        self.ptr = self.t.data_ptr() + 4 * (GUARD + off)

    def _payload(self, a):
        body = a[GUARD + self.off:len(a) - GUARD]
        return np.lib.stride_tricks.as_strided(body, (self.B, self.w), (4 * self.stride, 4)) if self.B else body[:0].reshape(0, self.w)

    def get(self):
        """The payload, after checking that nothing else changed."""
        a = self.t.cpu().numpy()
        out = self._payload(a).copy()
        self._payload(a)[...] = self._payload(self.host)
        assert np.array_equal(a, self.host), "bytes outside the payload were overwritten"
        return out

    def untouched(self):
        assert np.array_equal(self.t.cpu().numpy(), self.host), "a buffer that must not be written was written"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(xs, gfm, gcat, layout=None, wanted=None, fm_stride=1, gfm_stride=1):
    """Forward and backward of the segments `xs` through the ABI.  layout[k] = (row stride - width, offset in elements) of
    segment k's input AND gradient; returns (fm, row_sum, cat or None, [gradient or None])."""
    lib = _lib.load()
    B, nseg = xs[0].shape[0], len(xs)
    N = sum(x.shape[1] for x in xs)
    layout = layout or [(0, 0)] * nseg
    wanted = wanted or [True] * nseg
    ins = [Strided(B, x.shape[1], x.shape[1] + pad, off, x) for x, (pad, off) in zip(xs, layout)]
    segs = (_lib.FmSegment * nseg)()
    for k, b in enumerate(ins):
        segs[k].x, segs[k].row_stride, segs[k].width = b.ptr, b.stride, b.w
    fm, rs = Strided(B, 1, fm_stride), Strided(B, 1)
    cat = Strided(B, N) if gcat is not None else None
    rc = lib.tbe_fm_forward_f32(segs, nseg, B, fm.ptr, fm_stride, rs.ptr, cat.ptr if cat else None, _stream())
    assert rc == OK, lib.tbe_last_error()
    bgfm = Strided(B, 1, gfm_stride, 0, gfm.reshape(B, 1))
    bgcat = Strided(B, N, None, 0, gcat) if gcat is not None else None
    outs = [Strided(B, x.shape[1], x.shape[1] + pad, off) for x, (pad, off) in zip(xs, layout)]
    gsegs = (_lib.FmGradSegment * nseg)()
    for k, b in enumerate(outs):
        gsegs[k].g, gsegs[k].row_stride = (b.ptr, b.stride) if wanted[k] else (None, 0)
    rc = lib.tbe_fm_backward_f32(segs, gsegs, nseg, B, bgfm.ptr, gfm_stride, rs.ptr, bgcat.ptr if bgcat else None, _stream())
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()
    for b in ins + [bgfm] + ([bgcat] if bgcat else []):
        b.untouched()  # inputs are not modified
    grads = []
    for k, b in enumerate(outs):
        if wanted[k]:
            grads.append(b.get())
        else:
            b.untouched()
            grads.append(None)
    return fm.get()[:, 0], rs.get()[:, 0], cat.get() if cat else None, grads


def _inputs(rng, B, widths, with_cat):
    xs = [rng.integers(-1, 2, (B, w)).astype(np.float32) for w in widths]
    gfm = rng.integers(-4, 5, (B, 1)).astype(np.float32)
    gcat = rng.integers(-8, 9, (B, sum(widths))).astype(np.float32) if with_cat else None
    return xs, gfm, gcat


def _same(a, b, what):
    for name, u, v in zip(("fm", "row_sum", "cat"), a[:3], b[:3]):
        assert (u is None) == (v is None), (what, name)
        if u is not None:
            assert u.tobytes() == v.tobytes(), (what, name)
    for k, (u, v) in enumerate(zip(a[3], b[3])):
        assert (u is None) == (v is None) and (u is None or u.tobytes() == v.tobytes()), (what, "grad", k)


def _check(got, xs, gfm, gcat, wanted=None):
    fm, s, cat, grads = dr.fm_int_model(xs, gfm, gcat)
    np.testing.assert_array_equal(got[0], fm)
    np.testing.assert_array_equal(got[1], s)
    if gcat is not None:
        np.testing.assert_array_equal(got[2], cat)
    for k, g in enumerate(grads):
        if wanted is None or wanted[k]:
            np.testing.assert_array_equal(got[3][k], g, err_msg=f"gradient of segment {k}")


GEOMETRIES = [[1], [3], [4], [5], [255], [256], [257], [260], [3456], [8, 24], [3, 9], [128, 3328], [5, 260, 12], [1] * 8]


@pytest.mark.parametrize("with_cat", [True, False], ids=["cat", "nocat"])
@pytest.mark.parametrize("widths", GEOMETRIES, ids=lambda w: "x".join(map(str, w)) if len(w) < 8 else "8x1")
def test_kernels_equal_the_integer_model_on_every_path(widths, with_cat):
    """B = 1, 2 and 37 (more than one block at either rows-per-block: 32 for rows of up to 32 quads, 4 beyond); each once
    with tight, aligned segments (16-byte path wherever the widths allow it), once with every segment 4 B off the 16-byte
    grid and once with a row stride larger than the width — the scalar path — and the three must agree bit for bit.  Two
    runs are bit-identical."""
    rng = np.random.default_rng([len(widths), widths[0], with_cat])
    for B in (1, 2, 37):
        xs, gfm, gcat = _inputs(rng, B, widths, with_cat)
        aligned = _run(xs, gfm, gcat)
        _check(aligned, xs, gfm, gcat)
        _same(aligned, _run(xs, gfm, gcat), "second run")
        shifted = _run(xs, gfm, gcat, layout=[(0, 1)] * len(widths))
        _check(shifted, xs, gfm, gcat)
        _same(aligned, shifted, "4 B off the 16-byte grid")
        padded = _run(xs, gfm, gcat, layout=[(3, 0)] * len(widths))
        _check(padded, xs, gfm, gcat)
        _same(aligned, padded, "row stride = width + 3")


@pytest.mark.parametrize("with_cat", [True, False], ids=["cat", "nocat"])
def test_a_misaligned_segment_before_an_aligned_one_and_strides_in_multiples_of_four(with_cat):
    """One launch mixes both paths: segment 0 is 4 B off the grid (scalar), segment 1 aligned with a padded row stride that
    is a multiple of 4 (vector, guard values in the gaps); fm and grad_fm are columns of a [B, D + DI + 1] matrix."""
    rng = np.random.default_rng(7)
    D, DI = 8, 5
    for widths in ([8, 24], [128, 3328]):
        xs, gfm, gcat = _inputs(rng, 37, widths, with_cat)
        got = _run(xs, gfm, gcat, layout=[(0, 1), (8, 0)], fm_stride=D + DI + 1, gfm_stride=D + DI + 1)
        _check(got, xs, gfm, gcat)
        _same(got, _run(xs, gfm, gcat), "against tight aligned segments")


@pytest.mark.parametrize("with_cat", [True, False], ids=["cat", "nocat"])
def test_an_unwanted_gradient_segment_between_two_wanted_ones_is_not_written(with_cat):
    rng = np.random.default_rng(9)
    for widths in ([5, 260, 12], [8, 24, 8], [1] * 8):
        wanted = [k % 3 != 1 for k in range(len(widths))]
        xs, gfm, gcat = _inputs(rng, 37, widths, with_cat)
        got = _run(xs, gfm, gcat, wanted=wanted)
        assert [g is None for g in got[3]] == [not w for w in wanted]
        _check(got, xs, gfm, gcat, wanted)
    # nothing wanted at all: nothing is written
    got = _run(xs, gfm, gcat, wanted=[False] * len(widths))
    assert all(g is None for g in got[3])


def test_the_empty_batch_launches_nothing():
    xs = [np.zeros((0, 8), np.float32), np.zeros((0, 3), np.float32)]
    for gcat in (None, np.zeros((0, 11), np.float32)):
        fm, s, cat, grads = _run(xs, np.zeros((0, 1), np.float32), gcat)
        assert fm.shape == (0,) and s.shape == (0,) and all(g.shape[0] == 0 for g in grads)


def test_float_data_gives_the_same_bits_on_the_vector_and_the_scalar_path():
    """The same logical rows of ordinary floats (nothing exact here), once as aligned segments and once shifted or padded:
    the path a segment takes must not change a result bit, and a second run repeats the first."""
    rng = np.random.default_rng(13)
    tol_out, tol_grad = dr.gpu_tolerances()
    for widths in ([8, 24], [128, 3328], [260], [64, 4, 68]):
        B, N = 9, sum(widths)
        xs = [rng.standard_normal((B, w)).astype(np.float32) for w in widths]
        gfm, gcat = rng.standard_normal((B, 1)).astype(np.float32), rng.standard_normal((B, N)).astype(np.float32)
        for gc in (gcat, None):
            a = _run(xs, gfm, gc)
            _same(a, _run(xs, gfm, gc), "second run")
            _same(a, _run(xs, gfm, gc, layout=[(0, 1)] * len(widths)), "shifted")
            _same(a, _run(xs, gfm, gc, layout=[(4, 0)] + [(1, 3)] * (len(widths) - 1)), "mixed")
        # and they are the right numbers
        plain = _run(xs, gfm, None)
        e_out, e_grad = dr.fm_errors(xs, gfm, plain[0].reshape(B, 1), np.concatenate(plain[3], 1))
        print(f"{widths}: output error {e_out:.2e} (tolerance {tol_out:.2e}), gradient error {e_grad:.2e} ({tol_grad:.2e})")
        assert e_out <= tol_out and e_grad <= tol_grad
