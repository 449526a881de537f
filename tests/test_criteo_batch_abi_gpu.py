"""GPU: the Criteo batch kernel through the C ABI (include/tbe_hip.h `tbe_criteo_batch_i64` / `_i32`, csrc/criteo_batch.hip),
bit for bit against the numpy model of tests/_criteo_ref.py (which tests/test_criteo_datapipe.py ties to the reference's
recorded batches).  Every buffer stands between guard elements, outputs are prefilled with canaries, inputs are read back."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _criteo_ref as cr
from _guarded import Buf, TypedBuf
from fbgemm_gpu import _lib

pytestmark = pytest.mark.gpu

T = _lib.CRITEO_TILE_ROWS
HMAX = 2 ** 31 - 1
EXTREMES = np.array([-2 ** 31, -1, 0, 2 ** 31 - 1], dtype=np.int32)
HASH_SETS = {"none": None, "ones": [1] * 26, "max": [HMAX] * 26, "mixed": cr.HASHES}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _draw(rows, seed):
    """Raw rows of the given segment sizes; the four extreme ids stand in every column of the first and last rows."""
    arrays = cr.synthetic_arrays(rows, seed=seed)
    total = sum(rows)
    if total >= 8:
        flat = np.concatenate([s for _, s, _ in arrays])
        flat[:4], flat[-4:] = EXTREMES[:, None], EXTREMES[::-1, None]
        out, at = [], 0
        for d, s, l in arrays:
            out.append((d, flat[at:at + len(s)].copy(), l))
            at += len(s)
        arrays = out
    return arrays


class Case:
    """One call: the segments live in guarded buffers that start `base` rows before the segment (an odd base puts the
    sparse rows 8 bytes off the 16-byte grid; dense rows are 52 bytes, 4 bytes off every wider grid)."""

    def __init__(self, arrays, bases, hashes, perm):
        self.arrays, self.B = arrays, sum(len(a[0]) for a in arrays)
        self.hashes, self.perm = hashes, perm
        rng = np.random.default_rng(99)
        self.src, self.src_host = [], []
        self.segs = (_lib.CriteoSegment * max(len(arrays), 1))()
        for k, ((d, s, l), base) in enumerate(zip(arrays, bases)):
            n = len(d)
            lead = cr.synthetic_arrays([base], seed=int(rng.integers(1 << 30)))[0]  # other rows in front: never read
            host = [np.concatenate([lead[0], d]), np.concatenate([lead[1], s]), np.concatenate([lead[2], l])]
            bufs = [Buf(host[0].size, host[0]), TypedBuf(host[1].size, np.int32, host[1]),
                    TypedBuf(host[2].size, np.int32, host[2])]
            self.src.append(bufs)
            self.src_host.append(host)
            sg = self.segs[k]
            sg.dense, sg.sparse, sg.labels = bufs[0].ptr + 52 * base, bufs[1].ptr + 104 * base, bufs[2].ptr + 4 * base
            sg.rows = n
            if n == 0:  # an empty segment's pointers must never be looked at
                sg.dense, sg.sparse, sg.labels = None, 8, 1
        self.hash_buf = TypedBuf(26, np.int32, hashes) if hashes is not None else None
        self.perm_buf = TypedBuf(self.B, np.int64, perm) if perm is not None else None

    def launch(self, width, outs):
        fn = _lib.load().tbe_criteo_batch_i64 if width == np.int64 else _lib.load().tbe_criteo_batch_i32
        rc = fn(self.segs, len(self.arrays), self.B, self.hash_buf.ptr if self.hash_buf else None,
                self.perm_buf.ptr if self.perm_buf else None, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, _stream())
        _lib.check(rc, "tbe_criteo_batch")

    def outputs(self, width):
        return [Buf(self.B * 13), TypedBuf(26 * self.B, width), TypedBuf(self.B, np.int32), TypedBuf(1, np.int32, [0])]

    def run(self, width):
        outs = self.outputs(width)
        self.launch(width, outs)
        torch.cuda.synchronize()
        return self.read(outs)

    def read(self, outs):
        got = (outs[0].get((self.B, 13)), outs[1].get(), outs[2].get(), int(outs[3].get()[0]))
        for bufs, host in zip(self.src, self.src_host):  # inputs unchanged, guards intact
            for b, h in zip(bufs, host):
                cr.assert_same_bits(b.get(), h.reshape(-1), "input read back")
        if self.hash_buf:
            cr.assert_same_bits(self.hash_buf.get(), np.asarray(self.hashes, dtype=np.int32), "hashes read back")
        if self.perm_buf:
            cr.assert_same_bits(self.perm_buf.get(), np.asarray(self.perm, dtype=np.int64), "perm read back")
        return got

    def expected(self, width):
        return cr.batch_ref(self.arrays, self.B, self.hashes, self.perm, width)

    def check(self, what):
        want64 = self.expected(np.int64)
        got64 = self.run(np.int64)
        cr.assert_batch_equal(got64, want64, what + " i64")
        got32 = self.run(np.int32)
        cr.assert_batch_equal(got32, self.expected(np.int32), what + " i32")
        cr.assert_same_bits(got32[1], got64[1].astype(np.int32), what + " i32 is i64 narrowed")
        assert np.array_equal(got32[1].astype(np.int64), got64[1])
        return got64


def _perm(kind, B, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "none":
        return None
    if kind == "identity":
        return np.arange(B, dtype=np.int64)
    if kind == "reversal":
        return np.arange(B, dtype=np.int64)[::-1].copy()
    if kind == "random":
        return rng.permutation(B).astype(np.int64)
    if kind == "repeats":
        return rng.integers(0, B, size=B, dtype=np.int64)
    raise KeyError(kind)


@pytest.mark.parametrize("B", [1, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("perm", ["none", "random"])
def test_batch_sizes_around_the_tile(B, perm):
    Case(_draw([B], seed=B), [0], cr.HASHES, _perm(perm, B, seed=B)).check(f"B={B} perm={perm}")


@pytest.mark.parametrize("width", [np.int64, np.int32])
def test_the_empty_batch_launches_nothing(width):
    c = Case([], [], cr.HASHES, None)
    outs = c.outputs(width)
    c.launch(width, outs)
    torch.cuda.synchronize()
    assert c.read(outs)[3] == 0  # guards intact, counter untouched
    c = Case(_draw([0, 0], seed=1), [0, 1], None, None)
    outs = c.outputs(width)
    c.launch(width, outs)
    torch.cuda.synchronize()
    c.read(outs)


SEGMENTS = {
    "one": [2 * T + 3],
    "two": [70, 61],
    "three_with_a_row_of_one": [10, 1, 120],
    "eight": [5, 17, 1, 40, 3, 30, 20, 15],
    "empty_first": [0, 2 * T + 3],
    "empty_middle": [T, 0, T + 3],
    "empty_last": [2 * T + 3, 0],
    "empty_everywhere": [0, 0, 3, 0, 0, 60, 0, 0],
    "boundary_on_the_tile_edge": [T, T + 3],
    "boundary_one_row_before": [T - 1, T + 4],
    "boundary_one_row_after": [T + 1, T + 2],
    "every_row_its_own_segment": [1] * 8,
}


@pytest.mark.parametrize("name", list(SEGMENTS))
@pytest.mark.parametrize("perm", ["none", "random"])
def test_segmentation_changes_no_bit(name, perm):
    rows = SEGMENTS[name]
    B = sum(rows)
    flat = _draw([B], seed=7)[0]
    whole = Case([flat], [0], cr.HASHES, _perm(perm, B, seed=3)).run(np.int64)
    arrays, at = [], 0
    for n in rows:
        arrays.append(tuple(a[at:at + n] for a in flat))
        at += n
    for bases in ([k % 2 for k in range(len(rows))], [(k + 1) % 2 + 2 for k in range(len(rows))]):  # even / odd source rows
        got = Case(arrays, bases, cr.HASHES, _perm(perm, B, seed=3)).check(f"{name} bases={bases}")
        cr.assert_batch_equal(got, whole, f"{name}: segmented equals unsegmented")


@pytest.mark.parametrize("base", [0, 1, 2, 3])
def test_source_alignment_changes_no_bit(base):
    """base even: the sparse range starts on the 16-byte grid; odd: 8 bytes off it.  Dense moves by 52 bytes per row."""
    B = T + 5
    c = Case(_draw([B], seed=11), [base], cr.HASHES, _perm("random", B, seed=base))
    assert (c.segs[0].sparse % 16 == 0) == (base % 2 == 0) and (c.segs[0].dense % 16 == 0) == (base % 4 == 0)
    c.check(f"base={base}")


@pytest.mark.parametrize("hashes", list(HASH_SETS))
def test_hash_sets_and_extreme_ids(hashes):
    B = 2 * T + 3
    arrays = _draw([T, 1, T + 2], seed=5)
    assert np.array_equal(arrays[0][1][:4, 0], EXTREMES) and np.array_equal(arrays[2][1][-4:, 25], EXTREMES[::-1])
    c = Case(arrays, [1, 0, 3], HASH_SETS[hashes], _perm("reversal", B))
    got = c.check(hashes)
    values = got[1].reshape(26, B)
    if hashes == "none":  # sign-extended
        assert values[:, B - 1].tolist() == [-2 ** 31] * 26 and values[:, 0].tolist() == [-2 ** 31] * 26
        assert values[:, B - 2].tolist() == [-1] * 26
    if hashes == "ones":
        assert not values.any()
    if hashes == "max":  # rows B-1 .. B-4 of the output are source rows 0 .. 3
        assert values[:, B - 1].tolist() == [HMAX - 1] * 26 and values[:, B - 2].tolist() == [HMAX - 1] * 26
        assert values[:, B - 3].tolist() == [0] * 26 and values[:, B - 4].tolist() == [0] * 26
    if hashes != "none":
        assert values.min() >= 0 and (values < np.asarray(HASH_SETS[hashes], dtype=np.int64)[:, None]).all()


@pytest.mark.parametrize("kind", ["none", "identity", "reversal", "random", "repeats"])
def test_permutations(kind):
    B = 2 * T + 3
    arrays = _draw([T + 1, T + 2], seed=13)
    got = Case(arrays, [1, 2], cr.HASHES, _perm(kind, B, seed=2)).check(kind)
    assert got[3] == 0
    if kind == "identity":
        cr.assert_batch_equal(got, Case(arrays, [1, 2], cr.HASHES, None).run(np.int64), "identity equals no perm")


def test_bad_permutation_entries_are_zero_rows_and_counted_exactly():
    B = 2 * T + 3
    perm = _perm("random", B, seed=4)
    bad = {0: -1, 1: B, T - 1: 2 ** 40, T: -2 ** 63, B - 1: B + 1, 77: 2 ** 63 - 1, 78: -B}
    for j, v in bad.items():
        perm[j] = v
    got = Case(_draw([T, T + 3], seed=17), [1, 0], cr.HASHES, perm).check("bad perm")
    assert got[3] == len(bad)
    values = got[1].reshape(26, B)
    for j in bad:
        assert not got[0][j].any() and not values[:, j].any() and got[2][j] == 0
    assert got[0][2].any() and values[:, 2].any()  # the neighbours are real rows


def test_two_runs_give_the_same_bits():
    B = 2 * T + 3
    c = Case(_draw([60, 71], seed=19), [1, 1], cr.HASHES, _perm("repeats", B, seed=6))
    for width in (np.int64, np.int32):
        cr.assert_batch_equal(c.run(width), c.run(width), "run twice")


def test_graph_capture_and_replay_after_the_inputs_changed_in_place():
    B = 2 * T + 3
    rows, bases = [T - 1, 1, T + 3], [1, 0, 2]
    c = Case(_draw(rows, seed=23), bases, cr.HASHES, _perm("random", B, seed=8))
    eager = c.run(np.int64)
    outs = c.outputs(np.int64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.launch(np.int64, outs)  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.launch(np.int64, outs)
    fresh = c.outputs(np.int64)  # poison what the warm-up wrote
    for o, f in zip(outs, fresh):
        o.t.copy_(f.t)
    graph.replay()
    torch.cuda.synchronize()
    cr.assert_batch_equal(c.read(outs), eager, "replay")
    # new rows, new hashes and a new permutation, written into the same buffers
    new = _draw(rows, seed=29)
    new_hashes = [h + 1 if h < HMAX else 5 for h in cr.HASHES]
    new_perm = _perm("repeats", B, seed=9)
    for k, (parts, base) in enumerate(zip(new, bases)):
        for i in range(3):  # dense, sparse, labels: the rows in front of the segment stay
            b = c.src[k][i]
            c.src_host[k][i] = np.concatenate([c.src_host[k][i][:base], parts[i]])
            g = (b.t.numel() - b.n) // 2
            b.t[g:g + b.n].copy_(torch.from_numpy(c.src_host[k][i].reshape(-1).copy()))
    c.arrays, c.hashes, c.perm = new, new_hashes, new_perm
    g = c.hash_buf.guard
    c.hash_buf.t[g:g + 26].copy_(torch.tensor(new_hashes, dtype=torch.int32))
    g = c.perm_buf.guard
    c.perm_buf.t[g:g + B].copy_(torch.from_numpy(new_perm))
    for o, f in zip(outs, fresh):
        o.t.copy_(f.t)
    graph.replay()
    torch.cuda.synchronize()
    cr.assert_batch_equal(c.read(outs), c.expected(np.int64), "replay after the inputs changed")
