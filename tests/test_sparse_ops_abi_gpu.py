"""GPU: the KJT index ops and pooled layout copies (csrc/sparse_ops.hip, csrc/pooled_exchange.hip) through the C ABI of
include/tbe_hip.h, bit for bit against oracle/tbe_oracle.c at every wave, block, tile and dispatch edge of the kernels.

Every buffer sits between guard elements (tests/_guarded.py) and is exactly as large as the entry may use; an output starts
as its type's canary, so whatever a call must leave alone is checked too, and every guard is checked after every call."""
import ctypes

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _vb_ref
from _guarded import CANARY, Buf, TypedBuf
from fbgemm_gpu import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
INT_OF = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}  # the element types of _guarded.INT_CANARY, by size


def _done(lib, rc):
    assert rc == OK, lib.tbe_last_error()
    torch.cuda.synchronize()


def _in(a, dtype=None):
    """An input array on the device between guards; `same()` checks guards and contents after the calls."""
    a = np.ascontiguousarray(a, dtype=dtype)
    buf = Buf(a.size, a) if a.dtype == np.float32 else TypedBuf(a.size, a.dtype, a)
    buf.same = lambda: np.testing.assert_array_equal(buf.get(), a.reshape(-1))
    return buf


def _offsets(lengths):
    return oracle.cumsum(np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1), 0)


# ---- gathered scan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldt", [np.int32, np.int64])
@pytest.mark.parametrize("T_out,B", [(0, 5), (1, 1), (1, 2048), (2, 1024), (1, 2049), (3, 683)])
def test_permute_2d_lengths_tile_edges(T_out, B, ldt):
    """T_out * B = 0, 1, 2048 (one scan tile), 2049 (tile edge inside a feature and across one); a permute that repeats
    one row of three and omits another.  in_offsets, out_offsets and out_lengths against the oracle."""
    lib = _lib.load()
    T_in = 3
    rng = np.random.default_rng(T_out * 10000 + B)
    lengths = rng.integers(0, 5, size=(T_in, B)).astype(ldt)
    perm = np.array([2, 0, 2][:T_out], dtype=np.int32)
    want_l, _, _ = oracle.permute_2d(perm, lengths, np.zeros(int(lengths.sum()), np.int64))
    d_perm, d_len = _in(perm), _in(lengths)
    out_l = TypedBuf(T_out * B, ldt)
    in_off, out_off = TypedBuf(T_in * B + 1, np.int64), TypedBuf(T_out * B + 1, np.int64)
    ws = TypedBuf(lib.tbe_permute_2d_workspace_bytes(T_in, T_out, B), np.uint8)
    _done(lib, lib.tbe_permute_2d_lengths(d_perm.ptr, T_in, T_out, B, d_len.ptr, lengths.itemsize, out_l.ptr, in_off.ptr,
                                          out_off.ptr, ws.ptr, ws.n, None))
    np.testing.assert_array_equal(out_l.get((T_out, B)), want_l)
    np.testing.assert_array_equal(in_off.get(), _offsets(lengths))
    np.testing.assert_array_equal(out_off.get(), _offsets(want_l))
    ws.get(), d_perm.same(), d_len.same()


# ---- permute data ----------------------------------------------------------------------------------------------------
def _permute_case(T_in, T_out, B, seed):
    """perm [T_out] over T_in rows (rows repeat and are left out once T_out > 2) and lengths [T_in, B] such that, of the
    T_out * B OUTPUT segments: the first and last of every wave of 64 are empty, the whole third group of 64 is empty, and one
    holds 200 elements (four 64-lane chunks); the rest hold 0..3."""
    rng = np.random.default_rng(seed)
    perm = rng.integers(0, T_in, size=T_out).astype(np.int32) if T_out > 2 else rng.permutation(T_in)[:T_out].astype(np.int32)
    nseg = T_out * B
    src = (perm.astype(np.int64)[:, None] * B + np.arange(B)[None, :]).reshape(-1)  # input segment of each output segment
    lengths = rng.integers(0, 4, size=T_in * B)
    empty = sorted({o for o in list(range(0, nseg, 64)) + list(range(63, nseg, 64)) + [nseg - 1] + list(range(128, 192))
                    if o < nseg and nseg > 1})
    lengths[src[empty]] = 0
    free = [o for o in range(nseg) if src[o] not in set(src[empty])]
    lengths[src[free[len(free) // 2] if free else 0]] = 200
    return perm, lengths.reshape(T_in, B)


def _check_permute_data(lib, perm, lengths, vdt, wdt, one_d):
    T_in, B = lengths.shape
    T_out, N = perm.size, int(lengths.sum())
    rng = np.random.default_rng(N)
    values = rng.integers(0, 100, size=N).astype(vdt)
    weights = rng.integers(0, 100, size=N).astype(wdt) if wdt is not None else None
    want_l, want_v, want_w = oracle.permute_2d(perm, lengths, values, weights)
    total = int(want_l.sum())
    d_perm, d_in, d_out = _in(perm), _in(_offsets(lengths)), _in(_offsets(want_l))
    d_val, d_w = _in(values), (_in(weights) if weights is not None else None)
    out_v = TypedBuf(total, vdt)
    out_w = TypedBuf(total, wdt) if weights is not None else None
    wp, owp, we = (d_w.ptr, out_w.ptr, weights.itemsize) if weights is not None else (None, None, 0)
    if one_d:
        rc = lib.tbe_permute_1d_data(d_perm.ptr, T_out, d_in.ptr, d_out.ptr, d_val.ptr, out_v.ptr, values.itemsize, wp, owp, we, None)
    else:
        rc = lib.tbe_permute_2d_data(d_perm.ptr, T_out, B, d_in.ptr, d_out.ptr, d_val.ptr, out_v.ptr, values.itemsize, wp, owp,
                                     we, None)
    _done(lib, rc)
    np.testing.assert_array_equal(out_v.get(), want_v)
    if weights is not None:
        np.testing.assert_array_equal(out_w.get(), want_w)
        d_w.same()
    d_perm.same(), d_in.same(), d_out.same(), d_val.same()


@pytest.mark.parametrize("T_out,B", [(1, 1), (3, 21), (2, 32), (5, 13), (5, 51), (4, 64), (257, 1)])
def test_permute_data_wave_and_block_edges(T_out, B):
    """1, 63, 64, 65, 255, 256 and 257 output segments (a wave serves 64, a block 4 waves) through tbe_permute_2d_data, and the
    same count of segments through tbe_permute_1d_data; empty segments at the wave edges, an empty group, a 200-element
    segment."""
    lib = _lib.load()
    perm, lengths = _permute_case(T_out + 1, T_out, B, T_out * 1000 + B)
    _check_permute_data(lib, perm, lengths, np.int64, np.int32, one_d=False)
    perm, lengths = _permute_case(T_out * B + 3, T_out * B, 1, T_out * 1000 + B + 1)
    _check_permute_data(lib, perm, lengths, np.int64, None, one_d=True)


@pytest.mark.parametrize("vsize,wsize", [(1, None), (2, None), (4, None), (8, None), (8, 1), (8, 2), (8, 4), (8, 8), (4, 8)])
def test_permute_data_every_element_size(vsize, wsize):
    """Values of 1 / 2 / 4 / 8 bytes, and weights absent or of 1 / 2 / 4 / 8 bytes, at 130 segments (two full waves and a part)."""
    perm, lengths = _permute_case(6, 5, 26, 7)
    _check_permute_data(_lib.load(), perm, lengths, INT_OF[vsize], INT_OF[wsize] if wsize else None, one_d=False)


# ---- expand_into_jagged_permute --------------------------------------------------------------------------------------
def _check_expand(lib, perm, in_len, out_len, dt, output_size=None, ref_perm=None):
    """One call; the expectation is _vb_ref's at the full output size, cut to `output_size` (the kernel's clamp), with
    `ref_perm` in place of a permute the reference cannot index."""
    in_off, out_off = _offsets(in_len).astype(dt), _offsets(out_len).astype(dt)
    full = int(out_off[-1])
    size = full if output_size is None else output_size
    want = _vb_ref.expand_into_jagged_permute((perm if ref_perm is None else ref_perm).astype(dt), in_off, out_off, full)[:size]
    d_perm, d_in, d_out = _in(perm, dt), _in(in_off), _in(out_off)
    out = TypedBuf(size, dt)
    _done(lib, lib.tbe_expand_into_jagged_permute(d_perm.ptr, d_in.ptr, d_out.ptr, perm.size, size, np.dtype(dt).itemsize,
                                                  out.ptr, None))
    np.testing.assert_array_equal(out.get(), want)
    d_perm.same(), d_in.same(), d_out.same()


@pytest.mark.parametrize("dt", [np.int32, np.int64])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_expand_wave_edges(P, dt):
    rng = np.random.default_rng(P)
    perm = rng.permutation(P)
    in_len = rng.integers(0, 6, size=P)
    _check_expand(_lib.load(), perm, in_len, in_len[perm], dt)


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_expand_splits_clamp_and_bad_permute(dt):
    """A 70 000-element segment among empty ones (its range is dealt to 69 waves); output_size below output_offset[P] (the
    stores stop at output_size); a permute entry outside [0, P) (its segment counts up from input offset 0)."""
    lib = _lib.load()
    perm = np.array([4, 2, 0, 1, 3])
    in_len = np.array([0, 0, 70000, 0, 0])
    _check_expand(lib, perm, in_len, in_len[perm], dt)
    rng = np.random.default_rng(5)
    perm, in_len = rng.permutation(70), rng.integers(1, 6, size=70)
    full = int(in_len.sum())
    for size in (full - 1, full - 67, 3):
        _check_expand(lib, perm, in_len, in_len[perm], dt, output_size=size)
    bad, ref = perm.copy(), perm.copy()
    bad[[3, 66]], ref[[3, 66]] = [70, -1], [0, 0]  # input_offset[0] == 0
    _check_expand(lib, bad, in_len, in_len[perm], dt, ref_perm=ref)


# ---- block bucketize -------------------------------------------------------------------------------------------------
def _bucketize_input(F, B, ldt, idt):
    """The same input whatever my_size is: bags of 0..4 ids (some empty), block sizes 7, 11, 13, ids below 36 blocks, among
    them multiples of the block size, 32 and 33 blocks exactly (the first id my_size = 32 / 33 drops) and 35 blocks."""
    rng = np.random.default_rng(F * 1000 + B)
    lengths = rng.integers(0, 5, size=F * B).astype(ldt)
    lengths[::7] = 0
    N = int(lengths.sum())
    blocks = np.array([7, 11, 13][:F], dtype=idt)
    blk_of = blocks[np.repeat(np.arange(F), B).repeat(lengths)].astype(np.int64)
    ids = rng.integers(0, 36, size=N) * blk_of + rng.integers(0, 2, size=N) * rng.integers(0, 7, size=N)
    for k, mult in enumerate((32, 33, 1, 0, 35)):
        if k < N:
            ids[k * (N // 5)] = mult * blk_of[k * (N // 5)]
    return lengths, ids.astype(idt), blocks, rng.random(N).astype(np.float32)


def _check_bucketize(lib, lengths, ids, blocks, weights, my_size, with_w=True, pos=True, seq=True):
    L, N, F = lengths.size, ids.size, blocks.size
    idt = ids.dtype
    want = oracle.block_bucketize(lengths, ids, blocks, my_size, weights if with_w else None, pos, seq)
    kept = int(want[0].sum())
    d_len, d_ids, d_blk, d_w = _in(lengths), _in(ids), _in(blocks), _in(weights)
    new_l = TypedBuf(L * my_size, lengths.dtype)
    new_i, new_w, new_p, unb = TypedBuf(N, idt), Buf(N), TypedBuf(N, idt), TypedBuf(N, idt)
    ws = TypedBuf(lib.tbe_bucketize_workspace_bytes(L, my_size), np.uint8)
    _done(lib, lib.tbe_block_bucketize(d_len.ptr, lengths.itemsize, L, d_ids.ptr, ids.itemsize, N, d_blk.ptr, F, my_size,
                                       d_w.ptr if with_w else None, int(pos), int(seq), new_l.ptr, new_i.ptr,
                                       new_w.ptr if with_w else None, new_p.ptr if pos else None,
                                       unb.ptr if seq else None, ws.ptr, ws.n, None))
    np.testing.assert_array_equal(new_l.get(), want[0])
    # only the ids that were kept are written: the tail still holds the sentinel, and so does an output that was not asked for
    for buf, exp, on in ((new_i, want[1], True), (new_w, want[2], with_w), (new_p, want[3], pos)):
        got, canary = buf.get(), (CANARY if buf is new_w else buf.canary)
        n = kept if on else 0
        if on:
            np.testing.assert_array_equal(got[:n], exp[:n])
        assert (got[n:] == canary).all()
    if seq:
        np.testing.assert_array_equal(unb.get(), want[4])  # -1 for a dropped id
    else:
        assert (unb.get() == unb.canary).all()
    ws.get(), d_len.same(), d_ids.same(), d_blk.same(), d_w.same()
    return kept


@pytest.mark.parametrize("my_size", [1, 32, 33])
@pytest.mark.parametrize("F,B", [(1, 1), (1, 255), (1, 256), (1, 257), (3, 86)])
def test_bucketize_block_edges_and_both_counter_homes(F, B, my_size):
    """lengths_size 1, 255, 256, 257 and 3 x 86 (a thread per bag, 256 a block); my_size 32 keeps the counters in LDS, 33
    in global memory, on the same input; ids on block boundaries and ids that are dropped."""
    lengths, ids, blocks, weights = _bucketize_input(F, B, np.int32, np.int64)
    kept = _check_bucketize(_lib.load(), lengths, ids, blocks, weights, my_size)
    assert kept < ids.size or ids.size < 5  # some id was dropped


@pytest.mark.parametrize("my_size", [32, 33])
def test_bucketize_every_type_pair_and_option(my_size):
    lib = _lib.load()
    for ldt in (np.int32, np.int64):
        for idt in (np.int32, np.int64):
            _check_bucketize(lib, *_bucketize_input(3, 86, ldt, idt), my_size)
    case = _bucketize_input(3, 86, np.int32, np.int64)
    for with_w in (False, True):
        for pos in (False, True):
            for seq in (False, True):
                _check_bucketize(lib, *case, my_size, with_w=with_w, pos=pos, seq=seq)


# ---- pooled all-to-all layout copies ---------------------------------------------------------------------------------
A2A_DIMS = {  # per W: every width a multiple of 4 with a width-4 slab | widths that are not
    1: ([4], [5]),
    2: ([4, 12], [3, 6]),
    8: ([4, 8, 128, 4, 16, 20, 4, 12], [3, 5, 4, 7, 1, 2, 9, 6]),
}


def _check_a2a(lib, dims, Bl, flag, shift=0):
    """pack at scale 0.5 against the oracle, unpack at 2.0 back to the input exactly.  `shift`: floats by which the slab
    buffer is moved off its 16-byte address."""
    W, D = len(dims), sum(dims)
    grad = np.random.default_rng(D * 100 + Bl).standard_normal((Bl, D)).astype(np.float32)
    d_dims, d_grad = _in(np.array(dims, dtype=np.int32)), _in(grad)
    send, out = Buf(Bl * D + shift), Buf(Bl * D)
    _done(lib, lib.tbe_a2a_pooled_pack(d_grad.ptr, send.ptr + 4 * shift, d_dims.ptr, W, Bl, D, flag, 0.5, None))
    got = send.get()
    assert (got[:shift] == CANARY).all()
    np.testing.assert_array_equal(got[shift:], oracle.a2a_pooled_pack(grad, dims, 0.5))
    _done(lib, lib.tbe_a2a_pooled_unpack(send.ptr + 4 * shift, out.ptr, d_dims.ptr, W, Bl, D, flag, 2.0, None))
    np.testing.assert_array_equal(out.get((Bl, D)), grad)
    np.testing.assert_array_equal(out.get((Bl, D)), oracle.a2a_pooled_unpack(got[shift:], dims, Bl, 2.0))
    send.get(), d_dims.same(), d_grad.same()


@pytest.mark.parametrize("Bl", [1, 33])
@pytest.mark.parametrize("W", [1, 2, 8])
def test_a2a_pooled_layout_vector_and_scalar_paths(W, Bl):
    lib = _lib.load()
    by4, odd = A2A_DIMS[W]
    _check_a2a(lib, by4, Bl, 1)
    _check_a2a(lib, by4, Bl, 0)  # the caller does not vouch for the widths: scalar path, same result
    _check_a2a(lib, odd, Bl, 0)
    _check_a2a(lib, by4, Bl, 1, shift=1)  # widths allow vectors, the address does not: scalar path, same result


# ---- offsets_range, jagged <-> dense ---------------------------------------------------------------------------------
JAGGED_LENGTHS = [[5], [0, 0, 3, 0, 0, 2, 4, 0]]  # B = 1; empty bags first, in the middle (equal offsets in a row) and last


@pytest.mark.parametrize("lengths", JAGGED_LENGTHS, ids=["one-bag", "empty-bags"])
def test_offsets_range_picks_the_last_of_equal_offsets(lengths):
    lib = _lib.load()
    starts = _offsets(lengths)[:-1]
    N = int(np.sum(lengths))
    d_off, out = _in(starts), TypedBuf(N, np.int64)
    _done(lib, lib.tbe_offsets_range(d_off.ptr, starts.size, N, out.ptr, None))
    np.testing.assert_array_equal(out.get(), oracle.offsets_range(starts, N))
    d_off.same()


@pytest.mark.parametrize("lengths", JAGGED_LENGTHS, ids=["one-bag", "empty-bags"])
def test_jagged_dense_pair_below_at_and_above_the_longest_bag(lengths):
    """tbe_jagged_2d_to_dense_f32 against the oracle; tbe_dense_to_jagged_2d_f32 against the oracle's own row placement:
    the oracle's dense image of the row numbers 1 .. N says which (bag, position) each row went to, 0 = padding."""
    lib = _lib.load()
    offsets = _offsets(lengths)
    B, N, D = len(lengths), int(offsets[-1]), 3
    rng = np.random.default_rng(B)
    values = rng.standard_normal((N, D)).astype(np.float32)
    d_val, d_off = _in(values), _in(offsets)
    for max_L in (max(lengths) - 2, max(lengths), max(lengths) + 2):
        dense = Buf(B * max_L * D)
        _done(lib, lib.tbe_jagged_2d_to_dense_f32(d_val.ptr, d_off.ptr, B, D, max_L, dense.ptr, None))
        np.testing.assert_array_equal(dense.get((B, max_L, D)), oracle.jagged_2d_to_dense(values, offsets, max_L))
        grad = rng.standard_normal((B, max_L, D)).astype(np.float32)
        row_at = oracle.jagged_2d_to_dense(np.arange(1, N + 1, dtype=np.float32)[:, None], offsets, max_L)[:, :, 0]
        want = np.zeros((N, D), dtype=np.float32)  # a row past max_L gets a zero gradient
        want[row_at[row_at > 0].astype(np.int64) - 1] = grad[row_at > 0]
        d_grad, out = _in(grad), Buf(N * D)
        _done(lib, lib.tbe_dense_to_jagged_2d_f32(d_grad.ptr, d_off.ptr, B, D, max_L, N, out.ptr, None))
        np.testing.assert_array_equal(out.get((N, D)), want)
        d_grad.same()
    d_val.same(), d_off.same()


# ---- argument errors -------------------------------------------------------------------------------------------------
def test_one_bad_argument_per_entry_is_refused_before_any_byte_moves():
    lib = _lib.load()
    i32 = TypedBuf(64, np.int32, np.arange(64))
    i64 = TypedBuf(64, np.int64, np.arange(64))
    f32 = Buf(64, np.arange(64))
    o32, o64, of32, ws = TypedBuf(64, np.int32), TypedBuf(64, np.int64), Buf(64), TypedBuf(4096, np.uint8)
    before = [b.all().copy() for b in (i32, i64, f32, o32, o64, of32, ws)]
    two31 = ctypes.c_int64(1 << 31)
    exchange = (i32.ptr, i32.ptr, i32.ptr, i64.ptr, i32.ptr, 0, 2, 4, 8, 1, 1.0, None)  # Fg = 0
    calls = [
        ("tbe_cumsum: elem_size 2", lib.tbe_cumsum, (i32.ptr, o32.ptr, 8, 2, 0, ws.ptr, ws.n, None)),
        ("tbe_permute_2d_lengths: len_elem_size 2",
         lib.tbe_permute_2d_lengths, (i32.ptr, 2, 2, 4, i32.ptr, 2, o32.ptr, o64.ptr, o64.ptr, ws.ptr, ws.n, None)),
        ("tbe_permute_2d_data: val_elem_size 3",
         lib.tbe_permute_2d_data, (i32.ptr, 2, 4, i64.ptr, i64.ptr, i32.ptr, o32.ptr, 3, None, None, 4, None)),
        ("tbe_permute_1d_lengths: L=-1 / P=2 outside [0, 2^31)",
         lib.tbe_permute_1d_lengths, (i32.ptr, -1, 2, i32.ptr, 4, o32.ptr, o64.ptr, o64.ptr, ws.ptr, ws.n, None)),
        ("tbe_permute_1d_data: P=2147483648 outside [0, 2^31)",
         lib.tbe_permute_1d_data, (i32.ptr, two31, i64.ptr, i64.ptr, i32.ptr, o32.ptr, 4, None, None, 4, None)),
        ("tbe_expand_into_jagged_permute: elem_size 2",
         lib.tbe_expand_into_jagged_permute, (i32.ptr, i32.ptr, i32.ptr, 4, 8, 2, o32.ptr, None)),
        ("tbe_block_bucketize: lengths_size 5 not a multiple of F=2",
         lib.tbe_block_bucketize, (i32.ptr, 4, 5, i64.ptr, 8, 8, i64.ptr, 2, 4, None, 0, 0, o32.ptr, o64.ptr, None, None, None,
                                   ws.ptr, ws.n, None)),
        ("tbe_a2a_pooled_unpack: bad sizes", lib.tbe_a2a_pooled_unpack, (f32.ptr, of32.ptr, i32.ptr, 0, 4, 8, 1, 1.0, None)),
        ("tbe_a2a_pooled_pack: bad sizes", lib.tbe_a2a_pooled_pack, (f32.ptr, of32.ptr, i32.ptr, 0, 4, 8, 1, 1.0, None)),
        ("tbe_pooled_exchange_unpack: bad sizes", lib.tbe_pooled_exchange_unpack, (f32.ptr, of32.ptr) + exchange),
        ("tbe_pooled_exchange_pack: bad sizes", lib.tbe_pooled_exchange_pack, (f32.ptr, of32.ptr) + exchange),
        ("tbe_jagged_2d_to_dense_f32: bad sizes", lib.tbe_jagged_2d_to_dense_f32, (f32.ptr, i64.ptr, -1, 2, 2, of32.ptr, None)),
        ("tbe_dense_to_jagged_2d_f32: null pointer",
         lib.tbe_dense_to_jagged_2d_f32, (f32.ptr, i64.ptr, 0, 2, 2, 4, of32.ptr, None)),
        ("tbe_offsets_range: null pointer / empty offsets", lib.tbe_offsets_range, (i64.ptr, 0, 8, o64.ptr, None)),
        ("tbe_copy_rows: bad sizes", lib.tbe_copy_rows, (i32.ptr, 4, i32.ptr, 2, -16, o32.ptr, None)),
    ]
    for text, fn, args in calls:
        assert fn(*args) == INVALID, text
        assert lib.tbe_last_error().decode() == text
    torch.cuda.synchronize()
    for b, was in zip((i32, i64, f32, o32, o64, of32, ws), before):
        np.testing.assert_array_equal(b.all(), was)
