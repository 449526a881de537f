"""Shared by the Criteo datapipe tests and tests/golden/make_criteo_golden.py: the synthetic day files (drawn from a seed,
never stored), a numpy model of the batch kernel (include/tbe_hip.h `tbe_criteo_batch_*`), the segment arithmetic of a
rank's batches written independently of the datapipe, and the bit-for-bit comparison every test uses.  Everything is a copy
or an integer operation, so there is no tolerance anywhere."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criteo_datapipe.npz")
SEED = 20260117
ROWS = [37, 5, 300]  # batch 16: the third batch spans all three files
ROWS_MANY = [3, 2, 1, 2, 3, 1, 2, 1, 2, 300]  # batch 16: the first batch has 9 pieces, more than the kernel's 8 segments
BATCH = 16
HASHES = [1, 2, 3, 7, 40_000_000, 2 ** 31 - 1] + list(range(1000, 1020))
WORLDS = [(1, 0), (2, 0), (2, 1), (3, 2)]  # (world_size, rank)
SHUFFLE_SEED = 5
N_DENSE, N_CAT = 13, 26


def synthetic_arrays(rows=ROWS, seed=SEED):
    """[(dense [n, 13] float32, sparse [n, 26] int32, labels [n, 1] int32)] per file.  Ids cover the whole int32 range,
    negatives included (real Criteo ids are hex values stored as int32); dense values are multiples of 1/64."""
    rng = np.random.default_rng(seed)
    out = []
    for n in rows:
        dense = (rng.integers(-64, 4096, size=(n, N_DENSE)) / 64).astype(np.float32)  # exact: no libm in the draw
        sparse = rng.integers(-2 ** 31, 2 ** 31, size=(n, N_CAT), dtype=np.int64).astype(np.int32)
        labels = rng.integers(0, 2, size=(n, 1), dtype=np.int64).astype(np.int32)
        out.append((dense, sparse, labels))
    return out


def checksum(arrays):
    """Pins the draw: [sum of ids, sum of ids * (column + 1), sum of dense bit patterns, sum of labels] as int64."""
    w = np.arange(1, N_CAT + 1, dtype=np.int64)
    return np.array([sum(int(s.astype(np.int64).sum()) for _, s, _ in arrays),
                     sum(int((s.astype(np.int64) * w).sum()) for _, s, _ in arrays),
                     sum(int(d.view(np.uint32).astype(np.int64).sum()) for d, _, _ in arrays),
                     sum(int(l.sum()) for _, _, l in arrays)], dtype=np.int64)


def write_files(directory, arrays, day0=0):
    """Writes day_<i>_{dense,sparse,labels}.npy; returns the three path lists."""
    paths = ([], [], [])
    for i, parts in enumerate(arrays):
        for kind, lst, a in zip(("dense", "sparse", "labels"), paths, parts):
            p = os.path.join(str(directory), f"day_{day0 + i}_{kind}.npy")
            np.save(p, a)
            lst.append(p)
    return paths


def rank_segments(rows, rank, world_size, batch):
    """Per batch of `rank`, its pieces (file, first row, rows): the rank owns rows [rank * q, (rank + 1) * q) of the files'
    concatenation, q = total // world_size, and batch b the next `batch` of them; the last partial batch is dropped."""
    q = sum(rows) // world_size
    starts = np.concatenate([[0], np.cumsum(rows)])
    out = []
    for b in range(q // batch):
        lo, hi = rank * q + b * batch, rank * q + (b + 1) * batch
        segs = []
        for f, n in enumerate(rows):
            a, z = max(lo, int(starts[f])), min(hi, int(starts[f]) + n)
            if a < z:
                segs.append((f, a - int(starts[f]), z - a))
        out.append(segs)
    return out


def floormod_i32(v, h):
    """numpy's floor modulo the way the kernel computes it: C's truncated remainder in int32, plus h when negative."""
    v, h = np.asarray(v, dtype=np.int32), np.asarray(h, dtype=np.int32)
    r = (np.abs(v.astype(np.int64)) % h.astype(np.int64)) * np.sign(v.astype(np.int64))  # C's v % h
    r = np.where(r < 0, r + h, r)
    return r.astype(np.int32)


def batch_ref(segments, B, hashes=None, perm=None, values_dtype=np.int64, fault=None):
    """The kernel's contract in numpy.  segments: [(dense [n, 13], sparse [n, 26], labels [n, 1])], empty ones allowed.
    Returns dense_out [B, 13], values_out [26 * B], labels_out [B], bad_perm.  `fault` injects one of FAULTS (the tests of
    the comparison itself)."""
    live = [s for s in segments if len(s[0])]
    dense = np.concatenate([s[0] for s in live]) if live else np.zeros((0, N_DENSE), np.float32)
    sparse = np.concatenate([s[1] for s in live]) if live else np.zeros((0, N_CAT), np.int32)
    labels = np.concatenate([s[2] for s in live]) if live else np.zeros((0, 1), np.int32)
    if fault == "segment_off_by_one" and len(live) > 1:
        n0 = len(live[0][0])  # the first boundary one row late: row n0 repeats row n0 - 1
        dense, sparse, labels = dense.copy(), sparse.copy(), labels.copy()
        dense[n0], sparse[n0], labels[n0] = dense[n0 - 1], sparse[n0 - 1], labels[n0 - 1]
    assert len(dense) == B
    src = np.arange(B, dtype=np.int64) if perm is None else np.asarray(perm, dtype=np.int64)
    if fault == "inverse_perm" and perm is not None:
        inv = np.empty_like(src)
        inv[src] = np.arange(B)
        src = inv
    ok = (src >= 0) & (src < B)
    safe = np.where(ok, src, 0)
    h = None if hashes is None else np.asarray(hashes, dtype=np.int64).reshape(1, N_CAT)
    if h is None:
        ids = sparse
    elif fault == "truncated_modulo":
        s64 = sparse.astype(np.int64)
        ids = ((np.abs(s64) % h) * np.sign(s64)).astype(np.int32)
    else:
        ids = floormod_i32(sparse, np.broadcast_to(h, sparse.shape))
        assert np.array_equal(ids, (sparse.astype(np.int64) % h).astype(np.int32))  # numpy's own %, the reference's
    d = np.where(ok[:, None], dense[safe], np.float32(0)).astype(np.float32)
    v = np.where(ok[:, None], ids[safe], 0).astype(values_dtype)
    l = np.where(ok, labels[safe, 0], 0).astype(np.int32)
    if fault == "columns_swapped":
        v[:, [3, 4]] = v[:, [4, 3]]
    values = np.ascontiguousarray(v.T).reshape(-1)
    if fault == "last_tile_unwritten":
        from_row = (B - 1) // 64 * 64
        d[from_row:], l[from_row:] = CANARY_F32, CANARY_I32
        values.reshape(N_CAT, B)[:, from_row:] = CANARY_I32
    return d, values, l, int((~ok).sum())


FAULTS = ["truncated_modulo", "columns_swapped", "inverse_perm", "last_tile_unwritten", "segment_off_by_one"]
CANARY_F32 = np.float32(-12345.5)
CANARY_I32 = 0x5A5A5A5A


def assert_same_bits(got, want, what=""):
    """The one comparison of these tests: same dtype, same shape, same bytes (floats by bit pattern: -0.0 and NaN count)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        i = int(bad[0]) if len(bad) else -1
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first at flat index {i}: "
                             f"{got.reshape(-1)[i]!r} != {want.reshape(-1)[i]!r}")


def assert_batch_equal(got, want, what=""):
    """got / want: (dense, values, labels[, bad_perm])."""
    for name, g, w in zip(("dense", "values", "labels"), got, want):
        assert_same_bits(g, w, f"{what} {name}")
    if len(got) > 3 and len(want) > 3:
        assert int(got[3]) == int(want[3]), f"{what} bad_perm: {got[3]} != {want[3]}"


def config_key(world, rank, hashed, mmap, shuffle):
    return f"w{world}r{rank}|h{int(hashed)}|m{int(mmap)}|s{int(shuffle)}"


def configs(mmap_values=(False, True)):
    return [(w, r, h, m, s) for (w, r) in WORLDS for h in (False, True) for m in mmap_values for s in (False, True)]


def scalar(g, key):
    """A recorded scalar (the archive stores it as a one-element array)."""
    return int(np.asarray(g[key]).reshape(-1)[0])


def golden_batches(g, key):
    """[(dense, values, labels)] of one recorded configuration."""
    d, v, l = g[f"cfg|{key}|dense"], g[f"cfg|{key}|values"], g[f"cfg|{key}|labels"]
    return [(d[i], v[i], l[i]) for i in range(len(d))]


def batch_arrays(batch):
    """(dense, values, labels) of a Batch, on the host."""
    return (batch.dense_features.cpu().numpy(), batch.sparse_features.values().cpu().numpy(), batch.labels.cpu().numpy())
