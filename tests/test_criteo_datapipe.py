"""CPU half of the Criteo datapipe (torchrec_amd/datasets/criteo.py, dlrm_dataloader.py, csrc/criteo_batch.hip): the host
path against the reference's recorded batches (tests/golden/criteo_datapipe.npz, written by
tests/golden/make_criteo_golden.py from the reference itself), BinaryCriteoUtils, the file selection per stage, the new
symbols and their argument checks, the numpy model of the kernel (tests/_criteo_ref.py) against the same recordings, and
the comparison of the GPU tests against injected faults."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _paths
import _criteo_ref as cr
from fbgemm_gpu import _lib
from torchrec_amd.datasets import criteo
from torchrec_amd.datasets.criteo import BinaryCriteoUtils, InMemoryBinaryCriteoIterDataPipe
from torchrec_amd.datasets import dlrm_dataloader

INVALID = -1


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def arrays():
    return cr.synthetic_arrays()


@pytest.fixture(scope="module")
def files(tmp_path_factory, arrays):
    return cr.write_files(tmp_path_factory.mktemp("criteo"), arrays)


def test_the_synthetic_draw_is_the_recorded_one(golden, arrays):
    assert cr.scalar(golden, "seed") == cr.SEED and list(golden["rows"]) == cr.ROWS and list(golden["hashes"]) == cr.HASHES
    assert cr.scalar(golden, "batch") == cr.BATCH and cr.scalar(golden, "shuffle_seed") == cr.SHUFFLE_SEED
    cr.assert_same_bits(cr.checksum(arrays), golden["checksum"], "checksum")
    sparse = np.concatenate([s for _, s, _ in arrays])
    assert (sparse < 0).mean() > 0.4 and sparse.min() < -2 ** 30 and sparse.max() > 2 ** 30  # the whole int32 range


def test_constants_and_batch_home():
    assert (criteo.INT_FEATURE_COUNT, criteo.CAT_FEATURE_COUNT, criteo.DAYS) == (13, 26, 24)
    assert criteo.DEFAULT_LABEL_NAME == "label" and criteo.TOTAL_TRAINING_SAMPLES == 4195197692
    assert criteo.DEFAULT_INT_NAMES == [f"int_{i}" for i in range(13)]
    assert criteo.DEFAULT_CAT_NAMES == [f"cat_{i}" for i in range(26)]
    assert criteo.DEFAULT_COLUMN_NAMES == ["label"] + criteo.DEFAULT_INT_NAMES + criteo.DEFAULT_CAT_NAMES
    from torchrec_amd.datasets.random import Batch as from_random
    from torchrec_amd.datasets.utils import Batch

    assert from_random is Batch


@pytest.mark.parametrize("world,rank,hashed,mmap,shuffle", cr.configs(),
                         ids=[cr.config_key(*c) for c in cr.configs()])
def test_host_path_equals_the_reference_batch_for_batch(golden, files, world, rank, hashed, mmap, shuffle):
    key = cr.config_key(world, rank, hashed, mmap, shuffle)
    want = cr.golden_batches(golden, key)
    np.random.seed(cr.SHUFFLE_SEED)
    pipe = InMemoryBinaryCriteoIterDataPipe(*files, batch_size=cr.BATCH, rank=rank, world_size=world,
                                            shuffle_batches=shuffle, mmap_mode=mmap,
                                            hashes=list(cr.HASHES) if hashed else None)
    assert len(pipe) == cr.scalar(golden, f"cfg|{key}|len") == len(want)
    got = list(pipe)
    assert len(got) == len(want)
    # the reference's quirk, kept: int64 ids only where numpy promoted int32 % int64 per batch
    assert want[0][1].dtype == (np.int64 if mmap and hashed else np.int32)
    for i, (b, w) in enumerate(zip(got, want)):
        assert b.dense_features.device.type == "cpu"
        cr.assert_batch_equal(cr.batch_arrays(b), w, f"{key} batch {i}")
        kjt = b.sparse_features
        assert kjt.keys() == list(golden["keys"]) and kjt.stride() == cr.scalar(golden, "stride") == cr.BATCH
        assert kjt.length_per_key() == [cr.BATCH] * 26 and kjt._lengths is None and kjt._offsets is None  # nothing built
    kjt = got[0].sparse_features
    cr.assert_same_bits(kjt.lengths().numpy(), golden["lengths"], "lengths")
    assert np.array_equal(kjt.offsets().numpy(), golden["offsets"])  # int64 here, int32 there: the values


def test_row_ranges_against_the_reference(golden):
    for i, case in enumerate(golden["rowrange_cases"]):
        rank, world, *lengths = [int(x) for x in case if x >= 0]
        got = BinaryCriteoUtils.get_file_idx_to_row_range(lengths, rank, world)
        assert [[k, a, b] for k, (a, b) in got.items()] == golden[f"rowrange|{i}"].tolist(), case


def test_load_npy_range_and_its_errors(tmp_path):
    a = np.arange(40, dtype=np.int32).reshape(10, 4)
    p = str(tmp_path / "a.npy")
    np.save(p, a)
    assert BinaryCriteoUtils.get_shape_from_npy(p) == (10, 4)
    assert BinaryCriteoUtils.get_shape_from_npy(p, path_manager_key="anything") == (10, 4)
    for mmap in (False, True):
        cr.assert_same_bits(np.asarray(BinaryCriteoUtils.load_npy_range(p, 3, 5, mmap_mode=mmap)), a[3:8], "range")
    p1 = str(tmp_path / "b.npy")
    np.save(p1, np.arange(5, dtype=np.int32))
    with pytest.raises(ValueError, match="Cannot load range for npy with ndim == 2"):
        BinaryCriteoUtils.load_npy_range(p1, 0, 1)
    with pytest.raises(ValueError, match=r"start_row \(10\) is out of bounds. It must be between 0 and 9, inclusive"):
        BinaryCriteoUtils.load_npy_range(p, 10, 1)
    with pytest.raises(ValueError, match=r"start_row \(-1\) is out of bounds"):
        BinaryCriteoUtils.load_npy_range(p, -1, 1)
    with pytest.raises(ValueError, match=r"num_rows \(8\) exceeds number of available rows \(10\) for the given start_row \(3\)"):
        BinaryCriteoUtils.load_npy_range(p, 3, 8)


def test_device_arguments_without_a_device_are_refused(files):
    with pytest.raises(ValueError, match="device"):
        InMemoryBinaryCriteoIterDataPipe(*files, batch_size=4, rank=0, world_size=1, resident="host")
    with pytest.raises(ValueError, match="device"):
        InMemoryBinaryCriteoIterDataPipe(*files, batch_size=4, rank=0, world_size=1, values_dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device"):
        InMemoryBinaryCriteoIterDataPipe(*files, batch_size=4, rank=0, world_size=1, device=torch.device("cpu"))


def test_get_dataloader_selects_the_files_of_each_stage(tmp_path, files):
    d = tmp_path / "days"
    d.mkdir()
    for day in range(criteo.DAYS):
        for kind in ("dense", "sparse", "labels"):
            (d / f"day_{day}_{kind}.npy").write_bytes(b"")
    train = dlrm_dataloader.stage_files(str(d), "train")
    for kind, lst in zip(("dense", "sparse", "labels"), train):
        assert lst == sorted(str(d / f"day_{day}_{kind}.npy") for day in range(criteo.DAYS - 1))
    for stage in ("val", "test"):
        assert dlrm_dataloader.stage_files(str(d), stage) == [[str(d / f"day_23_{kind}.npy")]
                                                              for kind in ("dense", "sparse", "labels")]
    assert dlrm_dataloader.stage_rank("train", 3, 8) == (3, 8)
    assert dlrm_dataloader.stage_rank("val", 3, 8) == (3, 16) and dlrm_dataloader.stage_rank("test", 3, 8) == (11, 16)
    assert dlrm_dataloader.STAGES == ["train", "val", "test"]
    with pytest.raises(ValueError, match="Must be one of"):
        dlrm_dataloader.get_dataloader(argparse.Namespace(), "gloo", "eval")


def test_get_dataloader_wraps_the_host_datapipe_like_the_reference(tmp_path, arrays, golden):
    """Real (tiny) files: day_0 .. day_2 for train, day_23 for val / test; the halves of the last day are the reference's
    rank / 2 * world_size trick."""
    cr.write_files(tmp_path, arrays)
    cr.write_files(tmp_path, arrays[2:], day0=23)
    args = argparse.Namespace(in_memory_binary_criteo_path=str(tmp_path), batch_size=cr.BATCH, shuffle_batches=False,
                              mmap_mode=False, num_embeddings=None, num_embeddings_per_feature=list(cr.HASHES))
    dl = dlrm_dataloader.get_dataloader(args, "gloo", "train")
    assert isinstance(dl, torch.utils.data.DataLoader) and args.pin_memory is False
    got = list(dl)
    want = cr.golden_batches(golden, cr.config_key(1, 0, True, False, False))
    assert len(dl) == len(got) == len(want)
    for b, w in zip(got, want):
        cr.assert_batch_equal(cr.batch_arrays(b), w, "train")
    halves = [list(dlrm_dataloader.get_dataloader(args, "gloo", stage)) for stage in ("val", "test")]
    d, s, l = arrays[2]
    for half, lo in zip(halves, (0, 150)):
        assert len(half) == 150 // cr.BATCH
        for i, b in enumerate(half):
            rows = slice(lo + i * cr.BATCH, lo + (i + 1) * cr.BATCH)
            want = cr.batch_ref([(d[rows], s[rows], l[rows])], cr.BATCH, cr.HASHES, None, np.int32)
            cr.assert_batch_equal(cr.batch_arrays(b), want[:3], "half")
    rnd = dlrm_dataloader.get_dataloader(argparse.Namespace(batch_size=8, num_embeddings=100, seed=1), "gloo", "train")
    b = next(iter(rnd))
    assert b.dense_features.shape == (8, 13) and b.sparse_features.values().numel() == 8 * 26


def test_new_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(_paths.ROOT, "include", "tbe_hip.h")).read()
    for name in ("tbe_criteo_batch_i64", "tbe_criteo_batch_i32"):
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    for text in ("#define TBE_CRITEO_MAX_SEGMENTS 8", "#define TBE_CRITEO_TILE_ROWS 64", "tbe_criteo_segment;",
                 "torchrec/datasets/criteo.py:760-784"):
        assert text in hdr, text
    assert _lib.CRITEO_MAX_SEGMENTS == 8 and _lib.CRITEO_TILE_ROWS == 64
    assert ctypes.sizeof(_lib.CriteoSegment) == 32
    assert lib.tbe_abi_version() == 3


def _segs(*items):
    a = (_lib.CriteoSegment * max(len(items), 1))()
    for k, (d, s, l, n) in enumerate(items):
        a[k].dense, a[k].sparse, a[k].labels, a[k].rows = d, s, l, n
    return a


@pytest.mark.parametrize("entry", ["tbe_criteo_batch_i64", "tbe_criteo_batch_i32"])
def test_entries_refuse_bad_arguments_before_any_launch(entry):
    """Every call here must return before a launch: the addresses are not device memory."""
    lib = _lib.load()
    fn = getattr(lib, entry)
    P = 0x10000

    def call(items, nseg=None, B=None, hashes=None, perm=None, dense=P, values=P, labels=P, bad=None):
        B = sum(i[3] for i in items) if B is None else B
        rc = fn(_segs(*items), len(items) if nseg is None else nseg, B, hashes, perm, dense, values, labels, bad, None)
        return rc, lib.tbe_last_error().decode()

    good = (P, P, P, 4)
    for nseg in (-1, 9):
        rc, msg = call([good], nseg=nseg)
        assert rc == INVALID and f"nseg={nseg}" in msg and "0 .. 8" in msg
    rc, msg = call([good], B=-1)
    assert rc == INVALID and "negative" in msg
    rc, msg = call([good, (P, P, P, -2)], B=2)
    assert rc == INVALID and "segment 1" in msg and "negative" in msg
    for k, bad_seg in enumerate([(None, P, P, 4), (P, None, P, 4), (P, P, None, 4)]):
        rc, msg = call([good, bad_seg])
        assert rc == INVALID and "segment 1" in msg and "null" in msg, msg
    for bad_seg in [(P + 2, P, P, 4), (P, P + 1, P, 4), (P, P, P + 3, 4)]:
        rc, msg = call([good, bad_seg])
        assert rc == INVALID and "segment 1" in msg and "misaligned" in msg, msg
    for B in (7, 9):
        rc, msg = call([good, good], B=B)
        assert rc == INVALID and "not the sum of the segment rows" in msg
    rc, msg = call([good], nseg=0, B=4)  # no segments, rows wanted
    assert rc == INVALID and "not the sum" in msg
    for kw in ({"dense": None}, {"values": None}, {"labels": None}):
        rc, msg = call([good], **kw)
        assert rc == INVALID and "null output" in msg
    for kw in ({"dense": P + 2}, {"labels": P + 1}, {"hashes": P + 2}, {"perm": P + 4}, {"bad": P + 2},
               {"values": P + 4 if entry.endswith("i64") else P + 2}):
        rc, msg = call([good], **kw)
        assert rc == INVALID and "misaligned" in msg, kw
    if entry.endswith("i32"):  # (the _i64 entry would accept this size and launch)
        big = (2 ** 31 + 25) // 26  # 26 * B > 2^31 - 1
        assert 26 * big >= 2 ** 31 > 26 * (big - 1)
        rc, msg = call([(P, P, P, big)])
        assert rc == INVALID and "26 * B" in msg
    rc, msg = call([(P, P, P, 2 ** 40 + 1)])
    assert rc == INVALID and "too large" in msg
    # the empty batch launches nothing and succeeds, whatever the pointers; empty segments are never looked at
    assert call([], B=0, dense=None, values=None, labels=None)[0] == 0
    assert call([(None, None, None, 0), (P + 1, None, P, 0)], B=0, dense=None, values=None, labels=None)[0] == 0


@pytest.mark.parametrize("world,rank,hashed,mmap,shuffle", cr.configs(), ids=[cr.config_key(*c) for c in cr.configs()])
def test_the_numpy_model_of_the_kernel_equals_the_reference(golden, arrays, world, rank, hashed, mmap, shuffle):
    """Ties the GPU tests' expectation to the reference: raw rows + segments + the batch's permutation -> the recorded batch."""
    want = cr.golden_batches(golden, cr.config_key(world, rank, hashed, mmap, shuffle))
    plan = cr.rank_segments(cr.ROWS, rank, world, cr.BATCH)
    assert len(plan) == len(want)
    np.random.seed(cr.SHUFFLE_SEED)
    for i, (segs, w) in enumerate(zip(plan, want)):
        pieces = [tuple(a[r0:r0 + n] for a in arrays[f]) for f, r0, n in segs]
        perm = np.random.permutation(cr.BATCH) if shuffle else None
        got = cr.batch_ref(pieces, cr.BATCH, cr.HASHES if hashed else None, perm, w[1].dtype)
        assert got[3] == 0
        cr.assert_batch_equal(got[:3], w, f"batch {i}")
    assert max(len(s) for s in plan) == (3 if (world, rank) in ((1, 0), (2, 0)) else 1)


def test_floor_modulo_examples():
    assert cr.floormod_i32(-7, 3) == 2 and cr.floormod_i32(-2 ** 31, 2 ** 31 - 1) == 2 ** 31 - 2
    assert cr.floormod_i32(2 ** 31 - 1, 2 ** 31 - 1) == 0 and cr.floormod_i32(-1, 1) == 0
    v = np.array([-2 ** 31, -1, 0, 2 ** 31 - 1], dtype=np.int32)
    for h in (1, 2, 3, 7, 40_000_000, 2 ** 31 - 1):
        assert np.array_equal(cr.floormod_i32(v, np.int32(h)), v.astype(np.int64) % h)


@pytest.mark.parametrize("fault", cr.FAULTS)
def test_the_comparison_rejects_every_injected_fault(fault):
    """The comparison the GPU tests use must fail on each of these stand-ins for a broken kernel."""
    B = 2 * 64 + 3
    arrays = cr.synthetic_arrays([64, 1, B - 65], seed=3)
    rng = np.random.default_rng(1)
    perm = rng.permutation(B)
    assert not np.array_equal(perm[perm], np.arange(B))  # not its own inverse
    want = cr.batch_ref(arrays, B, cr.HASHES, perm)
    cr.assert_batch_equal(cr.batch_ref(arrays, B, cr.HASHES, perm), want, "clean")
    with pytest.raises(AssertionError):
        cr.assert_batch_equal(cr.batch_ref(arrays, B, cr.HASHES, perm, fault=fault), want, fault)
