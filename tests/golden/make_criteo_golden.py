"""Records tests/golden/criteo_datapipe.npz from the REFERENCE's own InMemoryBinaryCriteoIterDataPipe.  Data only.

    python tests/golden/make_criteo_golden.py --reference /path/to/torchrec-checkout

torchrec/datasets/criteo.py and utils.py (and torchrec/sparse/jagged_tensor.py, torchrec/streamable.py behind them) are
loaded under namespace stand-ins for the `torchrec` packages, so that torchrec/__init__.py — which needs the built
library — is not executed.  iopath and pyre_extensions are not needed for what runs here: stand-ins are registered
(`PathManagerFactory().get(key).open` is `open`, `none_throws` is the identity), as the other golden makers do.

The day files are synthetic (tests/_criteo_ref.py synthetic_arrays: rows [37, 5, 300], ids over the whole int32 range) and are
NOT stored: `seed` and `checksum` pin the draw.  For every configuration — (world, rank) x hashes x mmap_mode x
shuffle_batches (under np.random.seed(5)) at batch 16 — every batch the reference yields is recorded:

    cfg|w<W>r<R>|h<0|1>|m<0|1>|s<0|1>|dense   [batches, 16, 13] float32
    ...|values                                 [batches, 416]     int32, or int64 with mmap_mode and hashes (the quirk)
    ...|labels                                 [batches, 16]      int32
    ...|len                                    len(datapipe)
    keys, lengths, offsets, stride             of the batches' KeyedJaggedTensor (the same for every batch)
    rowrange|<case>                            get_file_idx_to_row_range answers as rows of (file, left, right)
    rowrange_cases                             the cases: (rank, world_size, lengths...)
The archive is written with fixed member times, so a second run reproduces the file byte for byte."""
import argparse
import importlib
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _criteo_ref as cr  # noqa: E402

ROWRANGE_CASES = [(0, 1, 37, 5, 300), (0, 2, 37, 5, 300), (1, 2, 37, 5, 300), (2, 3, 37, 5, 300), (1, 4, 10, 10, 10, 10),
                  (3, 4, 1, 1, 1, 7), (0, 3, 2, 2), (2, 3, 2, 2), (5, 8, 100, 1, 1, 1, 100)]


def load_reference(root):
    io_mod = types.ModuleType("iopath.common.file_io")

    class PathManager:
        open = staticmethod(open)

    class PathManagerFactory:
        def get(self, key):
            return PathManager()

    io_mod.PathManager, io_mod.PathManagerFactory = PathManager, PathManagerFactory
    for name in ("iopath", "iopath.common"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["iopath.common.file_io"] = io_mod
    pe = types.ModuleType("pyre_extensions")
    pe.none_throws = lambda x, msg=None: x
    sys.modules["pyre_extensions"] = pe
    for name in ("torchrec", "torchrec.datasets", "torchrec.sparse"):  # namespaces: their __init__.py never runs
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(root, *name.split("."))]
        sys.modules[name] = m
    return importlib.import_module("torchrec.datasets.criteo")


def write_npz(path, rec):
    """np.load-compatible archive with fixed member times (np.savez stamps the clock into every member)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in rec.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds torchrec/)")
    ap.add_argument("--out", default=cr.GOLDEN)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    arrays = cr.synthetic_arrays()
    rec = {"seed": np.int64(cr.SEED), "rows": np.array(cr.ROWS, dtype=np.int64), "checksum": cr.checksum(arrays),
           "hashes": np.array(cr.HASHES, dtype=np.int64), "batch": np.int64(cr.BATCH),
           "shuffle_seed": np.int64(cr.SHUFFLE_SEED)}
    meta = None
    with tempfile.TemporaryDirectory() as tmp:
        paths = cr.write_files(tmp, arrays)
        for world, rank, hashed, mmap, shuffle in cr.configs():
            np.random.seed(cr.SHUFFLE_SEED)
            pipe = ref.InMemoryBinaryCriteoIterDataPipe(
                *paths, batch_size=cr.BATCH, rank=rank, world_size=world, shuffle_batches=shuffle, mmap_mode=mmap,
                hashes=list(cr.HASHES) if hashed else None)
            batches = list(pipe)
            assert len(batches) == len(pipe)
            pre = "cfg|" + cr.config_key(world, rank, hashed, mmap, shuffle) + "|"
            rec[pre + "dense"] = np.stack([b.dense_features.numpy() for b in batches])
            rec[pre + "values"] = np.stack([b.sparse_features.values().numpy() for b in batches])
            rec[pre + "labels"] = np.stack([b.labels.numpy() for b in batches])
            rec[pre + "len"] = np.int64(len(pipe))
            kjt = batches[0].sparse_features
            this = (list(kjt.keys()), kjt.lengths().numpy(), kjt.offsets().numpy(), kjt.stride())
            if meta is None:
                meta = this
            assert this[0] == meta[0] and this[3] == meta[3]
            assert np.array_equal(this[1], meta[1]) and np.array_equal(this[2], meta[2])
    rec["keys"] = np.array(meta[0])
    rec["lengths"], rec["offsets"], rec["stride"] = meta[1], meta[2], np.int64(meta[3])
    rec["rowrange_cases"] = np.array([list(c) + [-1] * (8 - len(c)) for c in ROWRANGE_CASES], dtype=np.int64)
    for i, (rank, world, *lengths) in enumerate(ROWRANGE_CASES):
        got = ref.BinaryCriteoUtils.get_file_idx_to_row_range(lengths, rank, world)
        rec[f"rowrange|{i}"] = np.array([[k, a, b] for k, (a, b) in got.items()], dtype=np.int64).reshape(-1, 3)
    write_npz(args.out, rec)
    print(f"{args.out}: {len(rec)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
