"""Binary (npy) Criteo datapipe: torchrec/datasets/criteo.py `BinaryCriteoUtils` (:181-388) and
`InMemoryBinaryCriteoIterDataPipe` (:638-840), and a device-side batch builder the reference does not have.

Host path (no `device`): the reference's batches, bit for bit — the same rows per rank, the same batch boundaries across
files, numpy's floor modulo on the (often negative) raw ids, one `np.random.permutation(batch_size)` per batch when shuffling.
One quirk of the reference is kept on purpose: the ids of a batch are **int32** without `mmap_mode` (the hash is applied in
place at load time, `sparse_arr %= hashes`) and **int64** with `mmap_mode` and hashes (the hash is applied per batch as
`int32 % int64`, which numpy promotes).

Device path (`device=torch.device("cuda", i)`): the rank's rows are read once, raw, into pinned host memory
(`resident="host"`) or uploaded once to the device (`resident="device"`).  A batch is then a handful of contiguous row
ranges: under "host" each is copied asynchronously into a raw staging buffer, under "device" the kernel reads the file
slices in place; one launch of `tbe_criteo_batch_*` (csrc/criteo_batch.hip) hashes, shuffles, transposes and widens.
Everything is enqueued on the stream that is current at `next()`; nothing is copied back and nothing synchronises.

Out of scope: tsv_to_npys, sparse_to_contiguous, shuffle, CriteoIterDataPipe, criteo_terabyte, criteo_kaggle."""
import os
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import IterableDataset

from ..sparse.jagged_tensor import KeyedJaggedTensor
from .utils import PATH_MANAGER_KEY, Batch

INT_FEATURE_COUNT = 13
CAT_FEATURE_COUNT = 26
DAYS = 24
DEFAULT_LABEL_NAME = "label"
DEFAULT_INT_NAMES: List[str] = [f"int_{idx}" for idx in range(INT_FEATURE_COUNT)]
DEFAULT_CAT_NAMES: List[str] = [f"cat_{idx}" for idx in range(CAT_FEATURE_COUNT)]
DEFAULT_COLUMN_NAMES: List[str] = [DEFAULT_LABEL_NAME, *DEFAULT_INT_NAMES, *DEFAULT_CAT_NAMES]
TOTAL_TRAINING_SAMPLES = 4195197692  # Number of rows across days 0-22 (day 23 is used for validation and testing)

_PERM_RING = 4  # pinned permutation buffers in flight


def _read_header(fin) -> Tuple[Tuple[int, ...], bool, np.dtype]:
    np.lib.format.read_magic(fin)
    return np.lib.format.read_array_header_1_0(fin)


def _check_range(shape: Tuple[int, ...], start_row: int, num_rows: int) -> Tuple[int, int]:
    if len(shape) == 2:
        total_rows, row_size = shape
    else:
        raise ValueError("Cannot load range for npy with ndim == 2.")  # the reference's wording (criteo.py:368)
    if not (0 <= start_row < total_rows):
        raise ValueError(
            f"start_row ({start_row}) is out of bounds. It must be between 0 and {total_rows - 1}, inclusive.")
    if not (start_row + num_rows <= total_rows):
        raise ValueError(
            f"num_rows ({num_rows}) exceeds number of available rows ({total_rows}) for the given start_row "
            f"({start_row}).")
    return total_rows, row_size


class BinaryCriteoUtils:
    """The loading half of the reference's BinaryCriteoUtils (criteo.py:181-388).  `path_manager_key` is accepted and
    ignored: iopath is no dependency here, files are opened with plain `open`."""

    @staticmethod
    def get_shape_from_npy(path: str, path_manager_key: str = PATH_MANAGER_KEY) -> Tuple[int, ...]:
        """Shape of an npy file from its header alone."""
        with open(path, "rb") as fin:
            shape, _order, _dtype = _read_header(fin)
            return shape

    @staticmethod
    def get_file_idx_to_row_range(lengths: List[int], rank: int, world_size: int) -> Dict[int, Tuple[int, int]]:
        """Which files, and which (inclusive) row range of each, `rank` handles: every rank gets total // world_size
        consecutive rows of the concatenation (the tail is dropped)."""
        total_length = sum(lengths)
        rows_per_rank = total_length // world_size
        rank_left_g = rank * rows_per_rank
        rank_right_g = (rank + 1) * rows_per_rank - 1
        output = {}
        file_left_g, file_right_g = -1, -1
        for idx, length in enumerate(lengths):
            file_left_g = file_right_g + 1
            file_right_g = file_left_g + length - 1
            if rank_left_g <= file_right_g and rank_right_g >= file_left_g:
                overlap_left_g, overlap_right_g = max(rank_left_g, file_left_g), min(rank_right_g, file_right_g)
                output[idx] = (overlap_left_g - file_left_g, overlap_right_g - file_left_g)
        return output

    @staticmethod
    def load_npy_range(fname: str, start_row: int, num_rows: int, path_manager_key: str = PATH_MANAGER_KEY,
                       mmap_mode: bool = False) -> np.ndarray:
        """Rows [start_row, start_row + num_rows) of a 2-D npy file."""
        with open(fname, "rb") as fin:
            shape, _order, dtype = _read_header(fin)
            _total_rows, row_size = _check_range(shape, start_row, num_rows)
            if mmap_mode:
                data = np.load(fname, mmap_mode="r")
                data = data[start_row: start_row + num_rows]
            else:
                fin.seek(start_row * row_size * dtype.itemsize, os.SEEK_CUR)
                data = np.fromfile(fin, dtype=dtype, count=num_rows * row_size)
            return data.reshape((num_rows, row_size))


def _read_rows_pinned(fname: str, start_row: int, num_rows: int, row_size: int, dtype: torch.dtype) -> torch.Tensor:
    """Rows [start_row, start_row + num_rows) of an npy file, read straight into a pinned tensor (no pageable copy)."""
    out = torch.empty((num_rows, row_size), dtype=dtype, pin_memory=True)
    view = out.numpy()
    with open(fname, "rb") as fin:
        shape, fortran_order, file_dtype = _read_header(fin)
        _check_range(shape, start_row, num_rows)
        if fortran_order or shape[1] != row_size or file_dtype != view.dtype:
            raise ValueError(f"{fname}: expected a C-ordered [rows, {row_size}] {view.dtype} array, found "
                             f"{'Fortran' if fortran_order else 'C'}-ordered {shape} {file_dtype}")
        fin.seek(start_row * row_size * file_dtype.itemsize, os.SEEK_CUR)
        got = fin.readinto(memoryview(view).cast("B")) if view.nbytes else 0
        if got != view.nbytes:
            raise ValueError(f"{fname}: file ends after {got} of {view.nbytes} bytes of the row range")
    return out


class InMemoryBinaryCriteoIterDataPipe(IterableDataset):
    """Datapipe over the binary (npy) Criteo files: each rank holds its share of the rows in memory and yields `Batch`es.

    Without `device` this is the reference's class (criteo.py:638-840) and the batches are its batches, on the CPU; ids are
    int32, or int64 with `mmap_mode` and hashes (module docstring).

    Keyword-only, the device path: `device` (a HIP device) makes `next()` enqueue the batch on that device's current stream
    and return device tensors; `resident` is "host" (default: raw rows in pinned memory, copied per batch) or "device" (raw
    rows uploaded once); `values_dtype` is torch.int64 (default, what the embedding kernels consume) or torch.int32 (the
    host path's dtype).  `hashes` must then be 26 integers in [1, 2**31 - 1] or None (ids pass through, sign-extended);
    `mmap_mode` is refused: file-backed pageable memory is no source for an asynchronous copy."""

    def __init__(self, dense_paths: List[str], sparse_paths: List[str], labels_paths: List[str], batch_size: int,
                 rank: int, world_size: int, shuffle_batches: bool = False, mmap_mode: bool = False,
                 hashes: Optional[List[int]] = None, path_manager_key: str = PATH_MANAGER_KEY, *,
                 device: Optional[torch.device] = None, resident: Optional[str] = None,
                 values_dtype: Optional[torch.dtype] = None) -> None:
        self.dense_paths = dense_paths
        self.sparse_paths = sparse_paths
        self.labels_paths = labels_paths
        self.batch_size = batch_size
        self.rank = rank
        self.world_size = world_size
        self.shuffle_batches = shuffle_batches
        self.mmap_mode = mmap_mode
        self.hashes = hashes
        self.path_manager_key = path_manager_key
        self.keys: List[str] = DEFAULT_CAT_NAMES
        self.device = torch.device(device) if device is not None else None
        if self.device is None:
            if resident is not None or values_dtype is not None:
                raise ValueError("resident / values_dtype belong to the device path: give device=torch.device('cuda', i)")
            self.resident, self.values_dtype = None, None
            self._load_data_for_rank()
        else:
            self._init_device(resident, values_dtype)
        self.num_rows_per_file: List[int] = [int(a.shape[0]) for a in self.dense_arrs]
        self.num_batches: int = sum(self.num_rows_per_file) // batch_size

    # ---- host path: the reference's --------------------------------------------------------------------------------
    def _row_ranges(self) -> Dict[int, Tuple[int, int]]:
        return BinaryCriteoUtils.get_file_idx_to_row_range(
            lengths=[BinaryCriteoUtils.get_shape_from_npy(path, path_manager_key=self.path_manager_key)[0]
                     for path in self.dense_paths],
            rank=self.rank, world_size=self.world_size)

    def _load_data_for_rank(self) -> None:
        file_idx_to_row_range = self._row_ranges()
        self.dense_arrs, self.sparse_arrs, self.labels_arrs = [], [], []
        for arrs, paths in zip([self.dense_arrs, self.sparse_arrs, self.labels_arrs],
                               [self.dense_paths, self.sparse_paths, self.labels_paths]):
            for idx, (range_left, range_right) in file_idx_to_row_range.items():
                arrs.append(BinaryCriteoUtils.load_npy_range(
                    paths[idx], range_left, range_right - range_left + 1, path_manager_key=self.path_manager_key,
                    mmap_mode=self.mmap_mode))
        # With mmap_mode the hash is applied per batch in __iter__; otherwise here, once, in place: the arrays stay int32
        # (numpy computes int32 % int64 in int64 and casts back; floor modulo, so negative raw ids land in [0, hash)).
        if not self.mmap_mode and self.hashes is not None:
            hashes_np = np.array(self.hashes).reshape((1, CAT_FEATURE_COUNT))
            for sparse_arr in self.sparse_arrs:
                sparse_arr %= hashes_np

    def _np_arrays_to_batch(self, dense: np.ndarray, sparse: np.ndarray, labels: np.ndarray) -> Batch:
        if self.shuffle_batches:
            shuffler = np.random.permutation(len(dense))  # one call per batch: np.random.seed reproduces the order
            dense = dense[shuffler]
            sparse = sparse[shuffler]
            labels = labels[shuffler]
        # from_fixed_lengths: one id per bag is host-side metadata; no lengths / offsets tensors are built per batch
        return Batch(
            dense_features=torch.from_numpy(dense),
            sparse_features=KeyedJaggedTensor.from_fixed_lengths(
                self.keys, torch.from_numpy(sparse.transpose(1, 0).reshape(-1)), [1] * CAT_FEATURE_COUNT),
            labels=torch.from_numpy(labels.reshape(-1)))

    def _segments(self) -> Iterator[List[Tuple[int, int, int]]]:
        """Per batch, the (file, first row, rows) pieces it is made of, in order; the last partial batch is dropped."""
        file_idx, row_idx = 0, 0
        for _ in range(self.num_batches):
            segs, need = [], self.batch_size
            while need > 0:
                rows_to_get = min(need, self.num_rows_per_file[file_idx] - row_idx)
                if rows_to_get > 0:
                    segs.append((file_idx, row_idx, rows_to_get))
                row_idx += rows_to_get
                need -= rows_to_get
                if row_idx >= self.num_rows_per_file[file_idx]:
                    file_idx += 1
                    row_idx = 0
            yield segs

    def _iter_host(self) -> Iterator[Batch]:
        hashes_np = (np.array(self.hashes).reshape((1, CAT_FEATURE_COUNT))
                     if self.mmap_mode and self.hashes is not None else None)
        for segs in self._segments():
            parts: List[List[np.ndarray]] = [[], [], []]
            for file_idx, row_idx, rows in segs:
                slice_ = slice(row_idx, row_idx + rows)
                sparse_inputs = self.sparse_arrs[file_idx][slice_, :]
                if hashes_np is not None:
                    sparse_inputs = sparse_inputs % hashes_np  # int32 % int64: these batches carry int64 ids
                parts[0].append(self.dense_arrs[file_idx][slice_, :])
                parts[1].append(sparse_inputs)
                parts[2].append(self.labels_arrs[file_idx][slice_, :])
            yield self._np_arrays_to_batch(*(p[0] if len(p) == 1 else np.concatenate(p) for p in parts))

    # ---- device path ---------------------------------------------------------------------------------------------
    def _init_device(self, resident: Optional[str], values_dtype: Optional[torch.dtype]) -> None:
        if self.device.type != "cuda":
            raise ValueError(f"device={self.device}: the device path runs on a HIP device; leave device out for CPU batches")
        if self.mmap_mode:
            raise ValueError("mmap_mode=True cannot be combined with device: file-backed pageable memory is no source for "
                             "an asynchronous copy")
        self.resident = "host" if resident is None else resident
        if self.resident not in ("host", "device"):
            raise ValueError(f"resident={resident!r}: must be 'host' or 'device'")
        self.values_dtype = torch.int64 if values_dtype is None else values_dtype
        if self.values_dtype not in (torch.int64, torch.int32):
            raise ValueError(f"values_dtype={values_dtype}: must be torch.int64 or torch.int32")
        if self.hashes is not None:
            if len(self.hashes) != CAT_FEATURE_COUNT:
                raise ValueError(f"hashes has {len(self.hashes)} entries: one per categorical feature, "
                                 f"{CAT_FEATURE_COUNT}, is needed")
            for name, h in zip(self.keys, self.hashes):
                if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 1 <= int(h) <= 2 ** 31 - 1:
                    raise ValueError(f"hashes: feature {name} has hash {h!r}; the device path needs an integer in "
                                     "[1, 2**31 - 1]")
        from fbgemm_gpu import _lib

        self._lib = _lib
        lib = _lib.load()
        self._entry = lib.tbe_criteo_batch_i64 if self.values_dtype == torch.int64 else lib.tbe_criteo_batch_i32
        self._entry_name = "tbe_criteo_batch_i64" if self.values_dtype == torch.int64 else "tbe_criteo_batch_i32"
        ranges = self._row_ranges()
        B, dev = self.batch_size, self.device
        self.dense_arrs, self.sparse_arrs, self.labels_arrs = [], [], []
        for arrs, paths, width, dtype in ((self.dense_arrs, self.dense_paths, INT_FEATURE_COUNT, torch.float32),
                                          (self.sparse_arrs, self.sparse_paths, CAT_FEATURE_COUNT, torch.int32),
                                          (self.labels_arrs, self.labels_paths, 1, torch.int32)):
            for idx, (left, right) in ranges.items():
                t = _read_rows_pinned(paths[idx], left, right - left + 1, width, dtype)  # raw: the kernel hashes
                arrs.append(t.to(dev) if self.resident == "device" else t)
        with torch.cuda.device(dev):
            self._stage = (torch.empty((B, INT_FEATURE_COUNT), dtype=torch.float32, device=dev),
                           torch.empty((B, CAT_FEATURE_COUNT), dtype=torch.int32, device=dev),
                           torch.empty((B, 1), dtype=torch.int32, device=dev))
            self._hashes_dev = (torch.tensor([int(h) for h in self.hashes], dtype=torch.int32, device=dev)
                                if self.hashes is not None else None)
            self._bad_perm = torch.zeros(1, dtype=torch.int32, device=dev)
            self._done = torch.cuda.Event()  # recorded after each launch: the staging buffers are free behind it
            if self.shuffle_batches:
                self._perm_dev = torch.empty(B, dtype=torch.int64, device=dev)
                ring = [torch.empty(B, dtype=torch.int64, pin_memory=True) for _ in range(_PERM_RING)]
                self._perm_ring = [(t, t.numpy(), torch.cuda.Event()) for t in ring]
                self._perm_next = 0
            torch.cuda.current_stream().synchronize()  # load time only: the uploads have landed before the first batch
        self._segs = (_lib.CriteoSegment * _lib.CRITEO_MAX_SEGMENTS)()

    def bad_perm_count(self) -> int:
        """Permutation entries outside [0, batch_size) the kernel has met (synchronises: a diagnostic, never called by the
        pipe; np.random.permutation yields none)."""
        return int(self._bad_perm.item())

    def _device_batch(self, segs: List[Tuple[int, int, int]]) -> Batch:
        _lib, B, dev = self._lib, self.batch_size, self.device
        stream = torch.cuda.current_stream(dev)
        # the staging buffers and the device permutation were last read by the previous launch, possibly on another stream
        stream.wait_event(self._done)
        arrs = (self.dense_arrs, self.sparse_arrs, self.labels_arrs)
        if self.resident == "host" or len(segs) > _lib.CRITEO_MAX_SEGMENTS:
            off = 0
            for file_idx, row_idx, rows in segs:  # one asynchronous copy per kind: a segment is a contiguous row range
                for stage, arr in zip(self._stage, arrs):
                    stage[off:off + rows].copy_(arr[file_idx][row_idx:row_idx + rows], non_blocking=True)
                off += rows
            pieces = [tuple(s.data_ptr() for s in self._stage) + (B,)]
        else:
            pieces = [(self.dense_arrs[f].data_ptr() + 4 * INT_FEATURE_COUNT * r,
                       self.sparse_arrs[f].data_ptr() + 4 * CAT_FEATURE_COUNT * r,
                       self.labels_arrs[f].data_ptr() + 4 * r, n) for f, r, n in segs]
        for k, (d, s, l, n) in enumerate(pieces):
            sg = self._segs[k]
            sg.dense, sg.sparse, sg.labels, sg.rows = d, s, l, n
        perm_ptr = None
        if self.shuffle_batches:
            pinned, view, free = self._perm_ring[self._perm_next]
            self._perm_next = (self._perm_next + 1) % _PERM_RING
            if not free.query():  # its copy of _PERM_RING batches ago has not run yet: only then does the host wait
                free.synchronize()
            view[:] = np.random.permutation(B)  # the host path's call: the same seed gives the same batches
            self._perm_dev.copy_(pinned, non_blocking=True)
            free.record(stream)
            perm_ptr = self._perm_dev.data_ptr()
        dense = torch.empty((B, INT_FEATURE_COUNT), dtype=torch.float32, device=dev)
        values = torch.empty(CAT_FEATURE_COUNT * B, dtype=self.values_dtype, device=dev)
        labels = torch.empty(B, dtype=torch.int32, device=dev)
        rc = self._entry(self._segs, len(pieces), B, _lib.ptr(self._hashes_dev), perm_ptr, dense.data_ptr(),
                         values.data_ptr(), labels.data_ptr(), self._bad_perm.data_ptr(), stream.cuda_stream)
        _lib.check(rc, self._entry_name)
        self._done.record(stream)
        return Batch(dense_features=dense,
                     sparse_features=KeyedJaggedTensor.from_fixed_lengths(self.keys, values, [1] * CAT_FEATURE_COUNT),
                     labels=labels)

    def _iter_device(self) -> Iterator[Batch]:
        for segs in self._segments():
            with torch.cuda.device(self.device):
                batch = self._device_batch(segs)
            yield batch

    def __iter__(self) -> Iterator[Batch]:
        return self._iter_host() if self.device is None else self._iter_device()

    def __len__(self) -> int:
        return self.num_batches
