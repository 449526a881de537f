"""Dataloader glue of the DLRM trainer (examples/dlrm/data/dlrm_dataloader.py:23-131): `get_dataloader(args, backend,
stage)` with the reference's file selection.  Without `args.device` it returns a torch DataLoader as the reference does;
with `args.device` set it returns the device datapipe itself (iterable, with `__len__`): its batches are device tensors
already, and a DataLoader with pin_memory would try to pin them."""
import argparse
import os
from typing import List, Tuple

from torch import distributed as dist
from torch.utils.data import DataLoader, IterableDataset

from .criteo import CAT_FEATURE_COUNT, DAYS, DEFAULT_CAT_NAMES, DEFAULT_INT_NAMES, InMemoryBinaryCriteoIterDataPipe
from .random import RandomRecDataset

STAGES = ["train", "val", "test"]


def _rank_and_world() -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def stage_rank(stage: str, rank: int, world_size: int) -> Tuple[int, int]:
    """(rank, world_size) the datapipe is built with: train splits its days over the ranks; val takes the first half of
    the last day and test the second, by posing as ranks [0, W) and [W, 2 W) of a world of 2 W
    (dlrm_dataloader.py:57-71)."""
    if stage == "train":
        return rank, world_size
    return (rank if stage == "val" else rank + world_size), world_size * 2


def stage_files(directory: str, stage: str) -> List[List[str]]:
    """[dense, sparse, labels] path lists of a stage, each sorted: train takes every day but the last, val and test the
    last day (dlrm_dataloader.py:52-81)."""
    files = os.listdir(directory)

    def is_final_day(s: str) -> bool:
        return f"day_{DAYS - 1}" in s

    if stage == "train":
        files = [s for s in files if not is_final_day(s)]
    else:
        files = [s for s in files if is_final_day(s)]
    return [sorted(os.path.join(directory, s) for s in files if kind in s) for kind in ["dense", "sparse", "labels"]]


def _identity(x):
    return x


class _Iterable(IterableDataset):
    """RandomRecDataset is a plain iterable; a DataLoader tells the iterable style from the map style by this base."""

    def __init__(self, source) -> None:
        self.source = source

    def __iter__(self):
        return iter(self.source)


def _get_random_dataloader(args: argparse.Namespace) -> DataLoader:
    hash_sizes = (args.num_embeddings_per_feature if getattr(args, "num_embeddings_per_feature", None) is not None
                  else [args.num_embeddings] * CAT_FEATURE_COUNT)
    return DataLoader(
        _Iterable(RandomRecDataset(keys=DEFAULT_CAT_NAMES, batch_size=args.batch_size, hash_sizes=hash_sizes,
                                   manual_seed=args.seed if hasattr(args, "seed") else None, ids_per_feature=1,
                                   num_dense=len(DEFAULT_INT_NAMES))),
        batch_size=None, batch_sampler=None, pin_memory=args.pin_memory, num_workers=0)


def _get_in_memory_dataloader(args: argparse.Namespace, stage: str):
    rank, world_size = stage_rank(stage, *_rank_and_world())
    files = stage_files(args.in_memory_binary_criteo_path, stage)
    hashes = (args.num_embeddings_per_feature if getattr(args, "num_embeddings", None) is None
              else [args.num_embeddings] * CAT_FEATURE_COUNT)
    common = dict(batch_size=args.batch_size, rank=rank, world_size=world_size,
                  shuffle_batches=getattr(args, "shuffle_batches", False), mmap_mode=getattr(args, "mmap_mode", False),
                  hashes=hashes)
    device = getattr(args, "device", None)
    if device is not None:
        return InMemoryBinaryCriteoIterDataPipe(*files, **common, device=device, resident=getattr(args, "resident", None),
                                                values_dtype=getattr(args, "values_dtype", None))
    return DataLoader(InMemoryBinaryCriteoIterDataPipe(*files, **common), batch_size=None, pin_memory=args.pin_memory,
                      collate_fn=_identity)


def get_dataloader(args: argparse.Namespace, backend: str, stage: str):
    """The loader of `stage` ("train", "val" or "test") for the trainer's command-line options: the random dataset
    without `args.in_memory_binary_criteo_path`, the binary Criteo datapipe with it."""
    stage = stage.lower()
    if stage not in STAGES:
        raise ValueError(f"Supplied stage was {stage}. Must be one of {STAGES}.")
    args.pin_memory = (backend == "nccl") if not hasattr(args, "pin_memory") else args.pin_memory
    if not hasattr(args, "in_memory_binary_criteo_path") or args.in_memory_binary_criteo_path is None:
        return _get_random_dataloader(args)
    return _get_in_memory_dataloader(args, stage)
