"""GPU: the device path of the Criteo datapipe (torchrec_amd/datasets/criteo.py) against its host path and the reference's
recorded batches (tests/golden/criteo_datapipe.npz), bit for bit; streams; the ValueErrors; and four training steps of a small
DLRM fed from the host datapipe and from the device datapipe."""
import argparse

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _criteo_ref as cr
from torchrec_amd.datasets.criteo import InMemoryBinaryCriteoIterDataPipe

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TORCH_OF = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32}


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{variant: path lists}: the recorded files [37, 5, 300] and the same rows cut into [3, 2, 1, 2, 3, 1, 2, 1, 2, 300] + the
    rest, so that a batch of 16 has more than 8 pieces."""
    arrays = cr.synthetic_arrays()
    flat = [np.concatenate([a[i] for a in arrays]) for i in range(3)]
    many_rows = cr.ROWS_MANY + [sum(cr.ROWS) - sum(cr.ROWS_MANY)]
    many, at = [], 0
    for n in many_rows:
        many.append(tuple(f[at:at + n] for f in flat))
        at += n
    assert max(len(s) for s in cr.rank_segments(many_rows, 0, 1, cr.BATCH)) > 8
    return {"three": cr.write_files(tmp_path_factory.mktemp("three"), arrays),
            "many": cr.write_files(tmp_path_factory.mktemp("many"), many)}


def _pipe(paths, world, rank, hashed, shuffle, **kw):
    return InMemoryBinaryCriteoIterDataPipe(*paths, batch_size=cr.BATCH, rank=rank, world_size=world,
                                            shuffle_batches=shuffle, hashes=list(cr.HASHES) if hashed else None, **kw)


def _epoch(pipe):
    np.random.seed(cr.SHUFFLE_SEED)
    out = []
    for b in pipe:
        assert b.sparse_features.keys() == [f"cat_{i}" for i in range(26)] and b.sparse_features.stride() == cr.BATCH
        out.append(cr.batch_arrays(b))
    return out


@pytest.mark.parametrize("variant", ["three", "many"])
@pytest.mark.parametrize("resident", ["host", "device"])
@pytest.mark.parametrize("width", [np.int64, np.int32])
def test_device_path_equals_the_host_path_and_the_reference(golden, files, variant, resident, width):
    for world, rank, hashed, _mmap, shuffle in cr.configs(mmap_values=(False,)):
        key = cr.config_key(world, rank, hashed, False, shuffle)
        want = cr.golden_batches(golden, key)  # the same rows whatever the files' cut: the concatenation is the same
        host = _epoch(_pipe(files[variant], world, rank, hashed, shuffle))
        pipe = _pipe(files[variant], world, rank, hashed, shuffle, device=DEV, resident=resident,
                     values_dtype=TORCH_OF[np.dtype(width)])
        first = next(iter(pipe))
        assert first.dense_features.device == DEV and first.labels.device == DEV and first.sparse_features.device() == DEV
        got = _epoch(pipe)
        assert len(pipe) == len(got) == len(want) == len(host)
        for i, (g, h, w) in enumerate(zip(got, host, want)):
            cr.assert_batch_equal(h, w, f"{key} host batch {i}")
            assert w[1].dtype == np.int32
            w = (w[0], w[1].astype(width), w[2])  # the golden's int32 ids, widened for the int64 comparison
            cr.assert_batch_equal(g, w, f"{key} {variant} {resident} batch {i}")
        cr.assert_batch_equal(_epoch(pipe)[-1], got[-1], "a second epoch")  # iterating twice gives the same epoch
        assert pipe.bad_perm_count() == 0


@pytest.mark.parametrize("resident", ["host", "device"])
def test_next_under_alternating_streams(golden, files, resident):
    want = cr.golden_batches(golden, cr.config_key(1, 0, True, False, True))
    pipe = _pipe(files["many"], 1, 0, True, True, device=DEV, resident=resident)
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.current_stream()]
    np.random.seed(cr.SHUFFLE_SEED)
    it, got = iter(pipe), []
    for i in range(len(pipe)):
        with torch.cuda.stream(streams[i % 3]):
            got.append(next(it))  # not synchronised here: the pipe orders its reused buffers itself
    torch.cuda.synchronize()
    assert next(it, None) is None
    for i, (b, w) in enumerate(zip(got, want)):
        cr.assert_batch_equal(cr.batch_arrays(b), (w[0], w[1].astype(np.int64), w[2]), f"batch {i}")


def test_value_errors(files):
    paths = files["three"]
    with pytest.raises(ValueError, match="mmap_mode"):
        InMemoryBinaryCriteoIterDataPipe(*paths, batch_size=4, rank=0, world_size=1, mmap_mode=True, device=DEV)
    for bad in (0, -3, 2 ** 31, 7.0, True):
        hashes = list(cr.HASHES)
        hashes[9] = bad
        with pytest.raises(ValueError, match="cat_9"):
            InMemoryBinaryCriteoIterDataPipe(*paths, batch_size=4, rank=0, world_size=1, hashes=hashes, device=DEV)
    with pytest.raises(ValueError, match="25 entries"):
        InMemoryBinaryCriteoIterDataPipe(*paths, batch_size=4, rank=0, world_size=1, hashes=cr.HASHES[:25], device=DEV)
    with pytest.raises(ValueError, match="resident"):
        InMemoryBinaryCriteoIterDataPipe(*paths, batch_size=4, rank=0, world_size=1, device=DEV, resident="disk")
    with pytest.raises(ValueError, match="values_dtype"):
        InMemoryBinaryCriteoIterDataPipe(*paths, batch_size=4, rank=0, world_size=1, device=DEV, values_dtype=torch.int16)


def test_get_dataloader_returns_the_device_datapipe(tmp_path, golden):
    from torchrec_amd.datasets import dlrm_dataloader

    cr.write_files(tmp_path, cr.synthetic_arrays())
    args = argparse.Namespace(in_memory_binary_criteo_path=str(tmp_path), batch_size=cr.BATCH, shuffle_batches=False,
                              mmap_mode=False, num_embeddings=None, num_embeddings_per_feature=list(cr.HASHES), device=DEV)
    dl = dlrm_dataloader.get_dataloader(args, "nccl", "train")
    assert isinstance(dl, InMemoryBinaryCriteoIterDataPipe) and dl.resident == "host" and dl.values_dtype == torch.int64
    want = cr.golden_batches(golden, cr.config_key(1, 0, True, False, False))
    got = _epoch(dl)
    assert len(dl) == len(got) == len(want)
    for g, w in zip(got, want):
        cr.assert_batch_equal(g, (w[0], w[1].astype(np.int64), w[2]), "get_dataloader")


TRAIN_HASHES = [1, 2, 3, 7, 5000, 999] + list(range(1000, 1020))


def _train(paths, steps, **kw):
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.train_pipeline import TrainPipelineSparseDist
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.models.dlrm import DLRMTrain
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.optim.keyed import CombinedOptimizer, KeyedOptimizerWrapper

    torch.manual_seed(0)
    D, B, lr = 128, 64, 0.05
    keys = [f"cat_{i}" for i in range(26)]
    tables = [EmbeddingBagConfig(name=f"t_{k}", embedding_dim=D, num_embeddings=TRAIN_HASHES[i], feature_names=[k])
              for i, k in enumerate(keys)]
    ebc = EmbeddingBagCollection(tables, device=torch.device("meta"))
    tm = DLRMTrain(ebc, 13, [64, D], [64, 1], dense_device=DEV)
    model = DistributedModelParallel(tm, env=ShardingEnv.from_local(1, 0), device=DEV,
                                     sharders=[EmbeddingBagCollectionSharder({"learning_rate": lr})])
    dense_opt = KeyedOptimizerWrapper(dict(model.named_parameters()), lambda p: tm.dense_optimizer(p, lr=lr))
    opt = CombinedOptimizer([model.fused_optimizer, dense_opt])
    pipe = TrainPipelineSparseDist(model, opt, DEV)
    model.train()
    np.random.seed(cr.SHUFFLE_SEED)
    data = InMemoryBinaryCriteoIterDataPipe(*paths, batch_size=B, rank=0, world_size=1, shuffle_batches=True,
                                            hashes=TRAIN_HASHES, **kw)
    it = iter(data)
    losses = [pipe.progress(it)[0].detach().cpu().numpy().copy() for _ in range(steps)]
    torch.cuda.synchronize()
    shards = {n: w.detach().cpu().numpy().copy() for n, (w, _) in model.sharded_modules()[0].local_shards().items()}
    dense = {k: v.detach().cpu().numpy().copy() for k, v in model.named_parameters()}
    return losses, shards, dense


@pytest.mark.parametrize("resident", ["host", "device"])
def test_training_from_the_device_datapipe_equals_training_from_the_host_datapipe(files, resident):
    """DistributedModelParallel + TrainPipelineSparseDist: next() runs under the pipeline's memcpy stream, batch.to(device) is a
    no-op for device batches, and the pipeline's waits are the synchronisation.  Same batches, same kernels: same bits."""
    l0, s0, d0 = _train(files["three"], 4)
    l1, s1, d1 = _train(files["three"], 4, device=DEV, resident=resident)
    for a, b in zip(l0, l1):
        cr.assert_same_bits(b, a, "loss")
    assert len(s0) > 0 and s0.keys() == s1.keys()
    for k in s0:
        cr.assert_same_bits(s1[k], s0[k], f"table shard {k}")
    for k in d0:
        cr.assert_same_bits(d1[k], d0[k], f"dense parameter {k}")
    assert np.isfinite(np.array(l0)).all() and len({float(x) for x in l0}) > 1
