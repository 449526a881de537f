"""tbe_auroc_counts_f32 (csrc/auroc.hip) through the C ABI against the host model of tests/_auroc_ref.py: all six integer
counters bit for bit, guard bytes round every buffer, both label widths; then torchrec_amd.metrics (AUROC, Accuracy,
evaluate), whose floats must equal the model's exactly.  The call site served: examples/dlrm/dlrm_main.py:252-265."""
import functools

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _auroc_ref as ref

pytestmark = pytest.mark.gpu

TILE = 2048          # samples per workgroup tile of the reduce kernels (kAucTile)
SEGMENTS = 1024      # above TILE * SEGMENTS samples a workgroup walks more than one tile (kAucMaxSegments)
KS = [256, 512, 1024, 2048, 4096, 8192, 3 * 8192]
SIZES = [0, 1, 2, 63, 64, 65] + [k + d for k in KS for d in (-1, 0, 1)] + [256 * 2048 + 1]
# two tiles per segment, the last segment holding one partial tile: the only sizes at which the segment loop iterates
BIG = TILE * SEGMENTS + 2 * TILE + 7
GUARD = 256  # bytes on either side of every buffer


def _guarded(nbytes, align, misalign=0):
    """A device byte buffer of a known pattern with `nbytes` usable bytes starting `misalign` bytes behind an
    `align`-aligned address, GUARD bytes in front and at least GUARD behind.  Returns (whole buffer, offset)."""
    buf = torch.full((nbytes + 2 * GUARD + align + misalign,), 0xA5, dtype=torch.uint8, device="cuda")
    off = GUARD + (-(buf.data_ptr() + GUARD)) % align + misalign
    return buf, off


def hip_counts(preds, labels, threshold=0.5, misalign=0):
    """Runs the entry on host arrays; returns the six counters.  Asserts that the inputs and every guard byte round
    preds, labels, counts and the workspace are unchanged afterwards."""
    from fbgemm_gpu import _lib
    from fbgemm_gpu._lib import check, stream_ptr

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n = preds.size
    assert preds.dtype == np.float32 and labels.dtype in (np.float32, np.int64) and labels.size == n
    nbytes = lib.tbe_auroc_workspace_bytes(n)
    assert nbytes > 0 and nbytes % 256 == 0
    bufs = []
    for arr, align, mis in ((preds, 16, misalign * 4), (labels, 16, misalign * labels.itemsize)):
        buf, off = _guarded(arr.nbytes, align, mis)
        buf[off:off + arr.nbytes] = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
        bufs.append((buf, off, buf.clone()))
    cbuf, coff = _guarded(48, 8)
    wbuf, woff = _guarded(nbytes, 256)
    (pbuf, poff, pcopy), (lbuf, loff, lcopy) = bufs
    check(lib.tbe_auroc_counts_f32(pbuf.data_ptr() + poff, lbuf.data_ptr() + loff, labels.itemsize, n, threshold,
                                   cbuf.data_ptr() + coff, wbuf.data_ptr() + woff, nbytes, stream_ptr(dev)),
          "tbe_auroc_counts_f32")
    torch.cuda.synchronize()
    assert torch.equal(pbuf, pcopy) and torch.equal(lbuf, lcopy), "an input or its guard bytes changed"
    for buf, off, size in ((cbuf, coff, 48), (wbuf, woff, nbytes)):
        assert bool((buf[:off] == 0xA5).all()) and bool((buf[off + size:] == 0xA5).all()), "guard bytes overwritten"
    return [int(v) for v in cbuf[coff:coff + 48].cpu().numpy().view(np.int64)]


def _labels_for(x, rng, slope=0.6):
    """Labels correlated with the score, so that 2U is far from P * N and from 0."""
    lo, hi = float(np.min(x)), float(np.max(x))
    q = (x.astype(np.float64) - lo) / (hi - lo) if hi > lo else np.full(x.shape, 0.5)
    return (rng.random(x.size) < 0.2 + slope * q).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """(preds, labels int64, the model's counters) — generated and modelled once, shared by both label widths."""
    rng = np.random.default_rng(KINDS.index(kind) * 1_000_003 + n)
    if kind == "distinct":
        x = ((rng.permutation(n) + 0.5) / max(n, 1)).astype(np.float32)
        assert np.unique(x).size == n
        y = _labels_for(x, rng) if n else np.zeros(0, dtype=np.int64)
    elif kind == "levels8":  # tie groups span many tiles; with n a tile multiple, group ends fall on tile edges
        x = (rng.integers(0, 8, size=n) / 8).astype(np.float32)
        y = _labels_for(x, rng) if n else np.zeros(0, dtype=np.int64)
    elif kind == "levels8_even":  # eight groups of n / 8 samples: at n = 3 * 8192 the group ends 6144, 12288, 18432 are tile edges
        x = rng.permutation((np.arange(n) * 8 // max(n, 1)) / 8).astype(np.float32)
        y = _labels_for(x, rng) if n else np.zeros(0, dtype=np.int64)
    elif kind == "one_level":  # a single group over the whole input
        x = np.full(n, 0.375, dtype=np.float32)
        y = rng.integers(0, 2, size=n).astype(np.int64)
    elif kind == "all_pos_but_one":
        x = rng.random(n).astype(np.float32)
        y = np.ones(n, dtype=np.int64)
        if n:
            y[rng.integers(0, n)] = 0
    elif kind == "all_neg_but_one":
        x = rng.random(n).astype(np.float32)
        y = np.zeros(n, dtype=np.int64)
        if n:
            y[rng.integers(0, n)] = 1
    elif kind == "alternating":
        x = (rng.integers(0, 64, size=n) / 64).astype(np.float32)
        y = (np.arange(n) % 2).astype(np.int64)
    elif kind == "specials":  # -0.0 mostly positive, +0.0 mostly negative: tying them or not changes 2U
        x = ref.SPECIALS[rng.integers(0, ref.SPECIALS.size, size=n)]
        y = rng.integers(0, 2, size=n).astype(np.int64)
        zero = x == 0
        y[zero] = np.where(np.signbit(x[zero]), rng.random(int(zero.sum())) < 0.8, rng.random(int(zero.sum())) < 0.2)
    elif kind == "sigmoid":  # float32 saturation: every logit above ~17 gives exactly 1.0
        logits = rng.uniform(-30, 30, size=n).astype(np.float32)
        x = torch.sigmoid(torch.from_numpy(logits)).numpy()
        y = (rng.random(n) < x).astype(np.int64)
    else:
        raise ValueError(kind)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, ref.counts(x, y, 0.5)


KINDS = ["distinct", "levels8", "levels8_even", "one_level", "all_pos_but_one", "all_neg_but_one", "alternating", "specials",
         "sigmoid"]
LABEL_DTYPES = [np.float32, np.int64]


@pytest.mark.parametrize("ldt", LABEL_DTYPES, ids=["f32", "i64"])
@pytest.mark.parametrize("kind", KINDS)
def test_counts_bit_exact_over_the_size_list(kind, ldt):
    for n in SIZES:
        x, y, want = case(kind, n)
        got = hip_counts(x, y.astype(ldt))
        assert got == want, (kind, n, got, want)


@pytest.mark.parametrize("ldt", LABEL_DTYPES, ids=["f32", "i64"])
@pytest.mark.parametrize("kind", ["distinct", "levels8", "one_level"])
def test_counts_bit_exact_with_several_tiles_per_segment(kind, ldt):
    x, y, want = case(kind, BIG)
    assert hip_counts(x, y.astype(ldt)) == want


def test_the_specials_case_can_see_a_missing_zero_canonicalisation():
    x, y, want = case("specials", 4097)
    assert want[0] == ref.counts_via_keys(x, y) != ref.counts_via_keys(x, y, canonicalise_zero=False)


@pytest.mark.parametrize("ldt", LABEL_DTYPES, ids=["f32", "i64"])
@pytest.mark.parametrize("n", [3 * 8192 + 1, 256 * 2048 + 1])
def test_two_levels_with_the_split_round_every_tile_edge(n, ldt):
    """Two tie groups whose boundary sits at k - 1, k, k + 1 sorted samples for every tile multiple k of the size list."""
    rng = np.random.default_rng(n)
    y = rng.integers(0, 2, size=n).astype(np.int64)
    perm = rng.permutation(n)
    for k in KS:
        for split in (k - 1, k, k + 1):
            if split >= n:
                continue
            x = np.full(n, 0.75, dtype=np.float32)
            x[perm[:split]] = 0.25  # `split` samples of the low level, scattered over the input
            want = ref.counts(x, y, 0.5)
            assert hip_counts(x, y.astype(ldt)) == want, (n, split)


@pytest.mark.parametrize("ldt", LABEL_DTYPES, ids=["f32", "i64"])
def test_inputs_that_are_not_16_byte_aligned(ldt):
    """preds / labels one element behind a 16-B boundary: the prepare kernel takes its one-by-one path."""
    for kind in ("distinct", "levels8"):
        for n in (1, 65, 2049, 8191, 3 * 8192 + 1):
            x, y, want = case(kind, n)
            assert hip_counts(x, y.astype(ldt), misalign=1) == want, (kind, n)


def test_threshold_and_accuracy_count():
    x, y, _ = case("levels8", 8193)
    for thr in (0.0, 0.125, 0.3, 0.875, 1.0, 2.0, -1.0):
        assert hip_counts(x, y.astype(np.float32), thr) == ref.counts(x, y, thr), thr


@pytest.mark.parametrize("ldt", LABEL_DTYPES, ids=["f32", "i64"])
def test_one_nan_and_one_bad_label_are_counted_and_nothing_faults(ldt):
    x, y, _ = case("distinct", 8193)
    x, y = x.copy(), y.astype(ldt)
    x[4097] = np.nan
    y[77] = 2
    got = hip_counts(x, y)
    assert got[4] == 1 and got[5] == 1
    assert got[1] + got[2] == x.size - 1  # the bad label is in neither class
    torch.cuda.synchronize()


def test_two_runs_are_bit_identical():
    x, y, want = case("sigmoid", 3 * 8192 + 1)
    a, b = hip_counts(x, y.astype(np.float32)), hip_counts(x, y.astype(np.float32))
    assert a == b == want


# ---- torchrec_amd.metrics ---------------------------------------------------------------------------------------------

def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached cases are read-only


def test_metric_updates_over_unequal_batches_equal_one_compute_on_the_concatenation():
    from torchrec_amd.metrics import AUROC, Accuracy

    x, y, want = case("sigmoid", 8193)
    dev = torch.device("cuda", 0)
    auroc, acc = AUROC(compute_on_step=False).to(dev), Accuracy(compute_on_step=False).to(dev)
    cuts = [0, 700, 700, 1024, 1025, 3000, 8193]  # an empty batch; 1024 -> 2048 -> 4096 -> 8192 -> 16384: four growths
    caps = set()
    for a, b in zip(cuts[:-1], cuts[1:]):
        auroc(_dev(x[a:b]), _dev(y[a:b]))
        acc.update(_dev(x[a:b]), _dev(y[a:b]))
        caps.add(auroc._preds.numel())
    assert len(caps) >= 3  # at least two buffer growths happened
    r = auroc.compute()
    assert r.dim() == 0 and r.dtype == torch.float64
    assert r.item() == ref.auroc(want)
    assert acc.compute().item() == ref.accuracy(want)
    one, one_acc = AUROC().to(dev), Accuracy().to(dev)
    one.update(_dev(x), _dev(y))
    one_acc.update(_dev(x), _dev(y))
    assert one.compute().item() == r.item() and one_acc.compute().item() == acc.compute().item()
    # reset: the next compute sees only what came after it
    x2, y2, want2 = case("levels8", 4095)
    auroc.reset()
    acc.reset()
    auroc.update(_dev(x2), _dev(y2))
    acc.update(_dev(x2), _dev(y2))
    assert auroc.compute().item() == ref.auroc(want2) and acc.compute().item() == ref.accuracy(want2)


@pytest.mark.parametrize("tdt", [torch.bool, torch.int32, torch.int64, torch.float32, torch.float64])
def test_metric_takes_column_preds_and_every_target_dtype(tdt):
    from torchrec_amd.metrics import AUROC, Accuracy

    x, y, want = case("levels8", 2049)
    dev = torch.device("cuda", 0)
    auroc, acc = AUROC().to(dev), Accuracy().to(dev)
    preds = _dev(x).reshape(-1, 1)  # [B, 1], as a model's logits come
    auroc.update(preds, _dev(y).to(tdt))
    acc.update(preds.double(), _dev(y).to(tdt).reshape(-1, 1))
    assert auroc.compute().item() == ref.auroc(want)
    assert acc.compute().item() == ref.accuracy(want)


def test_accuracy_threshold():
    from torchrec_amd.metrics import Accuracy

    x, y, _ = case("levels8", 2049)
    for thr in (0.125, 0.3, 0.875):
        acc = Accuracy(threshold=thr).to("cuda")
        acc.update(_dev(x), _dev(y))
        assert acc.compute().item() == ref.accuracy(ref.counts(x, y, thr))


def test_metric_errors_name_the_counts():
    from torchrec_amd.metrics import AUROC, Accuracy

    x = _dev(np.linspace(0, 1, 100, dtype=np.float32))
    m = AUROC().to("cuda")
    m.update(x, torch.ones(100, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="positives=100, negatives=0"):
        m.compute()
    m.reset()
    xn = x.clone()
    xn[3] = float("nan")
    m.update(xn, (torch.arange(100, device="cuda") % 2))
    with pytest.raises(ValueError, match="n_nan=1, n_bad_label=0"):
        m.compute()
    a = Accuracy().to("cuda")
    lab = (torch.arange(100, device="cuda") % 2)
    lab[10] = 2
    lab[11] = -1
    a.update(x, lab)
    with pytest.raises(ValueError, match="n_nan=0, n_bad_label=2"):
        a.compute()
    e = AUROC().to("cuda")
    with pytest.raises(ValueError, match="positives=0, negatives=0"):
        e.compute()
    e._count = 1 << 29  # the limit is checked on the count alone, before anything is launched (no such buffer exists)
    with pytest.raises(ValueError, match="2\\^29"):
        e.compute()


def test_metric_compute_on_a_side_stream():
    from torchrec_amd.metrics import AUROC

    x, y, want = case("distinct", 3 * 8192 + 1)
    m = AUROC().to("cuda")
    m.update(_dev(x), _dev(y))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = m.compute().item()
    assert r == ref.auroc(want)


@pytest.mark.parametrize("start_in_training", [True, False])
def test_evaluate_on_a_tiny_dlrm_equals_the_model_on_eager_eval_logits(start_in_training):
    from torchrec_amd.datasets.random import RandomRecDataset
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.train_pipeline import TrainPipelineSparseDist
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.metrics import evaluate
    from torchrec_amd.models.dlrm import DLRMTrain
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.optim.keyed import CombinedOptimizer, KeyedOptimizerWrapper

    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    rows, D, B = [1000, 57], 128, 64
    keys = [f"cat_{i}" for i in range(len(rows))]
    tables = [EmbeddingBagConfig(name=f"t_{k}", embedding_dim=D, num_embeddings=rows[i], feature_names=[k])
              for i, k in enumerate(keys)]
    ebc = EmbeddingBagCollection(tables, device=torch.device("meta"))
    model = DistributedModelParallel(DLRMTrain(ebc, 13, [64, D], [96, 32, 1], dense_device=dev),
                                     env=ShardingEnv.from_local(1, 0), device=dev,
                                     sharders=[EmbeddingBagCollectionSharder({"learning_rate": 0.05})])
    opt = CombinedOptimizer([model.fused_optimizer,
                             KeyedOptimizerWrapper(dict(model.named_parameters()), lambda p: torch.optim.SGD(p, lr=0.05))])
    with torch.no_grad():  # spread the logits: freshly initialised tables give near-constant predictions
        for w, _ in model.sharded_modules()[0].local_shards().values():
            w.normal_(0.0, 1.0)
    batches = list(iter(RandomRecDataset(keys, B, rows, manual_seed=7, num_generated_batches=5, num_batches=5, device=dev)))
    assert len(batches) == 5
    model.eval()
    preds, labels = [], []
    for b in batches:  # the eager forward, before the pipeline takes over the sharded module's forward
        _, (_, logits, lab) = model(b)
        preds.append(torch.sigmoid(logits).cpu().numpy())
        labels.append(lab.cpu().numpy())
    want = ref.counts(np.concatenate(preds), np.concatenate(labels), 0.5)
    assert want[1] > 0 and want[2] > 0
    pipe = TrainPipelineSparseDist(model, opt, dev)
    model.train(start_in_training)
    auroc, accuracy = evaluate(pipe, iter(batches))
    assert isinstance(auroc, float) and isinstance(accuracy, float)
    assert auroc == ref.auroc(want) and accuracy == ref.accuracy(want)
    assert model.training is start_in_training
    # the reference's chaining: limit_batches - 2 batches of `iterator`, then two of `next_iterator`, all evaluated here
    nxt = iter(batches[3:])
    again = evaluate(pipe, iter(batches[:3] + batches[:1]), nxt, limit_batches=5, stage="test")
    assert again == (auroc, accuracy)
    assert next(nxt, None) is None  # both batches of next_iterator were consumed
    assert model.training is start_in_training
