"""Host model of tbe_auroc_counts_f32 (csrc/auroc.hip), shared by tests/test_auroc.py and the GPU suites: the six integer
counters in numpy int64 / Python integers, and the uint32 key transform of the prepare kernel restated in numpy."""
import numpy as np

SPECIALS = np.array([
    -np.inf,
    np.finfo(np.float32).min,                                  # largest-magnitude negative normal
    -np.finfo(np.float32).tiny,                                # smallest-magnitude negative normal
    np.array(0x807FFFFF, dtype=np.uint32).view(np.float32),    # largest-magnitude negative denormal
    np.array(0x80000001, dtype=np.uint32).view(np.float32),    # smallest-magnitude negative denormal
    -0.0,
    0.0,
    np.array(0x00000001, dtype=np.uint32).view(np.float32),    # smallest positive denormal
    np.array(0x007FFFFF, dtype=np.uint32).view(np.float32),    # largest positive denormal
    np.finfo(np.float32).tiny,
    1.0,
    np.nextafter(np.float32(1.0), np.float32(2.0)),
    np.finfo(np.float32).max,
    np.inf,
], dtype=np.float32)


def key_transform(preds, canonicalise_zero=True):
    """The order-preserving uint32 key of a float32 array: -0.0 -> +0.0 first, then b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000)."""
    b = np.ascontiguousarray(preds, dtype=np.float32).view(np.uint32).copy()
    if canonicalise_zero:
        b[b == np.uint32(0x80000000)] = np.uint32(0)
    mask = np.where(b >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return b ^ mask


def two_u_from_sorted(keys_sorted, pos_sorted):
    """2U = sum_j (Pc[b_{j+1}] - Pc[b_j]) * (Nc[b_j] + Nc[b_{j+1}]) over the tie groups of an ascending key array (any
    dtype with ==); pos_sorted: 1 for a positive, 0 for a negative, in the same order.  Python integer."""
    n = len(keys_sorted)
    if n == 0:
        return 0
    pos = np.asarray(pos_sorted, dtype=np.int64)
    pc = np.concatenate([[0], np.cumsum(pos)])            # exclusive counts, [n + 1]
    nc = np.concatenate([[0], np.cumsum(1 - pos)])
    starts = np.flatnonzero(np.concatenate([[True], keys_sorted[1:] != keys_sorted[:-1]]))
    b = np.concatenate([starts, [n]])
    terms = (pc[b[1:]] - pc[b[:-1]]) * (nc[b[:-1]] + nc[b[1:]])   # each < 2^59 for n < 2^29
    return int(terms.sum(dtype=np.int64))


def counts(preds, labels, threshold=0.5):
    """[2U, P, N, n_correct, n_nan, n_bad_label] as Python integers.  Stable argsort on float compare, so that -0.0 and
    +0.0 tie as they do as floats.  With a NaN or a bad label 2U follows the device's conventions only loosely (the ABI
    leaves it unspecified): compare slots 4 and 5 then."""
    preds = np.ascontiguousarray(preds, dtype=np.float32).reshape(-1)
    labels = np.asarray(labels).reshape(-1)
    assert preds.shape == labels.shape
    is_pos = labels == 1
    is_neg = labels == 0
    n_bad = int((~(is_pos | is_neg)).sum())
    n_nan = int(np.isnan(preds).sum())
    with np.errstate(invalid="ignore"):
        n_correct = int(((preds >= np.float32(threshold)) == is_pos).sum())
    order = np.argsort(preds, kind="stable")
    two_u = two_u_from_sorted(preds[order], is_pos[order].astype(np.int64))
    return [two_u, int(is_pos.sum()), int(is_neg.sum()), n_correct, n_nan, n_bad]


def counts_via_keys(preds, labels, canonicalise_zero=True):
    """2U computed the way the device does: sort the uint32 keys, group by key equality.  With canonicalise_zero=False
    this is the bug the GPU test must be able to see (-0.0 ordered below +0.0 instead of tied with it)."""
    k = key_transform(preds, canonicalise_zero)
    order = np.argsort(k, kind="stable")
    return two_u_from_sorted(k[order], (np.asarray(labels).reshape(-1) == 1)[order].astype(np.int64))


def auroc(c):
    """The float the metric returns: Python int / int, correctly rounded."""
    return c[0] / (2 * c[1] * c[2])


def accuracy(c):
    return c[3] / (c[1] + c[2])
