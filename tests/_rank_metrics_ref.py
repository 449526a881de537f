"""Float64 numpy restatement of Recall@k / NDCG@k as include/tbe_hip.h (tbe_rank_metrics_f32) defines them, the golden
archive of the reference's own results, the tolerance derived from it, and the inputs the CPU and GPU tests share.

    pos_j  = #{i : s_i > s_j} + #{i < j : s_i == s_j}          the place of j in np.argsort(-s, kind="stable"); NaN last
    hits   = #{j positive : pos_j < k};   Recall = hits / min(k, n_pos)
    DCG    = sum of w[pos_j] over those hits in ascending pos_j;   IDCG = sum of w[0 : min(k, n_pos)];   w[p] = 1 / log2(p + 2)
The three keyword switches build the WRONG definitions the premise guards of tests/test_rank_metrics.py need."""
import functools
import os

import numpy as np

import _paths

KS_WANTED = (1, 5, 10)  # and C: the subset that fits is used (make_bert4rec_loss_golden.py)


def ks_for(C):
    return sorted({k for k in KS_WANTED + (C,) if k <= C})


def positions(s, ties_to_higher_index=False):
    """pos[j] for every j of one row of scores: NaN ranks after every number, -0.0 ties with +0.0."""
    s = np.asarray(s, dtype=np.float64)
    if s.shape[0] > 1024 and not ties_to_higher_index:  # the same places without the [C, C] tables (test_rank_metrics.py
        pos = np.empty(s.shape[0], dtype=np.int64)      # checks the two against each other on the edge rows)
        pos[np.argsort(-s, kind="stable")] = np.arange(s.shape[0])
        return pos
    key = np.where(np.isnan(s), -np.inf, s)          # every NaN below every number ...
    nan = np.isnan(s)
    C = s.shape[0]
    idx = np.arange(C)
    gt = (key[None, :] > key[:, None]) | (~nan[None, :] & nan[:, None])   # ... also below a true -inf
    eq = (key[None, :] == key[:, None]) & (nan[None, :] == nan[:, None])
    before = idx[None, :] > idx[:, None] if ties_to_higher_index else idx[None, :] < idx[:, None]
    return (gt | (eq & before)).sum(1)


def row_values(s, y, ks, ties_to_higher_index=False, inclusive=False):
    """({k: recall}, {k: ndcg}, {k: hits}) of one row in float64; NaN for a row without a positive."""
    y = np.asarray(y).astype(np.float64)
    pos = positions(s, ties_to_higher_index)[y == 1]
    n_pos = int((y == 1).sum())
    rec, ndcg, hits = {}, {}, {}
    for k in ks:
        hit_pos = np.sort(pos[(pos <= k) if inclusive else (pos < k)])
        w = 1.0 / np.log2(np.arange(2, 2 + max(k, int(hit_pos.max(initial=0)) + 1), dtype=np.float64))
        lim = min(k, n_pos)
        hits[k] = len(hit_pos)
        with np.errstate(invalid="ignore", divide="ignore"):
            rec[k] = np.float64(len(hit_pos)) / np.float64(lim)
            ndcg[k] = np.float64(w[hit_pos].sum()) / np.float64(w[:lim].sum())
    return rec, ndcg, hits


def per_row(scores, labels, ks, candidates=None, drop_last_candidate=False, **kw):
    """float64 [B, 2 nk] in the layout of the ABI's row_values (recalls, then ndcgs, ks ascending) and int hits [B, nk]."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    if candidates is not None:
        scores = np.take_along_axis(scores, np.asarray(candidates), axis=1)
    if drop_last_candidate:
        scores, labels = scores[:, :-1], labels[:, :-1]
    ks = sorted(ks)
    vals = np.empty((scores.shape[0], 2 * len(ks)), dtype=np.float64)
    hits = np.empty((scores.shape[0], len(ks)), dtype=np.int64)
    for b in range(scores.shape[0]):
        rec, ndcg, h = row_values(scores[b], labels[b], ks, **kw)
        vals[b] = [rec[k] for k in ks] + [ndcg[k] for k in ks]
        hits[b] = [h[k] for k in ks]
    return vals, hits


def metrics(scores, labels, ks, candidates=None, **kw):
    """The dict of the public function, in float64."""
    ks = sorted(set(ks))
    if kw.get("drop_last_candidate"):
        ks = [k for k in ks if k <= np.asarray(labels).shape[1] - 1]
    vals, _ = per_row(scores, labels, ks, candidates, **kw)
    mean = vals.mean(0) if len(vals) else np.full(2 * len(ks), np.nan)
    out = {}
    for q, k in enumerate(ks):
        out["Recall@%d" % k] = float(mean[q])
        out["NDCG@%d" % k] = float(mean[len(ks) + q])
    return out


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(_paths.ROOT, "tests", "golden", "bert4rec_metrics.npz"))
    return {k: z[k] for k in z.files}


def golden_cases():
    return sorted({k.split("|")[0] for k in golden()})


def golden_case(case):
    """(scores f32, labels i64, candidates or None, ks, {metric: the reference's float32 record})."""
    z = golden()
    ks = [int(k) for k in z[case + "|ks"]]
    cand = z[case + "|candidates"] if case + "|candidates" in z else None
    names = ["Recall@%d" % k for k in ks] + ["NDCG@%d" % k for k in ks]
    return z[case + "|scores"], z[case + "|labels"], cand, ks, dict(zip(names, (float(v) for v in z[case + "|f32"])))


@functools.lru_cache(maxsize=None)
def reference_f32_error():
    """The reference's own float32 error: its record against this float64 restatement, largest over the golden cases.  The
    reference computes the weights, the sums and the ideal DCG in float32 whatever dtype the scores have, so it has no
    float64 run to compare with.  Measured, not hard-coded; the premise guards of tests/test_rank_metrics.py show that a
    wrong restatement is orders of magnitude further away."""
    worst = 0.0
    for case in golden_cases():
        scores, labels, cand, ks, rec = golden_case(case)
        want = metrics(scores, labels, ks, cand)
        worst = max(worst, max(abs(rec[n] - want[n]) for n in rec))
    return worst


def tolerance():
    """8 x the reference's measured float32 error: this project's convention (metric values lie in [0, 1])."""
    return 8.0 * reference_f32_error()


def edge_rows():
    """(scores [6, 8] float32, labels [6, 8] int64): ties, NaN scores, -0.0, +-inf — every row has a positive.  The last
    column comments give the positives' positions under the tie rule."""
    nan, inf = np.nan, np.inf
    s = np.array([
        [1.0, 2.0, 2.0, 0.5, 2.0, -1.0, 0.0, 3.0],     # three-way tie at 2.0: indices 1, 2, 4 -> places 1, 2, 3
        [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, -0.0, 0.0],  # -0.0 ties with +0.0: places 1 .. 6 in index order
        [nan, 1.0, nan, -inf, 2.0, nan, 0.0, inf],     # NaNs after -inf, in index order: places 5, 6, 7
        [nan, nan, nan, nan, nan, nan, nan, nan],      # all NaN: index order
        [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0],      # all equal: index order
        [-inf, inf, -inf, inf, 0.0, -0.0, nan, 1.0],
    ], dtype=np.float32)
    y = np.array([
        [0, 0, 1, 0, 1, 0, 0, 0],
        [0, 0, 0, 1, 0, 0, 1, 0],
        [1, 0, 0, 1, 0, 1, 0, 0],
        [0, 0, 1, 0, 0, 0, 0, 1],
        [0, 1, 0, 0, 0, 0, 1, 0],
        [1, 0, 1, 1, 0, 1, 1, 0],
    ], dtype=np.int64)
    return s, y


EDGE_POSITIONS = [[2, 3], [4, 5], [5, 4, 7], [2, 7], [1, 6], [5, 6, 1, 4, 7]]  # of the positives, in index order


def k_boundary_rows(C, k):
    """Two rows of C distinct scores with one positive each: at place k - 1 (a hit of k) and at place k (no hit)."""
    s = np.tile(np.arange(C, 0, -1, dtype=np.float32), (2, 1))  # descending: place == index
    y = np.zeros((2, C), dtype=np.int64)
    y[0, k - 1] = 1
    if k < C:
        y[1, k] = 1
    else:
        y[1, k - 1] = 1
    return s, y
