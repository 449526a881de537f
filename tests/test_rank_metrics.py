"""CPU: torchrec_amd.metrics.recalls_and_ndcgs_for_ks — the float64 restatement (tests/_rank_metrics_ref.py) against the
reference's own records (tests/golden/bert4rec_metrics.npz), the torch fallback, the tie / NaN / -0.0 rules, the errors, and
premise guards: three wrong definitions that must leave the tolerance on these very inputs."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _rank_metrics_ref as rr
from torchrec_amd.metrics import recalls_and_ndcgs_for_ks
from torchrec_amd.metrics import ranking


def _close(got, want, tol):
    assert list(got) and set(got) == set(want)
    return max(abs(got[n] - want[n]) for n in want) <= tol


def test_the_archive_holds_the_cases_and_stays_small():
    import os

    here = os.path.join(_paths.ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(here, "bert4rec_metrics.npz")) < os.path.getsize(os.path.join(here, "bert4rec.npz"))
    shapes = set()
    for case in rr.golden_cases():
        scores, labels, cand, ks, rec = rr.golden_case(case)
        B, C = labels.shape
        shapes.add((B, C, cand is not None))
        assert ks == rr.ks_for(C) and len(rec) == 2 * len(ks)
        assert (labels.sum(1) >= 1).all()                                                 # every row has a positive
        listed = scores if cand is None else np.take_along_axis(scores, cand, axis=1)
        assert all(len(np.unique(row)) == C for row in listed)                            # tie-free
    assert shapes == {(1, 1, False), (7, 101, False), (37, 64, False), (5, 300, False), (9, 101, True)}


def test_the_reference_float32_error_is_measured_from_the_archive():
    err = rr.reference_f32_error()
    print(f"reference float32 record vs float64 restatement: {err:.3e}; tolerance {rr.tolerance():.3e}")
    assert 0.0 < err <= 16 * 2.0 ** -24  # a handful of float32 roundings of values in [0, 1], not a different definition


@pytest.mark.parametrize("case", rr.golden_cases())
def test_restatement_and_cpu_fallback_match_the_reference_records(case):
    scores, labels, cand, ks, rec = rr.golden_case(case)
    tol = rr.tolerance()
    assert _close(rr.metrics(scores, labels, ks, cand), rec, tol)
    got = recalls_and_ndcgs_for_ks(torch.from_numpy(scores), torch.from_numpy(labels), ks,
                                   candidates=None if cand is None else torch.from_numpy(cand))
    assert all(isinstance(v, float) for v in got.values())
    assert list(got) == [f"{m}@{k}" for k in sorted(ks, reverse=True) for m in ("Recall", "NDCG")]  # the reference's order
    assert _close(got, rec, tol)
    for dtype in (torch.bool, torch.float32):
        assert recalls_and_ndcgs_for_ks(torch.from_numpy(scores), torch.from_numpy(labels).to(dtype), ks,
                                        candidates=None if cand is None else torch.from_numpy(cand)) == got


@pytest.mark.parametrize("wrong", [{"ties_to_higher_index": True}, {"inclusive": True}, {"drop_last_candidate": True}])
def test_premise_a_wrong_definition_leaves_the_tolerance(wrong):
    """Ties broken the other way move a tie row; `pos <= k` and a dropped last candidate column move the golden cases."""
    tol = rr.tolerance()
    if "ties_to_higher_index" in wrong:
        s, y = rr.edge_rows()
        ks = [1, 2, 5]
        right, bad = rr.metrics(s, y, ks), rr.metrics(s, y, ks, **wrong)
        assert max(abs(right[n] - bad[n]) for n in right) > 1e3 * tol
        return
    # the dense golden case (37 x 64, ~30 % positives) has positives at place k and in its last column ...
    scores, labels, cand, ks, rec = rr.golden_case("37x64")
    bad = rr.metrics(scores, labels, ks, cand, **wrong)
    assert max(abs(bad[n] - rec[n]) for n in bad if n in rec) > 1e3 * tol
    # ... and so have the k-boundary rows of this file and of the GPU tests (one positive at place k, the best score last)
    s, y = rr.k_boundary_rows(12, 5)
    s, y = s[:, ::-1].copy(), y[:, ::-1].copy()  # ascending scores: the last column ranks first
    right, bad = rr.metrics(s, y, [5, 8]), rr.metrics(s, y, [5, 8], **wrong)
    assert max(abs(right[n] - bad[n]) for n in right) > 1e3 * tol


def test_ties_nan_and_signed_zero_follow_the_stable_descending_order():
    s, y = rr.edge_rows()
    for b in range(s.shape[0]):
        order = np.argsort(-s[b].astype(np.float64), kind="stable")
        pos = np.empty(s.shape[1], dtype=np.int64)
        pos[order] = np.arange(s.shape[1])
        np.testing.assert_array_equal(rr.positions(s[b]), pos)
        assert list(pos[y[b] == 1]) == rr.EDGE_POSITIONS[b]
    ks = [1, 2, 3, 5, 8]
    _, hits = rr.per_row(s, y, ks)
    want_hits = [[sum(p < k for p in row) for k in ks] for row in rr.EDGE_POSITIONS]
    np.testing.assert_array_equal(hits, want_hits)
    # the fallback ranks exactly so: per row (B = 1) its values are the restatement's
    for b in range(s.shape[0]):
        got = recalls_and_ndcgs_for_ks(torch.from_numpy(s[b:b + 1]), torch.from_numpy(y[b:b + 1]), ks)
        want = rr.metrics(s[b:b + 1], y[b:b + 1], ks)
        for k, h in zip(ks, want_hits[b]):
            assert got["Recall@%d" % k] == np.float32(h) / np.float32(min(k, len(rr.EDGE_POSITIONS[b])))  # exact in rank
        assert _close(got, want, rr.tolerance())


def test_k_boundaries():
    for C, k in ((12, 1), (12, 5), (12, 12)):
        s, y = rr.k_boundary_rows(C, k)
        _, hits = rr.per_row(s, y, [k])
        assert hits[0, 0] == 1 and hits[1, 0] == (1 if k == C else 0)
        got = recalls_and_ndcgs_for_ks(torch.from_numpy(s), torch.from_numpy(y), [k])
        assert got["Recall@%d" % k] == (1.0 if k == C else 0.5)


def test_a_row_without_a_positive_yields_nan_as_in_the_reference():
    s, y = rr.edge_rows()
    y = y.copy()
    y[2] = 0
    want = rr.metrics(s, y, [1, 5])
    got = recalls_and_ndcgs_for_ks(torch.from_numpy(s), torch.from_numpy(y), [1, 5])
    assert all(np.isnan(v) for v in want.values()) and all(np.isnan(v) for v in got.values())
    vals, _ = rr.per_row(s, y, [1, 5])
    assert np.isnan(vals[2]).all() and np.isfinite(np.delete(vals, 2, axis=0)).all()


def test_every_value_error_fires_before_anything_is_computed():
    s, y = (torch.from_numpy(a) for a in rr.edge_rows())
    for ks, text in (([0], "k=0"), ([-1, 2], "k=-1"), ([9], "k=9 outside 1 .. C=8"), ([], "empty"), (range(1, 9), None)):
        if text is None:
            assert len(recalls_and_ndcgs_for_ks(s, y, ks)) == 16  # 8 distinct ks are fine
            continue
        with pytest.raises(ValueError, match=text):
            recalls_and_ndcgs_for_ks(s, y, ks)
    wide = torch.zeros(2, 12)
    wide_y = torch.zeros(2, 12, dtype=torch.int64)
    wide_y[:, 0] = 1
    with pytest.raises(ValueError, match="9 distinct ks"):
        recalls_and_ndcgs_for_ks(wide, wide_y, range(1, 10))
    assert len(recalls_and_ndcgs_for_ks(wide, wide_y, [1, 1, 2, 2, 3, 4, 5, 6, 7, 8])) == 16  # repeats are one k
    with pytest.raises(ValueError, match="differ in shape"):
        recalls_and_ndcgs_for_ks(s, y[:, :7], [1])
    with pytest.raises(ValueError, match="differ in shape"):
        recalls_and_ndcgs_for_ks(s, y, [1], candidates=torch.zeros(6, 7, dtype=torch.int64))


def test_bad_candidates_and_labels_raise_with_their_counts():
    s, y = (torch.from_numpy(a) for a in rr.edge_rows())
    bad_y = y.clone()
    bad_y[0, 0], bad_y[3, 3] = 2, -1
    with pytest.raises(ValueError, match="n_bad_candidate=0, n_bad_label=2"):
        recalls_and_ndcgs_for_ks(s, bad_y, [1])
    cand = torch.arange(8).repeat(6, 1)
    cand[1, 2], cand[4, 7], cand[5, 0] = 8, -1, 1 << 40
    with pytest.raises(ValueError, match="n_bad_candidate=3, n_bad_label=0"):
        recalls_and_ndcgs_for_ks(s, y, [1], candidates=cand)


def test_the_weight_table_is_the_references_expression():
    w = ranking.dcg_weights(10)
    assert w.dtype == torch.float32 and torch.equal(w, 1 / torch.log2(torch.arange(2, 12).float()))
    big = ranking.dcg_weights(ranking.MAX_CANDIDATES)
    assert float(big.min()) > 2.0 ** -4 and float(big.max()) == 1.0  # what makes the kernel's float64 sums exact
