"""Records tests/golden/bert4rec_metrics.npz from the REFERENCE's own recalls_and_ndcgs_for_ks
(examples/bert4rec/bert4rec_metrics.py).  Data only.

    python tests/golden/make_bert4rec_loss_golden.py --reference /path/to/torchrec-checkout

The reference package is imported the way make_bert4rec_golden.py does, then examples.bert4rec.bert4rec_metrics.

Keys:  <case>|scores    float32 [B, C], or [B, V] with <case>|candidates int64 [B, C] (the reference then sees the gathered
                        scores, as examples/bert4rec/bert4rec_main.py:244-245 gathers them)
       <case>|labels    int64 [B, C]
       <case>|ks        the subset of {1, 5, 10, C} that fits, ascending
       <case>|f32       the reference's floats: Recall@k for the ks, then NDCG@k
Every case is tie-free (the reference's sort is not stable) and every row has a positive."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_deepfm_golden import import_reference_package, write_npz  # noqa: E402

# name: (B, C, share of positives or None for one positive in column 0, V of a [B, V] + candidates case or None)
CASES = {"1x1": (1, 1, None, None), "7x101": (7, 101, None, None), "37x64": (37, 64, 0.3, None), "5x300": (5, 300, 0.5, None),
         "9x101of500": (9, 101, None, 500)}


def tie_free_scores(rng, B, width):
    """Distinct float32 values in every row."""
    base = rng.permutation(4 * width)[:width].astype(np.float32)
    rows = np.stack([rng.permutation(base) for _ in range(B)])
    return rows * np.float32(0.03125) - np.float32(1.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds torchrec/ and examples/)")
    ap.add_argument("--out", default=os.path.join(HERE, "bert4rec_metrics.npz"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    import_reference_package(args.reference)
    from examples.bert4rec.bert4rec_metrics import recalls_and_ndcgs_for_ks

    rng = np.random.default_rng(20241020)
    rec = {}
    for name, (B, C, share, V) in CASES.items():
        scores = tie_free_scores(rng, B, V or C)
        if share is None:
            labels = np.zeros((B, C), dtype=np.int64)
            labels[:, 0] = 1
        else:
            labels = (rng.random((B, C)) < share).astype(np.int64)
            labels[np.arange(B), rng.integers(0, C, size=B)] = 1
        ks = sorted({k for k in (1, 5, 10, C) if k <= C})
        listed = scores
        if V is not None:
            cand = np.stack([rng.permutation(V)[:C] for _ in range(B)]).astype(np.int64)
            rec[name + "|candidates"] = cand
            listed = np.take_along_axis(scores, cand, axis=1)
        for row in listed:
            assert len(np.unique(row)) == C, "ties"
        got = recalls_and_ndcgs_for_ks(torch.from_numpy(listed), torch.from_numpy(labels), ks)
        rec[name + "|scores"], rec[name + "|labels"] = scores, labels
        rec[name + "|ks"] = np.asarray(ks, dtype=np.int64)
        rec[name + "|f32"] = np.asarray([got["Recall@%d" % k] for k in ks] + [got["NDCG@%d" % k] for k in ks], dtype=np.float32)
    write_npz(args.out, rec)
    print(f"{args.out}: {len(rec)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
