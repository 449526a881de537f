"""CPU: the host model of the device-side AUROC (tests/_auroc_ref.py) against sklearn, the key transform of the prepare
kernel, and the argument checks of tbe_auroc_counts_f32 that must fail before anything is launched (examples/dlrm/
dlrm_main.py:252-265 is the call site the entry serves)."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _auroc_ref as ref
import torchrec_amd.metrics  # noqa: F401  (the package under test: this file is about nothing else)


def _sk():
    return pytest.importorskip("sklearn.metrics").roc_auc_score


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n).astype(np.float32), rng.integers(0, 2, size=n)


def test_model_matches_sklearn_on_random_data():
    x, y = _random(5000, 1)
    assert abs(ref.auroc(ref.counts(x, y)) - _sk()(y, x)) <= 1e-12


def test_model_matches_sklearn_on_heavily_tied_data():
    rng = np.random.default_rng(2)
    x = (rng.integers(0, 8, size=5000) / 8).astype(np.float32)
    y = (rng.random(5000) < 0.2 + 0.6 * x).astype(np.int64)
    c = ref.counts(x, y)
    assert abs(ref.auroc(c) - _sk()(y, x)) <= 1e-12
    assert c[0] == ref.counts_via_keys(x, y)


def test_model_all_tied_is_exactly_one_half():
    x = np.full(1001, 0.25, dtype=np.float32)
    y = np.arange(1001) % 3 == 0
    c = ref.counts(x, y)
    assert c[0] == c[1] * c[2] and ref.auroc(c) == 0.5
    assert abs(_sk()(y, x) - 0.5) <= 1e-12


@pytest.mark.parametrize("flip,expect", [(False, 1.0), (True, 0.0)])
def test_model_perfectly_separated(flip, expect):
    x, y = _random(2000, 3)
    x = (x * 0.4 + 0.5 * (y != flip)).astype(np.float32)  # the positives (or, flipped, the negatives) above every other sample
    assert ref.auroc(ref.counts(x, y)) == expect
    assert abs(_sk()(y, x) - expect) <= 1e-12


def test_model_counts_are_the_pairwise_definition():
    """2U against the O(n^2) definition the ABI states: sum over positives of 2 * #{neg <} + #{neg ==}."""
    rng = np.random.default_rng(4)
    x = (rng.integers(0, 20, size=300) / 20).astype(np.float32)
    y = rng.integers(0, 2, size=300)
    pos, neg = x[y == 1], x[y == 0]
    brute = int((2 * (neg[None, :] < pos[:, None]).sum() + (neg[None, :] == pos[:, None]).sum()))
    c = ref.counts(x, y, threshold=0.4)
    assert c[0] == brute and c[1] == pos.size and c[2] == neg.size and c[4] == 0 and c[5] == 0
    assert c[3] == int(((x >= np.float32(0.4)) == (y == 1)).sum())


def test_key_transform_is_strictly_monotone_on_the_specials():
    s = ref.SPECIALS
    assert np.all(np.diff(s.astype(np.float64)) >= 0)  # the list itself is ascending, -0.0 next to +0.0
    k = ref.key_transform(s).astype(np.int64)
    zero = int(np.flatnonzero(s == 0)[0])  # the -0.0 entry
    assert np.signbit(s[zero]) and not np.signbit(s[zero + 1])
    assert k[zero] == k[zero + 1] == 0x80000000
    rest = np.delete(k, zero)
    assert np.all(np.diff(rest) > 0)
    assert k[0] == 0x007FFFFF and k[-1] == 0xFF800000  # -inf, +inf: ordinary values at the ends


def test_key_transform_agrees_with_float_order_on_random_bit_patterns():
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, size=20000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    k = ref.key_transform(x)
    order = np.argsort(k, kind="stable")
    xs = x[order]
    assert np.all(xs[1:] >= xs[:-1])
    assert np.array_equal(k[order][1:] == k[order][:-1], xs[1:] == xs[:-1])  # equal keys <=> equal floats


def test_a_model_without_the_zero_canonicalisation_differs_on_signed_zeros():
    """Premise of the GPU suite's specials case: ordering -0.0 below +0.0 changes 2U, so a kernel that forgets the
    canonicalisation cannot pass it."""
    x = np.array([-0.0, -0.0, 0.0, 0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    y = np.array([1, 1, 0, 0, 0, 0, 1, 0])  # not symmetric in the sign of zero: a symmetric mix hides the bug
    good = ref.counts(x, y)[0]
    assert good == ref.counts_via_keys(x, y, canonicalise_zero=True)
    assert good != ref.counts_via_keys(x, y, canonicalise_zero=False)


def _lib():
    from fbgemm_gpu import _lib

    return _lib.load()


FAKE = 0x10000  # a non-null, 256-B aligned address that is never dereferenced: every call below fails before any launch


def test_entry_refuses_2_pow_29_samples_before_any_launch():
    lib = _lib()
    big = 1 << 29
    assert lib.tbe_auroc_workspace_bytes(big) == 0
    assert lib.tbe_auroc_workspace_bytes(big - 1) > 4 * 4 * (big - 1)
    assert lib.tbe_auroc_workspace_bytes(-1) == 0
    rc = lib.tbe_auroc_counts_f32(FAKE, FAKE, 4, big, 0.5, FAKE, FAKE, 1 << 40, None)
    assert rc == -1 and b"2^29" in lib.tbe_last_error()


def test_entry_refuses_a_bad_label_width_before_any_launch():
    lib = _lib()
    nbytes = lib.tbe_auroc_workspace_bytes(100)
    for width in (0, 1, 2, 16):
        rc = lib.tbe_auroc_counts_f32(FAKE, FAKE, width, 100, 0.5, FAKE, FAKE, nbytes, None)
        assert rc == -1 and b"float32 (4) or int64 (8)" in lib.tbe_last_error()


def test_entry_refuses_a_short_or_misaligned_workspace_and_null_pointers_before_any_launch():
    lib = _lib()
    nbytes = lib.tbe_auroc_workspace_bytes(100)
    assert nbytes > 0 and nbytes % 256 == 0
    rc = lib.tbe_auroc_counts_f32(FAKE, FAKE, 8, 100, 0.5, FAKE, FAKE, nbytes - 1, None)
    assert rc == -3 and b"workspace too small" in lib.tbe_last_error()
    rc = lib.tbe_auroc_counts_f32(FAKE, FAKE, 8, 100, 0.5, FAKE, FAKE + 64, nbytes, None)
    assert rc == -1 and b"256-B aligned" in lib.tbe_last_error()
    for args in ((None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)):
        preds, labels, cnt, ws = args
        rc = lib.tbe_auroc_counts_f32(preds, labels, 4, 100, 0.5, cnt, ws, nbytes, None)
        assert rc == -1 and b"null pointer" in lib.tbe_last_error()
    assert lib.tbe_abi_version() == 3


def test_metrics_refuse_cpu_tensors():
    from torchrec_amd.metrics import AUROC, Accuracy

    for m in (AUROC(), Accuracy(threshold=0.3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.update(torch.tensor([0.1, 0.9]), torch.tensor([0, 1]))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.tensor([0.1, 0.9]), torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="compute_on_step"):
        AUROC(compute_on_step=True)
