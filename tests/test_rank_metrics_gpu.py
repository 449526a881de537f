"""GPU: torchrec_amd.metrics.recalls_and_ndcgs_for_ks on the kernel path — the reference's records
(tests/golden/bert4rec_metrics.npz) through the public function, the `[:, -1, :]` view with candidates, label dtypes, one
device-to-host copy per call, the errors, and the fallback beyond the kernel's limit."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _rank_metrics_ref as rr
from torchrec_amd.metrics import recalls_and_ndcgs_for_ks
from torchrec_amd.metrics import ranking

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _close(got, want, tol):
    assert list(got) and set(got) == set(want)
    return max(abs(got[n] - want[n]) for n in want) <= tol


@pytest.fixture
def kernel_calls(monkeypatch):
    """Counts the calls into tbe_rank_metrics_f32 and the torch fallback."""
    from fbgemm_gpu import _lib

    lib = _lib.load()
    calls = {"kernel": 0, "torch": 0}
    real_k, real_t = lib.tbe_rank_metrics_f32, ranking._recalls_and_ndcgs_torch

    class Lib:
        def __getattr__(self, name):
            return getattr(lib, name)

        def tbe_rank_metrics_f32(self, *a):
            calls["kernel"] += 1
            return real_k(*a)

    def torch_path(*a, **kw):
        calls["torch"] += 1
        return real_t(*a, **kw)

    monkeypatch.setattr(ranking._lib, "load", lambda: Lib())
    monkeypatch.setattr(ranking, "_recalls_and_ndcgs_torch", torch_path)
    return calls


@pytest.mark.parametrize("case", rr.golden_cases())
def test_golden_cases_through_the_public_function(case, kernel_calls):
    scores, labels, cand, ks, rec = rr.golden_case(case)
    got = recalls_and_ndcgs_for_ks(_dev(scores), _dev(labels), ks, candidates=_dev(cand))
    assert kernel_calls == {"kernel": 1, "torch": 0}
    assert all(isinstance(v, float) for v in got.values())
    assert list(got) == [f"{m}@{k}" for k in sorted(ks, reverse=True) for m in ("Recall", "NDCG")]
    print(f"{case}: tolerance {rr.tolerance():.3e}, error {max(abs(got[n] - rec[n]) for n in rec):.2e}")
    assert _close(got, rec, rr.tolerance()) and _close(got, rr.metrics(scores, labels, ks, cand), rr.tolerance())
    again = recalls_and_ndcgs_for_ks(_dev(scores), _dev(labels), ks, candidates=_dev(cand))
    assert again == got  # bit-identical
    for dtype in (torch.bool, torch.float32):
        assert recalls_and_ndcgs_for_ks(_dev(scores), _dev(labels).to(dtype), ks, candidates=_dev(cand)) == got
    assert kernel_calls == {"kernel": 4, "torch": 0}


def test_the_last_position_view_goes_in_as_it_is_with_one_copy_to_the_host(kernel_calls, monkeypatch):
    """scores[:, -1, :] of a [B, T, V] tensor with candidates: bert4rec_main.py:244-245 inside the call."""
    rng = np.random.default_rng(21)
    B, T, V, C = 33, 4, 500, 101
    full = torch.from_numpy(rng.standard_normal((B, T, V)).astype(np.float32)).to(DEV)
    cand = np.stack([rng.permutation(V)[:C] for _ in range(B)]).astype(np.int64)
    labels = np.zeros((B, C), dtype=np.int64)
    labels[:, 0] = 1
    view = full[:, -1, :]
    assert not view.is_contiguous()
    ks = [1, 5, 10]
    lab, can = _dev(labels), _dev(cand)
    recalls_and_ndcgs_for_ks(view, lab, [10], candidates=can)  # the weight table of k = 10 is on the device from here on
    kernel_calls["kernel"] = 0
    reads = []
    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist", "numpy", "__int__", "__float__", "__bool__"):
            real = getattr(torch.Tensor, name)

            def counted(self, *a, _real=real, _name=name, **kw):
                if self.is_cuda:
                    reads.append(_name)
                return _real(self, *a, **kw)

            mp.setattr(torch.Tensor, name, counted)
        got = recalls_and_ndcgs_for_ks(view, lab, ks, candidates=can)
    assert reads == ["cpu"], reads  # one device-to-host copy, nothing else reads the device
    assert kernel_calls == {"kernel": 1, "torch": 0}
    want = rr.metrics(view.cpu().numpy(), labels, ks, cand)
    assert _close(got, want, rr.tolerance())
    ref = recalls_and_ndcgs_for_ks(view.gather(1, _dev(cand)), _dev(labels), ks)  # the reference's two-step form
    assert ref == got


def test_edge_rows_and_a_row_without_a_positive():
    s, y = rr.edge_rows()
    ks = [1, 2, 3, 5, 8]
    got = recalls_and_ndcgs_for_ks(_dev(s), _dev(y), ks)
    assert _close(got, rr.metrics(s, y, ks), rr.tolerance())
    cpu = recalls_and_ndcgs_for_ks(torch.from_numpy(s), torch.from_numpy(y), ks)
    assert _close(got, cpu, rr.tolerance())  # the fallback follows the same tie rule
    y = y.copy()
    y[4] = 0
    assert all(np.isnan(v) for v in recalls_and_ndcgs_for_ks(_dev(s), _dev(y), ks).values())


def test_errors_before_any_launch_and_bad_data_after_the_one_copy(kernel_calls):
    s, y = rr.edge_rows()
    for ks, text in (([0], "k=0"), ([9], "k=9 outside 1 .. C=8"), ([], "empty")):
        with pytest.raises(ValueError, match=text):
            recalls_and_ndcgs_for_ks(_dev(s), _dev(y), ks)
    with pytest.raises(ValueError, match="9 distinct ks"):
        recalls_and_ndcgs_for_ks(torch.zeros(2, 12, device=DEV), torch.ones(2, 12, dtype=torch.int64, device=DEV), range(1, 10))
    assert kernel_calls == {"kernel": 0, "torch": 0}
    bad_y = y.copy()
    bad_y[0, 0], bad_y[3, 3] = 2, -1
    with pytest.raises(ValueError, match="n_bad_candidate=0, n_bad_label=2"):
        recalls_and_ndcgs_for_ks(_dev(s), _dev(bad_y), [1])
    cand = np.tile(np.arange(8), (6, 1))
    cand[1, 2], cand[4, 7], cand[5, 0] = 8, -1, 1 << 40
    with pytest.raises(ValueError, match="n_bad_candidate=3, n_bad_label=0"):
        recalls_and_ndcgs_for_ks(_dev(s), _dev(y), [1], candidates=_dev(cand))
    assert kernel_calls == {"kernel": 2, "torch": 0}


def test_beyond_the_limit_and_other_dtypes_take_torch(kernel_calls):
    rng = np.random.default_rng(5)
    C = ranking.MAX_CANDIDATES + 1
    s = rng.standard_normal((2, C)).astype(np.float32)
    y = np.zeros((2, C), dtype=np.int64)
    y[:, 7] = 1
    got = recalls_and_ndcgs_for_ks(_dev(s), _dev(y), [1, 10])
    assert kernel_calls == {"kernel": 0, "torch": 1}
    assert _close(got, rr.metrics(s, y, [1, 10]), rr.tolerance())
    s, y = rr.edge_rows()
    recalls_and_ndcgs_for_ks(_dev(s).double(), _dev(y), [1])
    recalls_and_ndcgs_for_ks(_dev(s), _dev(y).int(), [1])
    assert kernel_calls == {"kernel": 0, "torch": 3}
