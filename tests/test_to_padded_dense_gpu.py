"""GPU: JaggedTensor.to_padded_dense through tbe_jagged_to_padded_dense_{i64,i32,f32} against every record of the
reference's own loop (tests/golden/bert4rec.npz) and the edges: B = 0, N = 1, all bags empty, the three value types,
2^24 + 1, desired_length=None, and no device-to-host copy when desired_length is given."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
from test_bert4rec_model import check_padded_dense_edges, check_padded_dense_records
from torchrec_amd.sparse.jagged_tensor import JaggedTensor

pytestmark = pytest.mark.gpu


def test_every_reference_record_matches_exactly():
    check_padded_dense_records("cuda")


def test_edges():
    check_padded_dense_edges("cuda")


def test_a_given_desired_length_needs_no_device_to_host_copy():
    dev = torch.device("cuda")
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 9, size=300).astype(np.int64)  # more than one block of outputs
    values = rng.integers(-5, 1000, size=int(lengths.sum())).astype(np.int64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).to(dev)
    jt = JaggedTensor(values=torch.from_numpy(values).to(dev), offsets=offsets)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = jt.to_padded_dense(desired_length=5, padding_value=-2.0, pad_from_beginning=False, chop_from_beginning=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = np.full((300, 5), -2.0, np.float32)
    lo = np.concatenate([[0], np.cumsum(lengths)])
    for b in range(300):
        n = min(int(lengths[b]), 5)
        want[b, :n] = values[lo[b]:lo[b] + n]
    np.testing.assert_array_equal(got.cpu().numpy(), want)
