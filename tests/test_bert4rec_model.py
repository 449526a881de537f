"""CPU: torchrec_amd.models.bert4rec on its fall-back path against the reference's float32 records
(tests/golden/bert4rec.npz), the module tree's state-dict names, mask recognition, and JaggedTensor.to_padded_dense."""
import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _attention_ref as R
import _bert4rec_golden as G
from fbgemm_gpu import _lib
from torchrec_amd.models import bert4rec as M
from torchrec_amd.sparse.jagged_tensor import JaggedTensor


def _tol():
    supported = lambda L, d: bool(_lib.load().tbe_attention_supported(L, d))  # noqa: E731
    return R.measured_tolerance(((1, 1, R.max_L(supported, 128), 128),))


def build_mha(case, device="cpu"):
    z = G.load()
    H = int(case.split("h")[-1])
    P = G.params("mha", case)
    m = M.MultiHeadedAttention(num_heads=H, dim_model=P["output_linear.bias"].shape[0], dropout=0.0, device=device)
    assert list(m.state_dict().keys()) == list(P.keys())
    m.load_state_dict({n: torch.from_numpy(v) for n, v in P.items()})
    return m, z[f"mha|{case}|valid"]


def run_mha(m, case, mask, device="cpu"):
    """(out, gxq, gxk, gxv at the recorded rows, parameter gradients cut as the archive cuts them)."""
    xq, xk, xv, g, rows = G.mha_inputs(case)
    leaves = [torch.from_numpy(x).to(device).requires_grad_() for x in (xq, xk, xv)]
    m.zero_grad()
    out = m(*leaves, mask=mask)
    out.backward(torch.from_numpy(g).to(device))
    res = {"out": out.detach().cpu().numpy()[:, rows]}
    for n, x in zip(("gxq", "gxk", "gxv"), leaves):
        res[n] = x.grad.cpu().numpy()[:, rows]
    for n, p in m.named_parameters():
        res["grad|" + n] = G.stored_grad(p.grad.cpu().numpy())
    return res


def compare(res, kind, case, prec, tol):
    z, pre = G.load(), f"{kind}|{case}|{prec}|"
    assert {pre + n for n in res} == {k for k in z if k.startswith(pre)}
    for n, got in res.items():
        want = z[pre + n].astype(np.float64)
        scale = R.scale_of(want)
        if n.endswith("linear_layers.1.bias"):
            # The key projection's bias gradient is exactly zero in exact arithmetic (softmax ignores a constant added to a
            # whole row of scores); what is recorded and computed there is rounding residue of sums whose terms have the
            # scale of the same layer's weight gradient.  Every other output is compared at its own scale.
            scale = max(scale, R.scale_of(z[pre + n[:-len("bias")] + "weight"]))
        R.assert_close(got, want, tol, f"{kind} {case} {n}", scale)


@pytest.mark.parametrize("how", ["expand", "repeat"])
@pytest.mark.parametrize("case", G.cases("mha"))
def test_multi_headed_attention_fallback_matches_the_reference_records(case, how):
    m, valid = build_mha(case)
    res = run_mha(m, case, G.mask_of(valid, how))
    assert m.last_path == "torch"
    compare(res, "mha", case, "f32", _tol())
    compare(res, "mha", case, "f64", _tol())  # the float32 fall-back is within the tolerance of the exact result too


def build_block(case, device="cpu"):
    B, L, hidden, heads = (int(x) for x in case.replace("h", "x").split("x"))
    P = G.params("block", case)
    m = M.TransformerBlock(hidden, heads, P["feed_forward.w_1.bias"].shape[0], 0.1, device=device).eval()
    assert list(m.state_dict().keys()) == list(P.keys())
    m.load_state_dict({n: torch.from_numpy(v) for n, v in P.items()})
    return m


def run_block(m, case, how, device="cpu"):
    z, pre = G.load(), f"block|{case}|"
    x = torch.from_numpy(z[pre + "x"]).to(device).requires_grad_()
    m.zero_grad()
    out = m(x, G.mask_of(z[pre + "valid"], how, device))
    out.backward(torch.from_numpy(z[pre + "g"]).to(device))
    res = {"out": out.detach().cpu().numpy(), "gx": x.grad.cpu().numpy()}
    for n, p in m.named_parameters():
        res["grad|" + n] = G.stored_grad(p.grad.cpu().numpy())
    return res


@pytest.mark.parametrize("case", G.cases("block"))
def test_transformer_block_fallback_matches_the_reference_records(case):
    compare(run_block(build_block(case), case, "repeat"), "block", case, "f32", _tol())


def test_state_dict_names_and_order_are_the_references():
    """The names above the lookup.  BERT4Rec itself needs a HIP device (its EmbeddingCollection has no CPU path): the whole
    model's names are compared in tests/test_bert4rec_model_gpu.py."""
    names = [str(n) for n in G.load()["model|train|names"]]
    block = [n[len("transformer_blocks.0."):] for n in names if n.startswith("transformer_blocks.0.")]
    assert list(M.TransformerBlock(16, 2, 64, 0.0).state_dict().keys()) == block
    assert list(M.clones(torch.nn.Linear(2, 2), 3).state_dict().keys()) == [f"{i}.{n}" for i in range(3)
                                                                             for n in ("weight", "bias")]
    with pytest.raises(AssertionError):
        M.MultiHeadedAttention(num_heads=3, dim_model=16)


def test_attention_returns_output_and_probabilities():
    torch.manual_seed(0)
    q, k, v = torch.randn(2, 3, 5, 4), torch.randn(2, 3, 5, 4), torch.randn(2, 3, 5, 4)
    valid = torch.tensor([[1, 1, 0, 1, 0], [0, 0, 0, 0, 0]], dtype=torch.bool)
    out, p = M.Attention()(q, k, v, mask=valid[:, None, None, :])
    assert out.shape == (2, 3, 5, 4) and p.shape == (2, 3, 5, 5)
    torch.testing.assert_close(p.sum(-1), torch.ones(2, 3, 5))
    assert bool((p[0, :, :, 2] == 0).all()) and bool((p[1] == 0.2).all())  # no valid key: uniform over all keys
    want, _, _ = R.forward(q.permute(0, 2, 1, 3).numpy(), k.permute(0, 2, 1, 3).numpy(), v.permute(0, 2, 1, 3).numpy(),
                           valid.numpy())
    np.testing.assert_allclose(out.permute(0, 2, 1, 3).numpy(), want, rtol=1e-5, atol=1e-6)


def test_key_padding_masks_are_recognised_by_construction():
    B, L = 3, 5
    valid = R.key_valid("per_sample", B, L)
    ok, kv = M.key_padding_mask(None, B, L)
    assert ok and kv is None
    for mask in (G.mask_of(valid, "expand"), torch.from_numpy(valid)[:, None, None, :],
                 torch.from_numpy(valid[:1])[:, None, None, :].expand(1, 1, L, L), torch.from_numpy(valid).long()[:, None, None, :].expand(B, 1, L, L)):
        ok, kv = M.key_padding_mask(mask, B, L)
        assert ok and kv.dtype == torch.uint8 and kv.shape == (B, L) and kv.is_contiguous()
        np.testing.assert_array_equal(kv.numpy().astype(bool), np.broadcast_to(mask[:, 0, 0, :].numpy() != 0, (B, L)))
    per_query = G.mask_of(valid, "repeat").clone()
    per_query[0, 0, 1, 2] = ~per_query[0, 0, 1, 2]
    for mask in (G.mask_of(valid, "repeat"), per_query, torch.from_numpy(valid), torch.ones(B, 2, L, L, dtype=torch.bool),
                 torch.ones(B, 1, L, L + 1, dtype=torch.bool)):
        assert M.key_padding_mask(mask, B, L) == (False, None)
    # a mask that differs between query rows goes through the reference's formula and gives the reference's numbers
    torch.manual_seed(1)
    m = M.MultiHeadedAttention(num_heads=2, dim_model=8, dropout=0.0)
    x = torch.randn(B, L, 8)
    q, k, v = (layer(x).view(B, L, 2, 4).transpose(1, 2) for layer in m.linear_layers)
    want = m.output_linear(M.Attention()(q, k, v, mask=per_query)[0].transpose(1, 2).reshape(B, L, 8))
    torch.testing.assert_close(m(x, x, x, mask=per_query), want)
    assert m.last_path == "torch"


# ---- JaggedTensor.to_padded_dense

def padded_dense_cases():
    z = G.load()
    for case in G.cases("tpd"):
        for pad in (0, 1):
            for chop in (0, 1):
                yield case, pad, chop, z[f"tpd|{case}|values"], z[f"tpd|{case}|lengths"], z[f"tpd|{case}|{pad}{chop}"]


def check_padded_dense_records(device):
    n = 0
    for case, pad, chop, values, lengths, want in padded_dense_cases():
        for as_offsets in (False, True):
            v, lens = torch.from_numpy(values).to(device), torch.from_numpy(lengths).to(device)
            offsets = torch.cat([lens.new_zeros(1), torch.cumsum(lens, 0)]).to(torch.int64)
            jt = JaggedTensor(values=v, offsets=offsets) if as_offsets else JaggedTensor(values=v, lengths=lens)
            got = jt.to_padded_dense(desired_length=want.shape[1], padding_value=10.5, pad_from_beginning=bool(pad),
                                     chop_from_beginning=bool(chop))
            assert got.dtype == torch.float32 and got.device.type == torch.device(device).type
            np.testing.assert_array_equal(got.cpu().numpy(), want.astype(np.float32), err_msg=f"{case} {pad}{chop}")
            n += 1
    assert n == 16


def check_padded_dense_edges(device):
    dev = torch.device(device)
    for dtype in (torch.int32, torch.int64, torch.float32):
        jt = JaggedTensor(values=torch.tensor([1, 2, 3, 4, 5, 6, 7, 8], dtype=dtype, device=dev),
                          offsets=torch.tensor([0, 2, 2, 3, 4, 5, 8], device=dev))
        got = jt.to_padded_dense(desired_length=2, padding_value=10.0, pad_from_beginning=False)  # the docstring's example
        assert got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy(), [[1, 2], [10, 10], [3, 10], [4, 10], [5, 10], [7, 8]])
        np.testing.assert_array_equal(jt.to_padded_dense(desired_length=1).cpu().numpy(), [[2], [0], [3], [4], [5], [8]])
        longest = jt.to_padded_dense(chop_from_beginning=False)  # desired_length=None: the longest bag, 3
        np.testing.assert_array_equal(longest.cpu().numpy(),
                                      [[0, 1, 2], [0, 0, 0], [0, 0, 3], [0, 0, 4], [0, 0, 5], [6, 7, 8]])
        empty = JaggedTensor(values=torch.zeros(0, dtype=dtype, device=dev), lengths=torch.zeros(4, dtype=torch.int32, device=dev))
        np.testing.assert_array_equal(empty.to_padded_dense(desired_length=3, padding_value=-1.5).cpu().numpy(),
                                      np.full((4, 3), -1.5, np.float32))
        assert tuple(empty.to_padded_dense().shape) == (4, 0)
        none = JaggedTensor(values=torch.zeros(0, dtype=dtype, device=dev), offsets=torch.zeros(1, dtype=torch.int64, device=dev))
        assert tuple(none.to_padded_dense(desired_length=5).shape) == (0, 5)  # the reference's torch.stack raises here
    for dtype in (torch.int32, torch.int64):  # torch's cast: round to nearest even
        big = JaggedTensor(values=torch.tensor([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1], dtype=dtype, device=dev),
                           lengths=torch.tensor([3], device=dev))
        np.testing.assert_array_equal(big.to_padded_dense(desired_length=3).cpu().numpy(), [[16777216.0, 16777220.0, -16777216.0]])


def test_to_padded_dense_on_the_cpu_equals_every_reference_record():
    check_padded_dense_records("cpu")
    check_padded_dense_edges("cpu")
    jt = JaggedTensor(values=torch.tensor([1.5, 2.5], dtype=torch.float64), lengths=torch.tensor([1, 1]))
    assert jt.to_padded_dense(desired_length=2).dtype == torch.float64  # what torch.cat with the float32 padding promotes to
