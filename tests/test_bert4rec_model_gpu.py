"""GPU: torchrec_amd.models.bert4rec on the kernel path (csrc/attention.hip) against the reference's records
(tests/golden/bert4rec.npz, float64 results) within the tolerance tests/test_attention.py measures; autograd plumbing, HIP
graph capture, the kernel dropout's reproducibility, a short training run against the torch path, and peak memory."""
import copy

import numpy as np
import pytest
import torch

import _paths  # noqa: F401
import _attention_ref as R
import _bert4rec_golden as G
from _deepfm_ref import GEMM_TOL
from torchrec_amd.models import bert4rec as M
from test_bert4rec_model import _tol, build_block, build_mha, compare, run_block, run_mha

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", G.cases("mha"))
def test_multi_headed_attention_kernel_path_matches_the_reference_records(case):
    m, valid = build_mha(case, DEV)
    res = run_mha(m, case, G.mask_of(valid, "expand", DEV), DEV)
    assert m.last_path == "kernel"
    compare(res, "mha", case, "f64", _tol())
    again = run_mha(m, case, G.mask_of(valid, "expand", DEV), DEV)
    for n in res:
        np.testing.assert_array_equal(res[n].view(np.uint32), again[n].view(np.uint32), err_msg=n)  # bit-reproducible
    # a materialised mask takes the reference's formula
    res = run_mha(m, case, G.mask_of(valid, "repeat", DEV), DEV)
    assert m.last_path == "torch"
    compare(res, "mha", case, "f64", _tol())


@pytest.mark.parametrize("case", G.cases("block"))
def test_transformer_block_kernel_path_matches_the_reference_records(case):
    m = build_block(case, DEV)
    compare(run_block(m, case, "expand", DEV), "block", case, "f64", _tol())
    assert m.attention.last_path == "kernel"


def build_model(case, **kw):
    """This package's BERT4Rec with the recorded reference state: every name but the item table's is the reference's."""
    z, pre = G.load(), f"model|{case}|"
    vocab, max_len, emb, nhead, layers, training = (int(x) for x in z[pre + "config"])
    dropout = float(z[pre + "dropout"].ravel()[0])
    model = M.BERT4Rec(vocab_size=vocab, max_len=max_len, emb_dim=emb, nhead=nhead, num_layers=layers, dropout=dropout,
                                device=torch.device(DEV), **kw)
    names = [str(n) for n in z[pre + "names"]]
    ours = list(model.state_dict().keys())
    table = "history.ec.embeddings.item_embedding.weight"
    assert [n for n in ours if not n.startswith("history.ec.")] == [n for n in names if n != table]
    ec_keys = [n for n in ours if n.startswith("history.ec.")]
    assert not ec_keys or ours.index(ec_keys[0]) == names.index(table)  # the table is registered where the reference's is
    missing, unexpected = model.load_state_dict({n: torch.from_numpy(z[pre + "sd|" + n]) for n in names if n != table},
                                                strict=False)
    assert not unexpected and all(n.startswith("history.ec.") for n in missing)
    with torch.no_grad():
        model.history.ec.table_weights()["item_embedding"].copy_(torch.from_numpy(z[pre + "sd|" + table]))
    return model.train(bool(training))


@pytest.mark.parametrize("case", G.cases("model"))
def test_bert4rec_matches_the_reference_records(case):
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    z, pre = G.load(), f"model|{case}|"
    model = build_model(case)
    kjt = KeyedJaggedTensor.from_lengths_sync(keys=["item"], values=torch.from_numpy(z[pre + "values"]).to(DEV),
                                              lengths=torch.from_numpy(z[pre + "lengths"]).to(DEV))
    logits = model(kjt)
    d_k = model.emb_dim // model.transformer_blocks[0].attention.num_heads
    assert model.transformer_blocks[0].attention.last_path == ("kernel" if d_k % 4 == 0 else "torch")
    np.testing.assert_allclose(logits.detach().cpu().numpy(), z[pre + "f64|logits"], **GEMM_TOL)
    logits.backward(torch.from_numpy(z[pre + "g"]).to(DEV))
    checked = 0
    for n, p in model.named_parameters():
        key = pre + "f64|grad|" + n
        if key in z:
            want = z[key]
            np.testing.assert_allclose(G.stored_grad(p.grad.cpu().numpy()), want, rtol=GEMM_TOL["rtol"],
                                       atol=GEMM_TOL["atol"] + GEMM_TOL["rtol"] * float(np.abs(want).max()), err_msg=n)
            checked += 1
    assert checked == sum(k.startswith(pre + "f64|grad|") for k in z)


def _mha(dim=32, H=2, p=0.0, seed=0):
    torch.manual_seed(seed)
    return M.MultiHeadedAttention(num_heads=H, dim_model=dim, dropout=p, device=torch.device(DEV))


def test_needs_input_grad_is_honoured_and_no_grad_works():
    from torchrec_amd.models.bert4rec import _FusedAttention

    B, L, H, d = 3, 9, 2, 8
    q, k, v, g = (torch.from_numpy(a.reshape(B, L, H * d)).to(DEV) for a in R.make_inputs(B, H, L, d))
    kv = torch.from_numpy(R.key_valid("per_sample", B, L).astype(np.uint8)).to(DEV)
    full = [t.clone().requires_grad_() for t in (q, k, v)]
    out = _FusedAttention.apply(*full, kv, H, 0.0, 0, 0)
    out.backward(g)
    for i in range(3):
        leaves = [t.clone().requires_grad_(j == i) for j, t in enumerate((q, k, v))]
        _FusedAttention.apply(*leaves, kv, H, 0.0, 0, 0).backward(g)
        assert [t.grad is not None for t in leaves] == [j == i for j in range(3)]
        assert torch.equal(leaves[i].grad, full[i].grad)
    m = _mha()
    x = torch.randn(B, L, 32, device=DEV)
    mask = G.mask_of(R.key_valid("per_sample", B, L), "expand", DEV)
    with torch.no_grad():
        quiet = m(x, x, x, mask=mask)
    assert m.last_path == "kernel" and not quiet.requires_grad
    assert torch.equal(quiet, m(x, x, x, mask=mask).detach())
    # double backward goes through differentiable torch operations
    xr = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(m(xr, xr, xr, mask=mask).square().sum(), xr, create_graph=True)
    assert m.last_path == "kernel"
    gx.sum().backward()
    assert xr.grad is not None and bool(torch.isfinite(xr.grad).all())


def test_forward_and_backward_captured_into_a_hip_graph_replay_the_eager_bits():
    B, L = 4, 33
    m = _mha(64, 2)
    x = torch.randn(B, L, 64, device=DEV).requires_grad_()
    gout = torch.randn(B, L, 64, device=DEV)
    mask = G.mask_of(R.key_valid("per_sample", B, L), "expand", DEV)
    params = list(m.parameters())

    def step():
        return (lambda out: (out, *torch.autograd.grad(out, [x] + params, gout)))(m(x, x, x, mask=mask))

    eager = [t.detach().clone() for t in step()]
    assert m.last_path == "kernel"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    assert m.last_path == "kernel"
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)


def test_kernel_dropout_is_reproducible_under_manual_seed_and_moves_between_calls():
    B, L = 3, 17
    base = _mha(32, 2, p=0.1).train()
    x = torch.randn(B, L, 32, device=DEV)
    torch.manual_seed(5)
    m1 = copy.deepcopy(base)
    first, second = m1(x, x, x).detach(), m1(x, x, x).detach()
    assert m1.last_path == "kernel" and not torch.equal(first, second)
    torch.manual_seed(5)
    m2 = copy.deepcopy(base)
    assert torch.equal(m2(x, x, x).detach(), first) and torch.equal(m2(x, x, x).detach(), second)
    torch.manual_seed(6)
    assert not torch.equal(copy.deepcopy(base)(x, x, x).detach(), first)
    quiet = copy.deepcopy(base).eval()
    assert torch.equal(quiet(x, x, x).detach(), quiet(x, x, x).detach())
    # the gradient uses the forward's mask: a second backward of the same graph gives the same bits
    xr = x.clone().requires_grad_()
    out = m2(xr, xr, xr)
    (g1,) = torch.autograd.grad(out, xr, torch.ones_like(out), retain_graph=True)
    (g2,) = torch.autograd.grad(out, xr, torch.ones_like(out))
    assert torch.equal(g1, g2) and bool(torch.isfinite(g1).all())


def test_four_training_steps_agree_with_the_torch_path():
    from fbgemm_gpu.split_embedding_configs import EmbOptimType
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    vocab, max_len, emb, nhead, layers, B = 50, 8, 16, 2, 2, 6
    fused = {"optimizer": EmbOptimType.ADAM, "learning_rate": 1e-2, "eps": 1e-8, "beta1": 0.9, "beta2": 0.999,
             "weight_decay": 0.0}
    models = []
    for _ in range(2):
        torch.manual_seed(11)
        models.append(M.BERT4Rec(vocab, max_len, emb, nhead, layers, dropout=0.0, device=torch.device(DEV),
                                          fused_params=dict(fused)))
    kernel, twin = models
    with torch.no_grad():
        twin.load_state_dict(kernel.state_dict())
        twin.history.ec.table_weights()["item_embedding"].copy_(kernel.history.ec.table_weights()["item_embedding"])
    for block in twin.transformer_blocks:
        block.attention.kernel_path = False
    dense = lambda m: [p for n, p in m.named_parameters() if not n.startswith("history.ec.")]  # noqa: E731
    opts = [torch.optim.Adam(dense(m), lr=1e-3) for m in models]
    rng = np.random.default_rng(2)
    ce = torch.nn.CrossEntropyLoss()
    for step in range(4):
        lengths = rng.integers(0, max_len + 1, size=B).astype(np.int32)
        lengths[step % B] = 0
        ids = rng.integers(1, vocab, size=int(lengths.sum())).astype(np.int64)
        target = torch.from_numpy(rng.integers(0, vocab, size=(B, max_len))).to(DEV)
        losses = []
        for m, opt in zip(models, opts):
            kjt = KeyedJaggedTensor.from_lengths_sync(["item"], torch.from_numpy(ids).to(DEV), torch.from_numpy(lengths).to(DEV))
            opt.zero_grad()
            loss = ce(m(kjt).reshape(B * max_len, vocab), target.reshape(-1))
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        assert kernel.transformer_blocks[0].attention.last_path == "kernel"
        assert twin.transformer_blocks[0].attention.last_path == "torch"
        torch.testing.assert_close(losses[0], losses[1], rtol=1e-4, atol=1e-5)
    torch.cuda.synchronize()
    torch.testing.assert_close(kernel.history.ec.table_weights()["item_embedding"],
                               twin.history.ec.table_weights()["item_embedding"], rtol=1e-3, atol=2e-5)
    for (n, a), b in zip(((n, p) for n, p in kernel.named_parameters() if not n.startswith("history.ec.")), dense(twin)):
        if n.endswith("attention.linear_layers.1.bias"):
            # The key projection's bias has an exactly zero gradient (softmax ignores a constant added to a whole row of
            # scores) and no output depends on it.  What either path computes there is rounding residue of about 1e-9, which
            # Adam's division by sqrt(v) turns into steps of up to lr with the residue's sign: no two correct implementations
            # agree on it.  Pinned instead: it has moved by no more than the four steps of lr.
            assert float((a.detach() - b.detach()).abs().max()) <= 2 * 4 * 1e-3
            continue
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-3, atol=2e-5, msg=lambda s, n=n: f"{n}: {s}")


def test_kernel_path_peaks_one_score_tensor_below_the_torch_path():
    """A condition, not a measurement: the torch path must keep p_attn [B, H, L, L] for autograd, the kernel path keeps no
    such tensor."""
    B, L, dim, H = 64, 200, 128, 2
    m = _mha(dim, H)
    x = torch.randn(B, L, dim, device=DEV)
    gout = torch.randn(B, L, dim, device=DEV)
    mask = G.mask_of(np.ones((B, L), bool), "expand", DEV)
    peaks = {}
    for path in ("kernel", "torch", "kernel", "torch"):  # the second round is the one that counts: everything is warm
        m.kernel_path = path == "kernel"
        xr = x.clone().requires_grad_()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m(xr, xr, xr, mask=mask).backward(gout)
        torch.cuda.synchronize()
        assert m.last_path == path
        peaks[path] = torch.cuda.max_memory_allocated() - base
        m.zero_grad()
        del xr
    scores = B * H * L * L * 4
    print(f"peak above the inputs: kernel {peaks['kernel'] / 2**20:.1f} MiB, torch {peaks['torch'] / 2**20:.1f} MiB, "
          f"one [B, H, L, L] float32 tensor {scores / 2**20:.1f} MiB")
    assert peaks["torch"] - peaks["kernel"] >= scores
