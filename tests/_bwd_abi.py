"""The TBE backward driven straight through the C ABI (include/tbe_hip.h), plus inputs designed around its chunk grid.

Two halves:

* `make_inputs` builds ids whose sorted runs meet the update kernel's chunk grid at chosen phases (csrc/
  tbe_backward_impl.hpp cuts the sorted contributions into chunks of `pick_chunk(N)` ids and finishes runs that cross a
  chunk boundary in `bwd_fixup_kernel`), with values for which every summation order is exact in FP32: integer
  gradients in [-4, 4], per-sample weights in {0.5, 1, 2} and bag lengths in {1, 2, 4}, so each term is a multiple of
  1/8 and |sum| * 8 stays far below 2^24.  A dropped, doubled or misattributed contribution moves a sum by >= 1/8, and a
  GPU result can be compared with the FP32 oracle bit for bit at any run length.  numpy only: the CPU guard of that
  premise (tests/test_backward_run_inputs.py) imports this half.
* `BackwardCase` lays tables and optimizer state in one flat device buffer between guard bytes, builds the feat_*
  arrays (a `row_base_shift` of 2^33 gives 64-bit sort keys, which the Python module only reaches with 2^32 rows), and
  runs `tbe_backward_fused_*` or `tbe_backward_prepare` + `tbe_backward_apply_*` with an explicit `flags` word.  The
  row-norm family (codes 4-7), an `ext=` (tbe_optimizer_ext) or `force_ex=True` take the `_ex` twins of those entries.
"""
import ctypes
import functools

import numpy as np

import _paths  # noqa: F401
from oracle import oracle

FLAG_UNIFORM_ALIGNED, FLAG_WEIGHTED = 1, 2  # TBE_FLAG_*
ROUND_NEAREST_EVEN, ROUND_STOCHASTIC = 0, 1  # TBE_ROUND_*

# What pick_chunk gives up to N = 524 288 and where bwd_fixup_kernel hands a chain to the whole workgroup
# (kLongChain).  Used ONLY to name the path that finished a row when a comparison fails; no expected value depends on it.
CHUNK, LONG_CHAIN = 32, 24
IN_CHUNK, WAVE_FIXUP, BLOCK_FIXUP = 0, 1, 2
PATH_NAMES = {IN_CHUNK: "in-chunk", WAVE_FIXUP: "wave fix-up", BLOCK_FIXUP: "block fix-up"}

MIXED_RUNS = [1, 31, 32, 33, 63, 64, 65, 1, 255, 256, 257, 767, 768, 769, 799, 800, 801, 832, 833, 3000, 5, 32, 32, 31, 1]
ALIGNED_RUNS = [32, 64, 32, 768, 800, 832, 32, 1600, 256]
BIG_RUNS = [1536, 1537, 1600, 1601, 63, 64, 65, 127, 128, 129]
BIG_N = 530000  # > 524 288: the chunk is 64 there
# name -> (designed runs in key order, out-of-range ids per feature)
LAYOUTS = {
    "MIXED": (MIXED_RUNS, 0),  # boundaries at mixed phases, chains of 1 .. 93 chunks, both sides of 24
    "ALIGNED": (ALIGNED_RUNS, 0),  # every run starts and ends on the chunk grid
    "OPEN_TAIL": (ALIGNED_RUNS + [3017], 0),  # a long chain ends at N, N % 32 != 0
    "INVALID_TAIL": (MIXED_RUNS + [1000], 40),  # sentinel keys share the last chunks with the tail of a real run
    "BIG": (BIG_RUNS + [1] * (BIG_N - sum(BIG_RUNS)), 0),
}


class Inputs:
    """One designed batch.  Arrays are read-only: tests share them."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._dev = None


def _bag_lengths(rng, n):
    """Lengths from {1, 2, 4} that sum to n: the last bag is clipped to what is left, a clipped 3 becomes 2 (+ a bag of 1)."""
    draw = rng.choice(np.array([1, 2, 4], dtype=np.int64), size=n)
    cs = np.cumsum(draw)
    k = int(np.searchsorted(cs, n))  # first bag that reaches n
    left = n - (int(cs[k - 1]) if k > 0 else 0)
    tail = [2, 1] if left == 3 else [left]
    return np.concatenate([draw[:k], np.array(tail, dtype=np.int64)])


@functools.lru_cache(maxsize=6)
def _make_inputs(layout, dims, ftm, weighted, nobag, seed):
    runs, n_bad = LAYOUTS[layout]
    runs = np.asarray(runs, dtype=np.int64)
    T, F = len(dims), len(ftm)
    rng = np.random.default_rng([seed, sorted(LAYOUTS).index(layout), F, T])
    rows = [len(runs) + 11 + 3 * t for t in range(T)]  # spare rows no id names
    touched = [np.sort(rng.choice(rows[t], size=len(runs), replace=False)).astype(np.int64) for t in range(T)]
    n_f = int(runs.sum()) + n_bad
    base_len = np.ones(n_f, dtype=np.int64) if layout == "BIG" else _bag_lengths(rng, n_f)
    B = int(base_len.size)
    ids, lengths = [], []
    for f in range(F):
        t = ftm[f]
        v = np.repeat(touched[t], runs)
        bad = np.where(np.arange(n_bad) % 2 == 0, -1, rows[t]).astype(np.int64)  # below and just past the table
        v = np.concatenate([v, bad])
        rng.shuffle(v)
        ids.append(v)
        lengths.append(rng.permutation(base_len))
    indices = np.concatenate(ids)
    offsets = np.concatenate([[0], np.cumsum(np.concatenate(lengths))]).astype(np.int64)
    N = int(indices.size)
    feat_D = [dims[t] for t in ftm]
    shape = (N, dims[0]) if nobag else (B, int(sum(feat_D)))
    grad = rng.integers(-4, 5, size=shape).astype(np.float32)
    psw = rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=N) if weighted else None
    for a in (indices, offsets, grad, psw):
        if a is not None:
            a.setflags(write=False)
    return Inputs(layout=layout, dims=list(dims), ftm=list(ftm), rows=rows, touched=touched, runs=runs, n_bad=n_bad,
                  F=F, B=B, N=N, indices=indices, offsets=offsets, grad=grad, psw=psw, nobag=nobag)


def make_inputs(layout, dims, ftm=None, weighted=False, nobag=False, seed=0):
    """Row touched[t][r] of table t receives runs[r] contributions from every feature of that table, shuffled over bags.
    Every table has the same runs; pooled gradients are [B, sum feat_D], PoolingMode.NONE gradients [N, D]."""
    ftm = tuple(ftm) if ftm is not None else tuple(range(len(dims)))
    return _make_inputs(layout, tuple(dims), ftm, bool(weighted), bool(nobag), seed)


def with_grad(inp, grad):
    """`inp` with another output gradient of the same shape (read-only, like the rest); nothing is shared on the device."""
    grad = np.ascontiguousarray(grad, dtype=np.float32)
    assert grad.shape == inp.grad.shape
    grad.setflags(write=False)
    kw = {k: v for k, v in inp.__dict__.items() if k != "_dev"}
    return Inputs(**dict(kw, grad=grad))


def feature_of_position(inp):
    return np.repeat(np.arange(inp.F), np.diff(inp.offsets[::inp.B]))


def bag_of_position(inp):
    return np.repeat(np.arange(inp.F * inp.B), np.diff(inp.offsets))


def valid_keys(inp, tabs):
    """(global row key, position) of every in-range id, in position order."""
    f = feature_of_position(inp)
    ok = (inp.indices >= 0) & (inp.indices < tabs.feat_rows[f])
    pos = np.nonzero(ok)[0]
    return tabs.feat_row_base[f[pos]] + inp.indices[pos], pos


def coalesced_grad_f64(inp, tabs, pooling):
    """The dense gradient of every table in float64: np.add.at on the global row key, table by table."""
    keys, pos = valid_keys(inp, tabs)
    f = feature_of_position(inp)[pos]
    bag = bag_of_position(inp)[pos]
    w = np.ones(pos.size) if inp.psw is None else inp.psw[pos].astype(np.float64)
    if pooling == oracle.POOL_MEAN:
        w = w / np.diff(inp.offsets)[bag]
    out = [np.zeros((r, d)) for r, d in zip(tabs.rows, tabs.dims)]
    table_base = {t: int(tabs.feat_row_base[tabs.ftm.index(t)]) for t in set(tabs.ftm)}
    for ff in range(inp.F):
        sel = np.nonzero(f == ff)[0]
        t, D = tabs.ftm[ff], int(tabs.feat_D[ff])
        if inp.nobag:
            g = inp.grad[pos[sel]].astype(np.float64)
        else:
            c0 = int(tabs.feat_D_offset[ff])
            g = inp.grad[bag[sel] - ff * inp.B, c0:c0 + D].astype(np.float64)
        np.add.at(out[t], keys[sel] - table_base[t], w[sel, None] * g)
    return out


def finishing_paths(inp, tabs):
    """Per table, per row: which stage of the backward finishes the row (-1: no id names it), from where its run lies on
    the chunk grid of the sorted keys."""
    keys, _ = valid_keys(inp, tabs)
    uniq, start, count = np.unique(np.sort(keys), return_index=True, return_counts=True)
    following = (start + count - 1) // CHUNK - start // CHUNK
    path = np.where(following == 0, IN_CHUNK, np.where(following <= LONG_CHAIN, WAVE_FIXUP, BLOCK_FIXUP))
    out = [np.full(r, -1, dtype=np.int64) for r in tabs.rows]
    for t in set(tabs.ftm):
        base = int(tabs.feat_row_base[tabs.ftm.index(t)])
        sel = (uniq >= base) & (uniq < base + tabs.rows[t])
        out[t][uniq[sel] - base] = path[sel]
    return out


# ---- the GPU half ----------------------------------------------------------------------------------------------------
GUARD_ELEMS = 64
GUARD_BYTE = 0xC3


OPT_LAMB, OPT_PARTIAL_ROWWISE_ADAM, OPT_PARTIAL_ROWWISE_LAMB, OPT_LARS_SGD = 4, 5, 6, 7  # TBE_OPT_*: the _ex entries only
NORM_FAMILY = (OPT_LAMB, OPT_PARTIAL_ROWWISE_ADAM, OPT_PARTIAL_ROWWISE_LAMB, OPT_LARS_SGD)


def opt_args(code, lr, eps=1e-8, weight_decay=0.0, beta1=0.9, beta2=0.999, iteration=1):
    from fbgemm_gpu._lib import OptimizerArgs

    return OptimizerArgs(int(code), lr, eps, weight_decay, beta1, beta2, iteration)


def opt_ext(momentum=0.0, eta=0.0, max_gradient=None):
    """tbe_optimizer_ext; max_gradient None = no clipping."""
    from fbgemm_gpu._lib import OptimizerExt

    return OptimizerExt(momentum, eta, 0.0 if max_gradient is None else max_gradient, int(max_gradient is not None))


class Result:
    def __init__(self, weights, state0, state1, bounds, guards_ok):
        self.weights, self.state0, self.state1, self.bounds, self.guards_ok = weights, state0, state1, bounds, guards_ok


def _state_shapes(code, rows, dims):
    """(shapes of state0, shapes of state1) per table for optimizer `code` (include/tbe_hip.h feat_state0/1)."""
    per_elem = [(r, d) for r, d in zip(rows, dims)]
    if code == oracle.OPT_EXACT_ROWWISE_ADAGRAD:
        return [(r,) for r in rows], None
    if code in (oracle.OPT_EXACT_ADAGRAD, oracle.OPT_DENSE_GRAD):
        return per_elem, None
    if code in (oracle.OPT_ADAM, OPT_LAMB):
        return per_elem, per_elem
    if code in (OPT_PARTIAL_ROWWISE_ADAM, OPT_PARTIAL_ROWWISE_LAMB):
        return per_elem, [(r,) for r in rows]
    if code == OPT_LARS_SGD:
        return per_elem, None
    return None, None


class BackwardCase:
    """Tables (+ the state arrays optimizer `code` needs) in ONE flat device buffer: every array starts 16-B aligned —
    4 B further for the tables listed in `misalign` — and is followed by GUARD_ELEMS elements of GUARD_BYTE bytes; the
    gaps before it hold the same byte.  `run` starts from the same initial bytes every time."""

    def __init__(self, rows, dims, ftm=None, row_base_shift=0, dtype="float32", code=oracle.OPT_EXACT_SGD, misalign=(),
                 seed=0, init=None):
        self.rows, self.dims = [int(r) for r in rows], [int(d) for d in dims]
        self.ftm = list(ftm) if ftm is not None else list(range(len(rows)))
        self.F, self.T = len(self.ftm), len(self.rows)
        self.dtype, self.code, self.shift = np.dtype(dtype), int(code), int(row_base_shift)
        self.max_D = max(self.dims[t] for t in self.ftm)
        rng = np.random.default_rng([seed, self.T, self.max_D])
        if init is None:
            w = [rng.standard_normal((r, d)).astype(np.float32).astype(self.dtype) for r, d in zip(self.rows, self.dims)]
            sh0, sh1 = _state_shapes(self.code, self.rows, self.dims)

            def states(shapes):
                if shapes is None:
                    return None
                if self.code == oracle.OPT_DENSE_GRAD:
                    return [np.zeros(s, dtype=np.float32) for s in shapes]
                return [rng.uniform(0.5, 1.5, size=s).astype(np.float32) for s in shapes]  # never zero: a used state

            init = {"weights": w, "state0": states(sh0), "state1": states(sh1)}
        self.init = init
        # byte layout
        self._slots = {}  # (kind, table) -> (byte offset, array)
        off = 256
        for kind in ("weights", "state0", "state1"):
            if init[kind] is None:
                continue
            for t, a in enumerate(init[kind]):
                off = (off + 15) // 16 * 16 + (4 if t in misalign else 0)
                self._slots[(kind, t)] = (off, a)
                off += a.nbytes + GUARD_ELEMS * a.itemsize
        self.nbytes = off + 256
        host = np.full(self.nbytes, GUARD_BYTE, dtype=np.uint8)
        self._gap = np.ones(self.nbytes, dtype=bool)
        for o, a in self._slots.values():
            host[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            self._gap[o:o + a.nbytes] = False
        self._host = host
        base = np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int64) + self.shift
        self.feat_row_base = np.array([base[t] for t in self.ftm], dtype=np.int64)
        max_key = int(base[-1]) - 1
        self.key_bits = (max_key + 1).bit_length()  # no valid key equals the all-ones sentinel
        self._dev = None

    def twin_f32(self):
        """The same case with FP32 tables holding float(w16) and the same states."""
        init = dict(self.init, weights=[w.astype(np.float32) for w in self.init["weights"]])
        return BackwardCase(self.rows, self.dims, self.ftm, self.shift, "float32", self.code, init=init)

    def oracle_tables(self):
        """(oracle.Tables with this case's feat_row_base and float32 copies of the weights, state0, state1)"""
        tabs = oracle.Tables(self.rows, self.dims, self.ftm)
        tabs.weights = [np.array(w, dtype=np.float32) for w in self.init["weights"]]
        tabs.feat_row_base = self.feat_row_base.copy()  # a plain attribute; the oracle's keys are int64
        copies = [None if self.init[k] is None else [a.copy() for a in self.init[k]] for k in ("state0", "state1")]
        return tabs, copies[0], copies[1]

    def uniform_aligned(self, stride):
        """Whether TBE_FLAG_UNIFORM_ALIGNED may be asserted (include/tbe_hip.h `flags`)."""
        dims = {self.dims[t] for t in self.ftm}
        aligned = all(o % 16 == 0 for o, _ in self._slots.values())
        return len(dims) == 1 and self.max_D % (8 if self.dtype == np.float16 else 4) == 0 and stride % 4 == 0 and aligned

    def _device(self):
        import torch

        if self._dev is None:
            buf = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0

            def addr(kind):
                if self.init[kind] is None:
                    return None
                return torch.tensor([buf.data_ptr() + self._slots[(kind, t)][0] for t in self.ftm], dtype=torch.int64).cuda()

            feat_D = [self.dims[t] for t in self.ftm]
            self._dev = dict(
                buf=buf, weights=addr("weights"), state0=addr("state0"), state1=addr("state1"),
                feat_D=torch.tensor(feat_D, dtype=torch.int32).cuda(),
                feat_rows=torch.tensor([self.rows[t] for t in self.ftm], dtype=torch.int64).cuda(),
                feat_row_base=torch.tensor(self.feat_row_base).cuda(),
                out_pooled=torch.tensor(np.concatenate([[0], np.cumsum(feat_D)[:-1]]).astype(np.int64)).cuda(),
                out_nobag=torch.zeros(self.F, dtype=torch.int64).cuda(),
                host=torch.tensor(self._host))
        return self._dev

    def run(self, inp, opt, pooling=oracle.POOL_SUM, feat_pooling=None, mode="fused", flags=None,
            rounding=ROUND_NEAREST_EVEN, seed=0, ext=None, force_ex=False):
        """mode "fused": tbe_backward_fused_*; "split": tbe_backward_prepare + tbe_backward_apply_*.  flags None = what a
        host may assert (UNIFORM_ALIGNED where it holds); TBE_FLAG_WEIGHTED is added whenever the batch has weights.
        ext (fbgemm_gpu._lib.OptimizerExt), an optimizer code of the row-norm family or force_ex=True (ext = NULL) call
        the tbe_backward_*_ex_* twin of the same entry."""
        import torch
        from fbgemm_gpu import _lib

        lib, d = _lib.load(), self._device()
        dev = torch.device("cuda", 0)
        if inp._dev is None:
            inp._dev = tuple(None if a is None else torch.tensor(a).cuda() for a in (inp.indices, inp.offsets, inp.psw, inp.grad))
        indices, offsets, psw, grad = inp._dev
        stride = int(inp.grad.shape[1])
        if flags is None:
            flags = FLAG_UNIFORM_ALIGNED if self.uniform_aligned(stride) else 0
        if psw is not None:
            flags |= FLAG_WEIGHTED
        fpool = None if feat_pooling is None else torch.tensor(list(feat_pooling), dtype=torch.int32).cuda()
        out_off = d["out_nobag"] if pooling == oracle.POOL_NONE else d["out_pooled"]
        d["buf"].copy_(d["host"])
        nbytes = lib.tbe_backward_workspace_bytes(inp.N, self.F, inp.B, self.max_D, self.key_bits)
        assert nbytes > 0
        raw = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")  # stale partial rows would read as NaN
        ws = (raw.data_ptr() + 255) // 256 * 256
        bounds = torch.zeros(1, dtype=torch.int32, device="cuda")
        faults = _lib.fault_count()
        st = _lib.stream_ptr(dev)
        p = _lib.ptr
        f16 = self.dtype == np.float16
        ex = ext is not None or force_ex or int(opt.optimizer) in NORM_FAMILY
        name = ("{}_ex_{}" if ex else "{}_{}").format("{}", "f16w" if f16 else "f32")
        ext_arg = ((ctypes.byref(ext) if ext is not None else None),) if ex else ()
        table_args = (p(d["weights"]), p(d["feat_D"]), p(out_off), p(d["feat_rows"]), p(d["feat_row_base"]), p(d["state0"]),
                      p(d["state1"]), self.F, inp.B, self.max_D, self.key_bits, p(indices), inp.N, p(offsets), p(psw),
                      int(pooling), p(fpool), p(grad), stride, opt, flags, ws, nbytes)
        rnd = (int(rounding), int(seed)) if f16 else ()
        if mode == "fused":
            fn = getattr(lib, name.format("tbe_backward_fused"))
            _lib.check(fn(*table_args, p(bounds), None, *rnd, *ext_arg, st), name.format("tbe_backward_fused"))
        else:
            assert mode == "split"
            _lib.check(lib.tbe_backward_prepare(p(d["feat_rows"]), p(d["feat_row_base"]), self.F, inp.B, self.max_D,
                                                self.key_bits, p(indices), inp.N, p(offsets), int(pooling),
                                                flags & FLAG_WEIGHTED, ws, nbytes, p(bounds), None, st), "tbe_backward_prepare")
            fn = getattr(lib, name.format("tbe_backward_apply"))
            _lib.check(fn(*table_args, *rnd, *ext_arg, st), name.format("tbe_backward_apply"))
        torch.cuda.synchronize()
        assert _lib.fault_count() == faults, "the pair sort gave up on a spin-wait"
        after = d["buf"].cpu().numpy()

        def take(kind):
            if self.init[kind] is None:
                return None
            out = []
            for t in range(self.T):
                o, a = self._slots[(kind, t)]
                out.append(after[o:o + a.nbytes].view(a.dtype).reshape(a.shape).copy())
            return out

        return Result(take("weights"), take("state0"), take("state1"), int(bounds.item()),
                      bool((after[self._gap] == GUARD_BYTE).all()))
