"""A numpy restatement of the TBE "exact" backward for the row-norm optimizer family (LAMB, PARTIAL_ROWWISE_ADAM,
PARTIAL_ROWWISE_LAMB, LARS_SGD) and gradient clipping, plus the input sets the tests of that family share.

Restatement (`Ref`): per touched table row the contributions of one batch are summed — every element of the output
gradient clamped first, then times the per-sample weight, then divided by the bag length for MEAN; ids outside the table
are skipped — and the formulas of include/tbe_hip.h (tbe_backward_*_ex_*) are applied to the row once.  The `dtype`
switch runs the same code in float64 (the reference of the GPU tests) or float32 (tests/test_fused_optimizers.py: the
two must agree within the GPU tests' tolerance, i.e. that tolerance is not tighter than FP32 arithmetic allows on these
inputs).  EXACT_SGD and EXACT_ROWWISE_ADAGRAD (default weight_decay_mode, no decay) are restated too: the clipping
tests run them.

`restate` applies the same per-row formulas to a GIVEN coalesced gradient and GIVEN initial states: the reference of the
run harness (tests/_bwd_abi.py, tests/test_fused_optimizers_runs_gpu.py), whose designed inputs make the gradient exact,
so that every difference from the float64 result is the optimizer's own arithmetic.  NORM_TOL is the tolerance of those
comparisons; `Ref.drop` is the mutation tests/test_fused_optimizers.py uses to show that NORM_TOL sees a wrong norm.

numpy only; nothing here touches a GPU.
"""
import functools

import numpy as np

SGD, ROWWISE_ADAGRAD, LAMB, PARTIAL_ROWWISE_ADAM, PARTIAL_ROWWISE_LAMB, LARS_SGD = 0, 1, 4, 5, 6, 7  # TBE_OPT_*
NORM_FAMILY = (LAMB, PARTIAL_ROWWISE_ADAM, PARTIAL_ROWWISE_LAMB, LARS_SGD)
OPT_NAMES = {SGD: "EXACT_SGD", ROWWISE_ADAGRAD: "EXACT_ROWWISE_ADAGRAD", LAMB: "LAMB",
             PARTIAL_ROWWISE_ADAM: "PARTIAL_ROWWISE_ADAM", PARTIAL_ROWWISE_LAMB: "PARTIAL_ROWWISE_LAMB", LARS_SGD: "LARS_SGD"}
POOL_SUM, POOL_MEAN, POOL_NONE = 0, 1, 2
RTOL = ATOL = 2e-5  # the project's tolerance for fused-optimizer results (tests/test_tbe_gpu.py)
# rtol = atol of the run harness's comparisons with `restate`.  The gradient is exact there, so only the optimizer's FP32
# arithmetic is left: NORM_F32_ERROR is the worst max |r32 - r64| / (1 + |r64|) of the float32 restatement over every
# configuration of RUN_CONFIGS (weights and states; measured by tests/test_fused_optimizers.py, which asserts it), and the
# kernel differs from that restatement only in the order of the norms' sums (per-lane fmaf chain + butterfly) and in its
# fused multiply-adds: a factor of 8.
NORM_F32_ERROR = 4.3e-7  # measured: 4.257e-7 (PARTIAL_ROWWISE_ADAM at [2048], weights)
NORM_TOL = 8 * NORM_F32_ERROR
assert NORM_TOL <= RTOL
# the norms of each optimizer: |w|, |g|, |u| and the mean(g^2) of the row-wise v
NORMS = {LAMB: ("w", "u"), PARTIAL_ROWWISE_ADAM: ("v",), PARTIAL_ROWWISE_LAMB: ("w", "u", "v"), LARS_SGD: ("w", "g")}

# (momentum1, momentum2) layout per optimizer: "elem" = [rows, D], "row" = [rows], None = absent
STATE_KINDS = {SGD: (None, None), ROWWISE_ADAGRAD: ("row", None), LAMB: ("elem", "elem"),
               PARTIAL_ROWWISE_ADAM: ("elem", "row"), PARTIAL_ROWWISE_LAMB: ("elem", "row"), LARS_SGD: ("elem", None)}


def hyper(code, weight_decay=0.0, **over):
    """The hyper-parameters the tests use for optimizer `code` (keyword names of SplitTableBatchedEmbeddingBagsCodegen).
    LARS_SGD: eta = 0.02, momentum = 0.9, and a learning rate of 1 so that its steps (lr * eta * |w| / |g|) are well above
    the comparison's absolute tolerance."""
    h = dict(learning_rate=1.0 if code == LARS_SGD else 0.05, eps=1e-3 if weight_decay else 1e-8, weight_decay=weight_decay,
             beta1=0.9, beta2=0.999, eta=0.02, momentum=0.9)
    h.update(over)
    return h


class Ref:
    """Tables + optimizer state of one module, advanced by `step`."""

    def __init__(self, rows, dims, ftm, weights, code, dtype=np.float64, learning_rate=0.05, eps=1e-8, weight_decay=0.0,
                 beta1=0.9, beta2=0.999, eta=0.001, momentum=0.9, max_gradient=None):
        self.rows, self.dims = list(rows), list(dims)
        self.ftm = list(ftm) if ftm is not None else list(range(len(rows)))
        self.code, self.dtype = int(code), np.dtype(dtype)
        self.lr, self.eps, self.wd, self.b1, self.b2 = learning_rate, eps, weight_decay, beta1, beta2
        self.eta, self.momentum, self.max_gradient = eta, momentum, max_gradient
        self.w = [np.array(w, dtype=self.dtype) for w in weights]
        shape = {"elem": lambda r, d: (r, d), "row": lambda r, d: (r,)}
        self.state = [None if k is None else [np.zeros(shape[k](r, d), dtype=self.dtype) for r, d in zip(rows, dims)]
                      for k in STATE_KINDS[self.code]]
        self.t = 0
        self.drop = None  # a name of NORMS: that sum of squares leaves out the row's last column (a wrong kernel, restated)

    # -- the coalesced gradient -------------------------------------------------------------------------------------
    def coalesce(self, indices, offsets, grad, psw=None, pooling=POOL_SUM):
        """(dense gradient per table, touched-row mask per table)"""
        F = len(self.ftm)
        B = (offsets.size - 1) // F
        g = np.asarray(grad, dtype=self.dtype)
        if self.max_gradient is not None:
            g = np.clip(g, -self.max_gradient, self.max_gradient)
        G = [np.zeros((r, d), dtype=self.dtype) for r, d in zip(self.rows, self.dims)]
        touched = [np.zeros(r, dtype=bool) for r in self.rows]
        col = 0
        for f in range(F):
            t = self.ftm[f]
            D = self.dims[t]
            for b in range(B):
                s, e = int(offsets[f * B + b]), int(offsets[f * B + b + 1])
                for p in range(s, e):
                    i = int(indices[p])
                    if i < 0 or i >= self.rows[t]:
                        continue
                    c = g[p, :D] if pooling == POOL_NONE else g[b, col:col + D]
                    if psw is not None:
                        c = c * self.dtype.type(psw[p])
                    if pooling == POOL_MEAN:
                        c = c / self.dtype.type(e - s)
                    G[t][i] += c
                    touched[t][i] = True
            col += D
        return G, touched

    # -- one train step ---------------------------------------------------------------------------------------------
    def step(self, indices, offsets, grad, psw=None, pooling=POOL_SUM):
        self.t += 1
        G, touched = self.coalesce(indices, offsets, grad, psw, pooling)
        for t in range(len(self.rows)):
            R = np.nonzero(touched[t])[0]
            if R.size:
                self._apply(t, R, G[t][R])

    def apply_coalesced(self, G, touched, iteration):
        """One step from a GIVEN coalesced gradient: G[t] is table t's dense gradient (cast to this Ref's dtype: the run
        harness's gradients are exact in either), touched[t] the rows ids name (updated even where G is zero), and
        `iteration` the step count of the bias correction (tbe_optimizer_args.iteration)."""
        self.t = int(iteration)
        for t in range(len(self.rows)):
            R = np.asarray(touched[t], dtype=np.int64)
            if R.size:
                self._apply(t, R, np.asarray(G[t], dtype=self.dtype)[R])
        return self

    def _apply(self, t, R, g):
        lr, eps, wd, b1, b2 = self.lr, self.eps, self.wd, self.b1, self.b2
        w = self.w[t][R]
        D = w.shape[1]

        def sumsq(x, which):
            return (x * x)[:, :D - 1 if self.drop == which else D].sum(axis=1)

        def norm(x, which):
            return np.sqrt(sumsq(x, which))

        def ratio(num, den):  # num / den where both are > 0, else 1
            ok = (num > 0) & (den > 0)
            return np.where(ok, num / np.where(ok, den, 1), 1).astype(self.dtype)

        if self.code == SGD:
            self.w[t][R] = w - lr * g
        elif self.code == ROWWISE_ADAGRAD:
            m = self.state[0][t][R] + (g * g).sum(axis=1) / D
            self.state[0][t][R] = m
            self.w[t][R] = w - (lr / (np.sqrt(m) + eps))[:, None] * g
        elif self.code == LARS_SGD:
            wn, gn = norm(w, "w"), norm(g, "g")
            ok = (wn > 0) & (gn > 0)
            alr = np.where(ok, lr * self.eta * wn / np.where(ok, gn + wd * wn, 1), lr).astype(self.dtype)
            m1 = self.momentum * self.state[0][t][R] + alr[:, None] * (g + wd * w)
            self.state[0][t][R] = m1
            self.w[t][R] = w - m1
        else:
            m1 = b1 * self.state[0][t][R] + (1 - b1) * g
            self.state[0][t][R] = m1
            if self.code == LAMB:
                m2 = b2 * self.state[1][t][R] + (1 - b2) * g * g
                self.state[1][t][R] = m2
                den = np.sqrt(m2) + eps
            else:
                v = b2 * self.state[1][t][R] + (1 - b2) * sumsq(g, "v") / D
                self.state[1][t][R] = v
                if self.code == PARTIAL_ROWWISE_ADAM:
                    den = (np.sqrt(v / (1 - b2 ** self.t)) + eps)[:, None]
                else:
                    den = (np.sqrt(v) + eps)[:, None]
            if self.code == PARTIAL_ROWWISE_ADAM:
                self.w[t][R] = w - lr * ((m1 / (1 - b1 ** self.t)) / den + wd * w)
            else:
                u = m1 / den + wd * w
                self.w[t][R] = w - lr * ratio(norm(w, "w"), norm(u, "u"))[:, None] * u
        for a in [self.w[t]] + [s[t] for s in self.state if s is not None]:
            assert a.dtype == self.dtype  # a float32 run must not be promoted on the way


def restate(code, init, G, touched, iteration, dtype=np.float64, drop=None, **hyper):
    """`Ref`'s formulas applied once to the coalesced gradient G (_bwd_abi.coalesced_grad_f64) from the initial weights
    and states `init` (BackwardCase.init: "weights", "state0", "state1").  Returns the Ref: .w and .state hold the result.
    float64 is the reference of the run harness, float32 the margin check; `drop` mutates one norm (Ref.drop)."""
    rows, dims = [w.shape[0] for w in init["weights"]], [w.shape[1] for w in init["weights"]]
    ref = Ref(rows, dims, None, [np.asarray(w, dtype=np.float32) for w in init["weights"]], code, dtype=np.dtype(dtype), **hyper)
    for k, kind in enumerate(STATE_KINDS[ref.code]):
        if kind is not None:
            given = init["state%d" % k]
            assert [a.shape for a in given] == [a.shape for a in ref.state[k]]
            ref.state[k] = [np.array(a, dtype=ref.dtype) for a in given]
    ref.drop = drop
    return ref.apply_coalesced(G, touched, iteration)


# ---- the configurations of the run harness (tests/test_fused_optimizers_runs_gpu.py) -----------------------------------
# sort payload: the bag number alone (narrow) or (bag, position) (wide: per-sample weights) -> (weighted, pooling)
RUN_PAYLOADS = {"narrow_sum": (False, POOL_SUM), "wide_sum": (True, POOL_SUM), "wide_mean": (True, POOL_MEAN)}
# one per dispatch class of run_apply (max_D <= 64, 128, 256, 512, 1024, 2048) + odd dims under a larger max_D + a table
# 4 B off the 16-B grid ([40, 12]: its second table); the payloads are spread over them
RUN_DIMS = [([64], "narrow_sum"), ([128], "wide_sum"), ([256], "wide_mean"), ([512], "narrow_sum"), ([1024], "wide_sum"),
            ([2048], "wide_mean"), ([7, 13], "narrow_sum"), ([13, 260], "wide_mean"), ([40, 12], "wide_sum")]
RUN_ITERATION = 3
RUN_CLIP = 1.5  # keeps every clamped term a multiple of 1/16 (tests/test_backward_run_inputs.py)


def run_hyper(code, weight_decay=0.0):
    """Hyper-parameters of the run harness: steps large enough, and a beta2 small enough, that a column missing from any
    one norm moves a weight or a state out of NORM_TOL (tests/test_fused_optimizers.py asserts it)."""
    h = dict(learning_rate=1.0 if code == LARS_SGD else 0.5, eps=1e-3 if weight_decay else 1e-8,
             weight_decay=weight_decay, beta1=0.9, beta2=0.5, eta=0.02, momentum=0.9)
    return {k: float(np.float32(v)) for k, v in h.items()}  # the values the C ABI's float fields hold


def norm_error(got, want):
    """|got - want| / (NORM_TOL + NORM_TOL |want|), element-wise: <= 1 is inside the run harness's tolerance."""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / (NORM_TOL + NORM_TOL * np.abs(want))


def _run_configs():
    out = []
    for i, (dims, payload) in enumerate(RUN_DIMS):  # every finishing path, every dispatch class (layout MIXED)
        for code, wd in zip(NORM_FAMILY, (0.0, 0.01, 0.0, 0.01) if i % 2 == 0 else (0.01, 0.0, 0.01, 0.0)):
            out.append(("MIXED", tuple(dims), payload, code, wd, None))
    for layout in ("ALIGNED", "OPEN_TAIL", "INVALID_TAIL"):
        for dims, payload in (([128], "wide_sum"), ([13, 260], "wide_mean")):
            out += [(layout, tuple(dims), payload, LAMB, 0.01, None), (layout, tuple(dims), payload, LARS_SGD, 0.0, None)]
    for dims, payload in (([128], "narrow_sum"), ([13, 260], "wide_mean")):  # clipping
        out += [("MIXED", tuple(dims), payload, LAMB, 0.0, RUN_CLIP), ("MIXED", tuple(dims), payload, PARTIAL_ROWWISE_ADAM, 0.01, RUN_CLIP)]
    return out


# every (layout, dims, payload, optimizer, weight decay, clipping bound) the run harness compares with `restate`
RUN_CONFIGS = _run_configs()


def run_config_id(cfg):
    layout, dims, payload, code, wd, clip = cfg
    return f"{layout}-d{'_'.join(map(str, dims))}-{payload}-{OPT_NAMES[code]}-wd{wd}" + (f"-clip{clip}" if clip is not None else "")


def run_inputs(layout, dims, payload, clip=None):
    """The designed batch of a run-harness configuration; with a clipping bound, the same batch with the output gradient
    clamped (what the kernel does to every element it loads)."""
    import _bwd_abi

    inp = _bwd_abi.make_inputs(layout, list(dims), weighted=RUN_PAYLOADS[payload][0])
    return inp if clip is None else _bwd_abi.with_grad(inp, np.clip(inp.grad, -clip, clip))


@functools.lru_cache(maxsize=4)
def _run_gradient(layout, dims, payload, clip):
    import _bwd_abi

    inp = run_inputs(layout, dims, payload, clip)
    tabs = _bwd_abi.BackwardCase(inp.rows, list(dims)).oracle_tables()[0]
    G = _bwd_abi.coalesced_grad_f64(inp, tabs, RUN_PAYLOADS[payload][1])
    for g in G:
        g.setflags(write=False)
    return G


def run_reference(cfg, init, dtype=np.float64, drop=None, touched=None):
    """`restate` for a run-harness configuration from the initial arrays `init` (BackwardCase.init)."""
    layout, dims, payload, code, wd, clip = cfg
    inp = run_inputs(layout, dims, payload, None)
    G = _run_gradient(layout, dims, payload, clip)
    return restate(code, init, G, inp.touched if touched is None else touched, RUN_ITERATION, dtype, drop,
                   max_gradient=None, **run_hyper(code, wd))


RUN_GUARD_CODES = (LAMB, PARTIAL_ROWWISE_LAMB, LARS_SGD)


def run_guard_case(code):
    """The trust-ratio guards on rows that the BLOCK fix-up finishes (layout MIXED, [128], narrow sum, no decay): of the
    rows whose chain is longer than kLongChain chunks, the one with the shortest run gets an all-zero coalesced gradient
    (every bag that names it has a zero output gradient) and the next one all-zero weights; both start from zero states,
    so |g| = |u| = 0 on the first and |w| = 0 on the second.
    Returns (cfg, inputs, init for BackwardCase(init=...), zero-gradient row, zero-weight row)."""
    import _bwd_abi

    cfg = ("MIXED", (128,), "narrow_sum", code, 0.0, None)
    base = run_inputs(*cfg[:3])
    case = _bwd_abi.BackwardCase(base.rows, [128], code=code)
    paths = _bwd_abi.finishing_paths(base, case.oracle_tables()[0])[0]
    runs_of_row = np.zeros(base.rows[0], dtype=np.int64)
    runs_of_row[base.touched[0]] = base.runs
    block = [int(r) for r in base.touched[0] if paths[r] == _bwd_abi.BLOCK_FIXUP]
    zero_g, zero_w = sorted(block, key=lambda r: runs_of_row[r])[:2]
    grad = np.array(base.grad)
    grad[np.unique(_bwd_abi.bag_of_position(base)[base.indices == zero_g])] = 0.0
    init = {k: None if v is None else [np.array(a) for a in v] for k, v in case.init.items()}
    init["weights"][0][zero_w] = 0.0
    for k in ("state0", "state1"):
        if init[k] is not None:
            init[k][0][[zero_g, zero_w]] = 0.0
    return cfg, _bwd_abi.with_grad(base, grad), init, zero_g, zero_w


def run_guard_reference(code, dtype=np.float64):
    import _bwd_abi

    cfg, inp, init, _, _ = run_guard_case(code)
    tabs = _bwd_abi.BackwardCase(inp.rows, [128]).oracle_tables()[0]
    G = _bwd_abi.coalesced_grad_f64(inp, tabs, POOL_SUM)
    return restate(code, init, G, inp.touched, RUN_ITERATION, dtype, **run_hyper(code, 0.0))


# ---- the shared input sets -------------------------------------------------------------------------------------------
class Case:
    """One input set: tables, initial weights and `steps` batches (indices, offsets, psw, grad).  Read-only: shared."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _lengths(rng, n, lo, hi, fixed):
    return np.full(n, fixed, dtype=np.int64) if fixed is not None else rng.integers(lo, hi + 1, size=n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(name, steps=2):
    """The shapes of the family's tests: the smallest at which each kernel path can go wrong.
    a      (7, 8) + (40, 36), SUM, B = 5, bags of 0-3: masked tail columns, 16-lane groups, duplicates, empty bags
    b64    (3, 128), SUM, B = 64, bags of 4: 256 ids into 3 rows — runs longer than the 32-id chunk (wave fix-up)
    b1024  the same table at B = 1024: chains longer than 24 chunks (block fix-up)
    c      (50, 520), MEAN, weighted, B = 6, bags of 0-3: two float4 per lane
    d      (20, 64), PoolingMode.NONE, B = 9, bags of 0-3: the sequence path
    u128   (30, 128) + (11, 128), SUM, B = 16, bags of 1-3: uniform and aligned — a FAST kernel's shape (clipping)
    Runs that start or end on a chunk edge, rows finished by all three paths in one launch, the dispatch classes 256, 1024
    and 2048, 64-bit keys and misaligned tables are the run harness's (RUN_CONFIGS below, tests/_bwd_abi.py,
    tests/test_fused_optimizers_runs_gpu.py)."""
    spec = {
        "a": dict(rows=[7, 40], dims=[8, 36], pooling=POOL_SUM, B=5, lo=0, hi=3, fixed=None, weighted=False),
        "b64": dict(rows=[3], dims=[128], pooling=POOL_SUM, B=64, lo=0, hi=0, fixed=4, weighted=False),
        "b1024": dict(rows=[3], dims=[128], pooling=POOL_SUM, B=1024, lo=0, hi=0, fixed=4, weighted=False),
        "c": dict(rows=[50], dims=[520], pooling=POOL_MEAN, B=6, lo=0, hi=3, fixed=None, weighted=True),
        "d": dict(rows=[20], dims=[64], pooling=POOL_NONE, B=9, lo=0, hi=3, fixed=None, weighted=False),
        "u128": dict(rows=[30, 11], dims=[128, 128], pooling=POOL_SUM, B=16, lo=1, hi=3, fixed=None, weighted=False),
    }[name]
    rows, dims, B = spec["rows"], spec["dims"], spec["B"]
    rng = np.random.default_rng([7, sorted("a b64 b1024 c d u128".split()).index(name)])
    weights = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    batches = []
    for _ in range(steps):
        lengths = _lengths(rng, len(rows) * B, spec["lo"], spec["hi"], spec["fixed"])
        indices = np.concatenate([rng.integers(0, rows[f], size=int(lengths[f * B:(f + 1) * B].sum()))
                                  for f in range(len(rows))]).astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        psw = (rng.random(indices.size).astype(np.float32) + 0.5) if spec["weighted"] else None
        shape = (indices.size, dims[0]) if spec["pooling"] == POOL_NONE else (B, sum(dims))
        grad = rng.standard_normal(shape).astype(np.float32)
        batches.append((indices, offsets, psw, grad))
    for a in weights + [x for b in batches for x in b if x is not None]:
        a.setflags(write=False)
    return Case(name=name, rows=rows, dims=dims, ftm=None, pooling=spec["pooling"], B=B, weights=weights, batches=batches)


@functools.lru_cache(maxsize=None)
def guard_case():
    """The trust-ratio guards: one (6, 8) table, SUM, B = 4, two steps.  Row 0 starts as all zeros (|w| = 0) and is
    touched with a non-zero gradient; row 1 is touched only by bags whose output gradient is all zero (|g| = 0, and with
    zero state and no weight decay |u| = 0); rows 2 and 3 are ordinary."""
    rng = np.random.default_rng(23)
    w = rng.standard_normal((6, 8)).astype(np.float32)
    w[0] = 0.0
    batches = []
    for _ in range(2):
        indices = np.array([0, 2, 1, 1, 1, 3], dtype=np.int64)  # bags: [0, 2] [1] [1, 1] [3]
        offsets = np.array([0, 2, 3, 5, 6], dtype=np.int64)
        grad = rng.standard_normal((4, 8)).astype(np.float32)
        grad[1] = 0.0
        grad[2] = 0.0
        batches.append((indices, offsets, None, grad))
    for a in [w] + [x for b in batches for x in b if x is not None]:
        a.setflags(write=False)
    return Case(name="guards", rows=[6], dims=[8], ftm=None, pooling=POOL_SUM, B=4, weights=[w], batches=batches)


@functools.lru_cache(maxsize=None)
def reference(case_name, code, weight_decay=0.0, max_gradient=None, dtype="float64", upcast_f16=False):
    """The restatement after every batch of the named input set: a Ref (shared: do not modify).  upcast_f16: the tables
    start as float(half(w)), what an FP16 module holds."""
    c = guard_case() if case_name == "guards" else case(case_name)
    weights = [w.astype(np.float16).astype(np.float32) for w in c.weights] if upcast_f16 else c.weights
    ref = Ref(c.rows, c.dims, c.ftm, weights, code, dtype=np.dtype(dtype), max_gradient=max_gradient,
              **hyper(code, weight_decay))
    for indices, offsets, psw, grad in c.batches:
        ref.step(indices, offsets, grad, psw, c.pooling)
    return ref


# every (input set, optimizer, weight decay, clipping bound) the GPU tests compare with the restatement
GPU_CONFIGS = (
    [(n, code, wd, None) for n in ("a", "b64", "b1024", "c", "d") for code, wd in
     zip(NORM_FAMILY, (0.0, 0.01, 0.0, 0.01) if n in ("a", "c", "b1024") else (0.01, 0.0, 0.01, 0.0))]
    + [("guards", code, 0.0, None) for code in (LAMB, PARTIAL_ROWWISE_LAMB, LARS_SGD)]
    + [("u128", SGD, 0.0, 0.5), ("u128", ROWWISE_ADAGRAD, 0.0, 0.5), ("a", LAMB, 0.0, 0.5),
       ("c", PARTIAL_ROWWISE_ADAM, 0.01, 0.5)]  # the last one: weighted MEAN with clipping (clamp before weight and division)
)
