"""A numpy restatement of the TBE "exact" backward for the row-norm optimizer family (LAMB, PARTIAL_ROWWISE_ADAM,
PARTIAL_ROWWISE_LAMB, LARS_SGD) and gradient clipping, plus the input sets the tests of that family share.

Restatement (`Ref`): per touched table row the contributions of one batch are summed — every element of the output
gradient clamped first, then times the per-sample weight, then divided by the bag length for MEAN; ids outside the table
are skipped — and the formulas of include/tbe_hip.h (tbe_backward_*_ex_*) are applied to the row once.  The `dtype`
switch runs the same code in float64 (the reference of the GPU tests) or float32 (tests/test_fused_optimizers.py: the
two must agree within the GPU tests' tolerance, i.e. that tolerance is not tighter than FP32 arithmetic allows on these
inputs).  EXACT_SGD and EXACT_ROWWISE_ADAGRAD (default weight_decay_mode, no decay) are restated too: the clipping
tests run them.

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

    def _apply(self, t, R, g):
        lr, eps, wd, b1, b2 = self.lr, self.eps, self.wd, self.b1, self.b2
        w = self.w[t][R]
        D = w.shape[1]

        def norm(x):
            return np.sqrt((x * x).sum(axis=1))

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
            wn, gn = norm(w), norm(g)
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
                v = b2 * self.state[1][t][R] + (1 - b2) * (g * g).sum(axis=1) / D
                self.state[1][t][R] = v
                if self.code == PARTIAL_ROWWISE_ADAM:
                    den = (np.sqrt(v / (1 - b2 ** self.t)) + eps)[:, None]
                else:
                    den = (np.sqrt(v) + eps)[:, None]
            if self.code == PARTIAL_ROWWISE_ADAM:
                self.w[t][R] = w - lr * ((m1 / (1 - b1 ** self.t)) / den + wd * w)
            else:
                u = m1 / den + wd * w
                self.w[t][R] = w - lr * ratio(norm(w), norm(u))[:, None] * u
        for a in [self.w[t]] + [s[t] for s in self.state if s is not None]:
            assert a.dtype == self.dtype  # a float32 run must not be promoted on the way


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
    u128   (30, 128) + (11, 128), SUM, B = 16, bags of 1-3: uniform and aligned — a FAST kernel's shape (clipping)"""
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
