"""numpy restatement of SwishLayerNorm (torchrec/modules/activation.py:18-55) and of its gradients, in float64 or in float32
with the operation order csrc/swish_layernorm.hip documents (include/tbe_hip.h), laid out the way the kernels compute them
(four row reductions, two column sums) so that the faults a kernel of this kind can have are expressible (`fault=`):

  "mean_last_col", "var_last_col", "c1_last_col", "c2_last_col"   the last column left out of one of the row reductions
  "gamma_last_row", "beta_last_row"                               the last row of the first row block left out of a column sum

Also: the fixtures' accessors, the inputs of the GPU tests (`gpu_case`), and the tolerance of the GPU tests, which is MEASURED
here (`gpu_tolerance`): 8 x the worst float32-vs-float64 error of the reference's own fixtures and of this restatement on the
GPU tests' shapes.  No case here has N = 1 (its normalised value is exactly 0 and a relative error means nothing)."""
import functools
import os

import numpy as np

from _crossnet_ref import rel_err  # max |a - ref| / max |ref|

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swish_layernorm.npz")
CASES = {"3x100": ((3,), [100]), "37x20": ((37,), [20]), "70x64": ((70,), [64]), "5x3x4x8": ((5, 3), [4, 8]),
         "9x10": ((9,), [10])}  # (leading dims, input_dims), as tests/golden/make_swish_layernorm_golden.py records them
MLP_ARGS = (40, [16, 8, 4])
EPS = 1e-5  # nn.LayerNorm's default
FAULTS = ("mean_last_col", "var_last_col", "c1_last_col", "c2_last_col", "gamma_last_row", "beta_last_row")
MAX_N = 4096


# ---- geometry of csrc/swish_layernorm.hip ----------------------------------------------------------------------------------
def threads_per_row(N):
    return 16 if N <= 64 else 64 if N <= 1024 else 256


def rows_per_block(N):
    return {16: 128, 64: 32, 256: 16}[threads_per_row(N)]


# Every threads-per-row class with both sides of its boundaries (64 | 68, 1024 | 1028), every float4 slot count a thread can
# hold (a wave per row: 1 ... 4 from 256, 512, 768, 1024; the block per row: 2 ... 4 from 2048, 3072, 4096), each count's
# first width (260, 516, 772; 1028, 2052, 3076: the last slot holds one float4), a slot row that is partly empty (60), and
# the limits 4 and 4096.
ABI_WIDTHS = (4, 60, 64, 68, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048, 2052, 3072, 3076, 4096)


def abi_shapes():
    """(B, N): at each width one row, and three row blocks of which the last is ragged."""
    out = []
    for N in ABI_WIDTHS:
        rpb = rows_per_block(N)
        out += [(1, N), (2 * rpb + max(3, rpb // 3), N)]
    return out


MODULE_SHAPES = [(70, 64), (15, 32), (3, 100)]  # the kernel-path fixtures' (B, N)
TRAIN_WIDTHS = (128, 64)  # MLP(64, [128, 64]) at B = 96
TRAIN_BATCH = 96


# ---- the op --------------------------------------------------------------------------------------------------------------
def _rowsum(a, fault, name):
    if fault == name:
        a = a[:, :-1]
    return a.sum(axis=1, dtype=a.dtype)


def _colsum(a, N, fault, name):
    if fault == name:
        keep = np.ones(a.shape[0], dtype=bool)
        keep[min(rows_per_block(N), a.shape[0]) - 1] = False
        a = a[keep]
    return a.sum(axis=0, dtype=a.dtype)


def run(gamma, beta, x, g, eps=EPS, dtype="float64", fault=None):
    """Forward and backward over x [B, N].  Returns {"out", "mean", "rstd", "grad_input", "grad_gamma", "grad_beta"}; every
    product and add of the float32 form is rounded on its own, in the kernels' order."""
    dt = np.dtype(dtype).type
    gamma, beta, y, g = (np.asarray(a, dtype=dt) for a in (gamma, beta, x, g))
    B, N = y.shape
    gamma, beta = gamma.reshape(N), beta.reshape(N)
    fn, one = dt(N), dt(1)
    with np.errstate(over="ignore"):
        mean = _rowsum(y, fault, "mean_last_col") / fn
        d = y - mean[:, None]
        var = _rowsum(d * d, fault, "var_last_col") / fn
        rstd = one / np.sqrt(var + dt(eps))
        n = d * rstd[:, None]
        z = n * gamma + beta
        s = one / (one + np.exp(-z))
        out = y * s
        dz = ((g * y) * s) * (one - s)
        dn = dz * gamma
        c1 = _rowsum(dn, fault, "c1_last_col") / fn
        c2 = _rowsum(dn * n, fault, "c2_last_col") / fn
        gy = g * s + rstd[:, None] * ((dn - c1[:, None]) - n * c2[:, None])
    return {"out": out, "mean": mean, "rstd": rstd, "grad_input": gy,
            "grad_gamma": _colsum(dz * n, N, fault, "gamma_last_row"), "grad_beta": _colsum(dz, N, fault, "beta_last_row")}


def result_errors(got, ref):
    """{name: rel_err} over every tensor both hold."""
    return {k: rel_err(got[k], ref[k]) for k in ref if k in got}


def gpu_case(B, N, seed=0):
    """(gamma, beta, x, g) float32 of a GPU test, distributed like the fixtures: gamma about 1, beta about 0 (both +- 0.5),
    x of mean 0.5 and standard deviation 2, standard normal g.  The last column — the one a faulty tail would miss — is
    given a deviation of 2.5, a gradient of 1.5 (random signs), gamma 1 and beta 0, so that its share of every row
    reduction is about 1 / N of the sum whatever the seed: with one row of 4096 columns a random last element can be small
    enough to hide (tests/test_swish_layernorm.py checks that it cannot)."""
    rng = np.random.default_rng([seed, B, N])
    gamma = (1.0 + 0.5 * rng.standard_normal(N)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(N)).astype(np.float32)
    x = (0.5 + 2.0 * rng.standard_normal((B, N))).astype(np.float32)
    g = rng.standard_normal((B, N)).astype(np.float32)
    gamma[-1], beta[-1] = 1.0, 0.0
    x[:, -1] = 0.5 + 2.5 * rng.choice([-1.0, 1.0], B)
    g[:, -1] = 1.5 * rng.choice([-1.0, 1.0], B)
    return gamma, beta, x, g


# ---- fixtures ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _record(pre, names):
    z = _golden()
    fx = {"params": {n: z[pre + "param|" + n] for n in names}, "x": z[pre + "x"], "g": z[pre + "g"]}
    for prec in ("f32", "f64"):
        fx[prec] = {"out": z[pre + prec + "|out"], "grad_input": z[pre + prec + "|grad_input"],
                    "grad": {n: z[pre + prec + "|grad|" + n] for n in names}}
    return fx


SLN_KEYS = ["norm.0.weight", "norm.0.bias"]


def fixture(case):
    """The reference module's recorded run: {"params", "x", "g", "f32": {"out", "grad_input", "grad": {...}}, "f64": ...}."""
    return _record(f"sln|{case}|", SLN_KEYS)


def mlp_keys():
    keys = []
    for i in range(len(MLP_ARGS[1])):
        keys += [f"_mlp.{i}._linear.weight", f"_mlp.{i}._linear.bias", f"_mlp.{i}._activation_fn.norm.0.weight",
                 f"_mlp.{i}._activation_fn.norm.0.bias"]
    return keys


def mlp_fixture():
    """The recorded run of the reference's MLP(40, [16, 8, 4], activation="swish_layernorm") on a batch of 3."""
    return _record("mlp|", mlp_keys())


def flat(case, rec):
    """A fixture's record as `run` lays its results out: [B, N] tensors and [N] parameter gradients."""
    N = int(np.prod(CASES[case][1]))
    return {"out": rec["out"].reshape(-1, N), "grad_input": rec["grad_input"].reshape(-1, N),
            "grad_gamma": rec["grad"]["norm.0.weight"].reshape(N), "grad_beta": rec["grad"]["norm.0.bias"].reshape(N)}


def run_fixture(case, dtype="float64", fault=None):
    fx = fixture(case)
    N = int(np.prod(CASES[case][1]))
    return run(fx["params"]["norm.0.weight"], fx["params"]["norm.0.bias"], fx["x"].reshape(-1, N), fx["g"].reshape(-1, N),
               EPS, dtype, fault)


# ---- the tolerance ---------------------------------------------------------------------------------------------------------
def gpu_test_shapes():
    return abi_shapes() + MODULE_SHAPES + [(TRAIN_BATCH, N) for N in TRAIN_WIDTHS]


@functools.lru_cache(maxsize=None)
def measured_errors():
    """The float32-vs-float64 error of (a) the reference's fixtures and (b) this restatement on the GPU tests' shapes:
    {label: worst rel_err over the run's tensors}."""
    errs = {}
    for case in CASES:
        fx = fixture(case)
        errs[f"reference {case}"] = max(result_errors(flat(case, fx["f32"]), flat(case, fx["f64"])).values())
    for B, N in gpu_test_shapes():
        c = gpu_case(B, N)
        errs[f"restatement {B}x{N}"] = max(result_errors(run(*c, dtype="float32"), run(*c, dtype="float64")).values())
    return errs


def gpu_tolerance():
    """8 x the worst measured float32-vs-float64 error: the factor covers another summation order and the device's expf
    (as in tests/_crossnet_ref.py).  Compared with `rel_err`."""
    return 8.0 * max(measured_errors().values())
