"""The TBE forward kernels (csrc/tbe_forward_impl.hpp) through the C ABI, on every dispatch path, against the oracle and BIT
FOR BIT: every (G, NV) class on the short and the long kernel, 16 and 64 bags per wave, each reason for the scalar column
path on its own, row windows, bad ids and malformed offsets, and the PoolingMode.NONE entries past their grid cap.

The inputs (tests/_fwd_abi.py) make every pooled sum exact in FP32 in any order — guarded on the CPU by
tests/test_forward_inputs.py, which also shows that `verify` rejects a forward with one injected fault — so no comparison
here has a tolerance.  `out` is prefilled with a NaN canary and has gap columns and guard bytes, the error counts are exact,
and an FP16 table must give what the FP32 entry gives on the up-cast table."""
import numpy as np
import pytest

import _fwd_abi as fa

pytestmark = pytest.mark.gpu


def _check(spec, dtypes=None):
    """Runs `spec` with every table type it is for; all must give the oracle's bits (hence each other's)."""
    exp = fa.spec_expected(spec)
    results = {}
    for dtype in dtypes or spec.dtypes:
        res, disp = fa.run_spec(spec, dtype)
        fa.verify(res, exp, disp, spec.dims, f"{spec.name} [{dtype}]")
        results[dtype] = res
    if len(results) == 2:  # said directly, too: FP16 tables == the FP32 entry on the up-cast tables
        np.testing.assert_array_equal(fa.bits(results["float16"].written), fa.bits(results["float32"].written))
        assert results["float16"].errors == results["float32"].errors
    return results


@pytest.mark.parametrize("spec", fa.class_cases(), ids=lambda s: s.name)
def test_every_class_at_16_bags_per_wave(spec):
    assert spec.dispatch().bags_per_wave == 16 and spec.dispatch().kernel == spec.lengths
    _check(spec)


@pytest.mark.parametrize("spec", fa.bpw64_cases(), ids=lambda s: s.name)
def test_64_bags_per_wave(spec):
    d = spec.dispatch()
    assert d.bags_per_wave == 64 and d.kernel == "short"
    _check(spec)


@pytest.mark.parametrize("spec", fa.vec_cases(), ids=lambda s: s.name)
def test_each_vec_disqualifier_on_its_own(spec):
    for dtype in spec.dtypes:
        assert list(spec.dispatch(dtype).vec) == fa.vec_expectation(spec, dtype)
    _check(spec)


@pytest.mark.parametrize("spec", fa.id_cases(), ids=lambda s: s.name)
def test_windows_bad_ids_and_malformed_offsets(spec):
    res = _check(spec)
    assert all(r.errors > 0 for r in res.values())


def _check_nobag(spec):
    exp = fa.expected_nobag(fa.nobag_tables(spec), fa.nobag_batch(spec))
    assert (exp.errors > 0) == spec.bad
    results = {}
    for dtype in spec.dtypes:
        res, disp = fa.run_nobag(spec, dtype)
        fa.verify(res, exp, disp, [spec.D], f"{spec.name} [{dtype}]")
        results[dtype] = res
    if len(results) == 2:
        np.testing.assert_array_equal(fa.bits(results["float16"].written), fa.bits(results["float32"].written))


@pytest.mark.parametrize("spec", fa.nobag_edge_cases(), ids=lambda s: s.name)
def test_nobag_class_edges_and_block_edges(spec):
    assert spec.dispatch().trips == 1
    _check_nobag(spec)


@pytest.mark.parametrize("spec", fa.nobag_other_cases(), ids=lambda s: s.name)
def test_nobag_grid_stride_empty_features_bad_ids_alignment(spec):
    if spec.name.startswith("past_cap"):
        assert spec.dispatch().trips == 2
    _check_nobag(spec)


@pytest.mark.parametrize("name", ["D128-short-wmean-B64", "D64-long-wmean-B65", "F26xB20165-skewed-wmean-maxD128"])
def test_pooled_is_deterministic(name):
    spec = next(s for s in fa.class_cases() + fa.bpw64_cases() if s.name == name)
    for dtype in spec.dtypes:
        a, _ = fa.run_spec(spec, dtype)
        b, _ = fa.run_spec(spec, dtype)
        np.testing.assert_array_equal(fa.bits(a.out), fa.bits(b.out))
        assert a.errors == b.errors and a.guards_ok and b.guards_ok


def test_nobag_is_deterministic():
    spec = next(s for s in fa.nobag_other_cases() if s.name.startswith("past_cap-G16"))
    for dtype in spec.dtypes:
        a, _ = fa.run_nobag(spec, dtype)
        b, _ = fa.run_nobag(spec, dtype)
        np.testing.assert_array_equal(fa.bits(a.out), fa.bits(b.out))
        assert a.errors == b.errors == 0 and a.guards_ok and b.guards_ok
