"""CPU guard of the premise tests/test_tbe_forward_abi_gpu.py rests on (tests/_fwd_abi.py): for every designed input the
pooled sums are exact in FP32 whatever the order, so the FP32 oracle equals a float64 sum rounded once and the FP32 sum taken
backwards, bit for bit, and a GPU kernel may be compared with it bitwise; every case list reaches the dispatch paths it is
for; and the comparison the GPU tests use rejects a numpy forward with one injected fault, naming the path.  Widening a
value range or thinning a case list breaks THIS test, not the GPU comparison."""
import numpy as np
import pytest

import _fwd_abi as fa
from oracle import oracle


def _unique_batches(specs):
    seen, out = set(), []
    for s in specs:
        key = (s.batch_key(), s.pooling, None if s.feat_pooling is None else tuple(s.feat_pooling))
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


POOLED = fa.class_cases() + _unique_batches(fa.bpw64_cases()) + _unique_batches(fa.vec_cases()) + fa.id_cases()


@pytest.mark.parametrize("spec", POOLED, ids=lambda s: s.name)
def test_oracle_equals_the_float64_sum_and_the_reversed_sum_exactly(spec):
    tables, batch = fa.build_tables(spec), fa.build_batch(spec)
    for t in tables:
        assert np.array_equal(t * 8, np.round(t * 8)) and np.abs(t).max() <= 4 and np.abs(t).max() > 0
        assert np.array_equal(t.astype(np.float16).astype(np.float32), t)
    if batch.psw is not None:
        assert set(np.unique(batch.psw).tolist()) <= {0.5, 1.0, 2.0}
    san = fa.sanitize(tables, batch, spec.feat_window)
    assert san.lens.max() <= fa.MAX_BAG and san.lens.size == spec.F * spec.B
    exp = fa.spec_expected(spec)
    assert exp.out.dtype == np.float32 and exp.out.shape == (spec.B, spec.sum_D)
    mean = fa.mean_flags(spec.F, spec.pooling, spec.feat_pooling)
    f64 = fa.pooled_f64(tables, san.idx, san.offs, san.psw, spec.F, spec.B, mean)
    assert np.array_equal(fa.bits(exp.out), fa.bits(f64))
    ridx, rpsw = fa.reversed_bags(san)
    back = fa.oracle_pooled(tables, ridx, san.offs, rpsw, spec.pooling, spec.feat_pooling)
    assert np.array_equal(fa.bits(exp.out), fa.bits(back))
    # every term is a multiple of 1/16 and |sum| * 16 stays far below 2^24: every partial sum of every order is representable
    sums = fa.pooled_f64(tables, san.idx, san.offs, san.psw, spec.F, spec.B, [False] * spec.F).astype(np.float64)
    assert np.array_equal(sums * 16, np.round(sums * 16)) and np.abs(sums).max() * 16 <= 38400 and np.abs(sums).max() > 0
    assert exp.errors == san.n_bad + san.n_malformed
    if spec.ids == "plain":
        assert exp.errors == 0 and san.n_foreign == 0
    # an empty bag reads +0.0
    empty = np.nonzero(san.lens.reshape(spec.F, spec.B)[0] == 0)[0]
    assert (fa.bits(exp.out[empty, :spec.dims[0]]) == 0).all()


def test_class_cases_reach_every_class_on_both_kernels_vec_and_scalar():
    specs = fa.class_cases()
    keys, b_at, modes = set(), {16: set(), 64: set()}, set()
    long_not_multiple_of_4 = 0
    for s in specs:
        d = s.dispatch()
        assert d.bags_per_wave == 16 and d.kernel == s.lengths, s.name
        assert (d.G, d.NV) == fa.class_of(s.max_D) and max(s.dims) == s.max_D
        assert list(d.vec) == [True] * (s.F - 1) + [False] and s.dims[-1] % 2 == 1 and 8 in s.dims
        assert 0 < s.stride - s.sum_D < 12 and s.stride % 4 == 0
        keys |= {d.key(f) for f in range(s.F)}
        modes.add((d.kernel, d.G, d.NV, s.weighted, s.pooling, s.feat_pooling is not None))
        if d.G in b_at:
            b_at[d.G].add(s.B)
        long_not_multiple_of_4 += d.kernel == "long" and (s.F * s.B) % 4 != 0
        lens = np.diff(fa.build_batch(s).offsets).reshape(s.F, s.B)
        if d.kernel == "long":
            assert set(np.unique(lens).tolist()) <= set(fa.LONG_LENGTHS)
            if s.B >= len(fa.LONG_LENGTHS):
                assert all(set(lens[f].tolist()) == set(fa.LONG_LENGTHS) for f in range(s.F)), s.name
            else:
                assert {64, 65, 200, 0} <= set(lens.reshape(-1).tolist())
        else:
            assert set(np.unique(lens).tolist()) <= {0, 1, 2, 3}
    want = {(k, G, NV, 16, v) for k in ("short", "long") for _, G, NV in fa.CLASSES for v in (True, False)}
    assert keys == want
    assert len(modes) == 2 * 6 * 4  # unweighted SUM, weighted SUM, weighted MEAN, mixed MEAN per kernel and class
    assert b_at[16] == set(fa.BATCHES) and b_at[64] == set(fa.BATCHES)
    assert long_not_multiple_of_4 >= 1
    lower_plus_4 = {s.dims[1] for s in specs}
    assert lower_plus_4 == {4, 68, 132, 260, 516, 1028} and {s.dims[-1] for s in specs} == set(fa.ODD_D)


def test_bpw64_cases_really_have_64_bags_per_wave():
    specs = fa.bpw64_cases()
    assert len(specs) == 3 * 2 * 2 * 4
    seen = set()
    for s in specs:
        d = s.dispatch()
        assert d.bags_per_wave == 64 and d.kernel == "short" and s.F * s.B >= 1 << 19, s.name
        seen.add(((s.F, s.B), s.lengths, (s.weighted, s.pooling), s.max_D))
    assert len(seen) == len(specs)
    assert [(64 // fa.class_of(m)[0]) * fa.U for m in sorted({x[3] for x in seen})] == [16, 8, 4, 4] and {x[0] for x in seen} == set(fa.SHAPES_64)
    assert (262144 + 65) % 256 == 65 and 20165 % 256 == 197  # the second wave of the last tile holds one bag; a partly filled tile


@pytest.mark.parametrize("G", [16, 32, 64])
@pytest.mark.parametrize("bpw,B", [(16, 300), (64, 20165), (64, 262144 + 65)])
def test_skewed_layout_puts_a_200_and_an_empty_bag_in_flight_together(G, bpw, B):
    lens = fa.skewed_lengths(1, B)[0]
    assert {64, 65, 200} <= set(lens.tolist()) and (lens == 0).mean() >= 0.9 and lens.mean() < fa.LONG_AVG
    mates = fa.quad_mates(B, bpw, G)
    in_flight = np.where(mates >= 0, lens[np.maximum(mates, 0)], -1)  # [4, B]
    both = (in_flight == 200).any(axis=0) & (in_flight == 0).any(axis=0)
    assert both.any()
    assert ((mates == np.arange(B)[None, :]).sum(axis=0) == 1).all()  # a bag is one of its own four


def test_vec_cases_hold_exactly_one_disqualifier():
    names = set()
    for s in fa.vec_cases():
        for dtype in s.dtypes:
            d = s.dispatch(dtype)
            assert (d.G, d.NV, d.bags_per_wave) == (32, 1, 16) and d.kernel == s.lengths
            assert list(d.vec) == fa.vec_expectation(s, dtype), (s.name, dtype)
            reasons = [any(D % 4 for D in s.dims), s.stride % 4 != 0, bool(s.misalign), s.out_off != 0]
            assert sum(reasons) == (0 if s.name.startswith("aligned") else 1), s.name
            assert all(D in (128, 64) for D, v in zip(s.dims, d.vec) if D % 4 == 0) and s.stride > s.sum_D
            names.add((s.name.rsplit("-", 1)[0], dtype, d.kernel))
    for kernel in ("short", "long"):
        for dtype in ("float32", "float16"):
            assert {("aligned", dtype, kernel), ("odd_front", dtype, kernel), ("stride", dtype, kernel), ("out_off", dtype, kernel)} <= names
        assert ("table_off_4B", "float32", kernel) in names
        assert {(f"table_off_{n}", "float16", kernel) for n in ("2B", "4B_f16", "6B")} <= names


def test_id_cases_hold_every_kind_of_id_and_offset():
    seen = set()
    for s in fa.id_cases():
        d, batch = s.dispatch(), fa.build_batch(s)
        san = fa.sanitize(fa.build_tables(s), batch, s.feat_window)
        seen.add((s.ids, d.kernel, d.bags_per_wave))
        if s.ids == "window":
            assert san.n_bad > 0 and san.n_foreign > 0 and (batch.indices == fa.ID_SKIP).any() and san.n_malformed == 0
            assert (san.idx >= 0).sum() > 0.4 * san.idx.size
        elif s.ids == "bad":
            assert san.n_bad > 0 and san.n_foreign == 0 and san.n_malformed == 0
        else:
            st, en = batch.offsets[:-1], batch.offsets[1:]
            assert (st < 0).any() and (en > batch.N).any() and ((st > en) & (st >= 0) & (en <= batch.N)).any()
            assert san.n_malformed >= 16 and san.n_bad == 0
            good = ~((st < 0) | (en > batch.N) | (st > en))
            order = np.argsort(st[good], kind="stable")
            assert (st[good][order][1:] >= en[good][order][:-1]).all()  # no two good bags overlap
    assert seen == {(i, k, b) for i in ("window", "bad", "malformed") for k, b in (("short", 16), ("long", 16), ("short", 64))}


def test_nobag_cases_reach_every_class_a_second_trip_and_empty_features():
    edge, other = fa.nobag_edge_cases(), fa.nobag_other_cases()
    per_class = {}
    for s in edge:
        d = s.dispatch()
        per_class.setdefault((d.G, d.NV), set()).add((s.D, s.N - d.per_block))
        assert d.trips == 1 and d.per_block == 16 * (64 // d.G)
    assert set(per_class) == {(G, NV) for _, G, NV in fa.CLASSES}
    for ci, (top, G, NV) in enumerate(fa.CLASSES):
        pb = 16 * (64 // G)
        assert per_class[(G, NV)] == {(D, n) for D in (fa.CLASS_LOWER[ci] + 1, top, fa.NOBAG_ODD_D[ci]) for n in (1 - pb, -1, 0, 1)}
    by_name = {s.name: s for s in other}
    for G, (D, N) in fa.NOBAG_PAST_CAP.items():
        d = by_name[f"past_cap-G{G}-D{D}-N{N}"].dispatch()
        assert d.G == G and d.grid == fa.NOBAG_GRID_CAP and d.trips == 2 and N > d.grid * d.per_block and all(d.vec)
    e = by_name["empty_first_middle_last"].counts
    assert e[0] == e[1] == 0 and e[3] == e[4] == 0 and e[-1] == 0 and sum(c > 0 for c in e) == 3
    assert by_name["F1"].F == 1 and by_name["F70"].F == 70 and by_name["F70"].counts.count(0) >= 20
    for name in ("F70-bad", "bad-D64", "bad-D2047"):
        assert fa.expected_nobag(fa.nobag_tables(by_name[name]), fa.nobag_batch(by_name[name])).errors > 0
    assert by_name["table_off_4B"].dispatch("float32").vec == (True, False, True)
    for off in (2, 4, 6):
        assert by_name[f"table_off_{off}B_f16"].dispatch("float16").vec == (True, False, True)
    assert by_name["out_off"].dispatch().vec == (False, False, False)
    for s in edge + other:
        batch = fa.nobag_batch(s)
        assert batch.N == s.N and np.array_equal(batch.offsets[::s.B], np.concatenate([[0], np.cumsum(s.counts)]))
        exp = fa.expected_nobag(fa.nobag_tables(s), batch)
        assert exp.out.shape == (s.N, s.D) and (exp.errors > 0) == s.bad


# ---- the comparison rejects a wrong forward ----------------------------------------------------------------------------
def _spec(lists, name):
    return next(s for s in lists if s.name == name)


def _standin(spec, fault=None):
    res, disp = fa.standin_forward(fa.build_tables(spec), fa.build_batch(spec), spec.max_D, spec.pooling, spec.feat_pooling,
                                   spec.feat_window, spec.stride, fault)
    fa.verify(res, fa.spec_expected(spec), disp, spec.dims, spec.name)


LONG_64 = "D64-long-wmean-B65"  # G = 16: four groups per wave
SKEWED_16 = fa.Spec("skewed-B300", [8, 132], 300, "skewed", 132, True, oracle.POOL_MEAN, pad=4)
FAULT_CASES = [
    ("drop_pos64", fa.class_cases, LONG_64, r"long kernel, G=16 NV=1, 16 bags per wave, feature 0 \(vec\): \d+ elements differ"),
    ("drop_group1", fa.class_cases, LONG_64, r"long kernel, G=16 NV=1, 16 bags per wave, feature 0 \(vec\): \d+ elements differ"),
    ("zero_bags_16_63", fa.bpw64_cases, "F2xB262209-short-wmean-maxD64",
     r"short kernel, G=16 NV=1, 64 bags per wave, feature \d \(vec\): .* first at bag (1[6-9]|[2-5]\d|6[0-3]) "),
    ("skip_last_slot", fa.class_cases, "D2048-short-sum-B130",
     r"short kernel, G=64 NV=8, 16 bags per wave, feature 0 \(vec\): .* column 1792 \(slot v = 7\): got nan"),
    ("drop_4th_scalar", fa.class_cases, "D64-short-sum-B1", r"short kernel, G=16 NV=1, 16 bags per wave, feature 3 \(scalar\): .* column 3 "),
    ("mean_maxlen", None, SKEWED_16, r"short kernel, G=64 NV=1, 16 bags per wave, feature \d \(\w+\): \d+ elements differ"),
    ("mean_maxlen", fa.bpw64_cases, "F26xB20165-skewed-wmean-maxD128", r"short kernel, G=32 NV=1, 64 bags per wave, feature"),
    ("foreign_bad", fa.id_cases, "window-short16", r"short kernel, G=64 NV=1, 16 bags per wave: bounds_errors \d+, want exactly \d+"),
    ("foreign_bad", fa.id_cases, "window-long16", r"long kernel, G=64 NV=1, 16 bags per wave: bounds_errors \d+, want exactly \d+"),
    ("gap_overwrite", fa.class_cases, "D256-long-wsum-B17", r"long kernel, G=64 NV=1, 16 bags per wave: gap column \d+ of row 8 was written"),
]


@pytest.mark.parametrize("fault,cases,name,message", FAULT_CASES, ids=[f"{c[0]}-{getattr(c[2], 'name', c[2])}" for c in FAULT_CASES])
def test_verify_rejects_an_injected_fault_and_names_the_path(fault, cases, name, message):
    spec = name if cases is None else _spec(cases(), name)
    _standin(spec)  # the stand-in itself passes
    with pytest.raises(AssertionError, match=message):
        _standin(spec, fault)


def test_verify_rejects_a_canary_left_in_an_empty_bag_and_a_touched_guard():
    spec = _spec(fa.class_cases(), "D128-short-wmean-B64")
    tables, batch = fa.build_tables(spec), fa.build_batch(spec)
    res, disp = fa.standin_forward(tables, batch, spec.max_D, spec.pooling, stride=spec.stride)
    empty = int(np.nonzero(np.diff(batch.offsets)[:spec.B] == 0)[0][0])
    res.out[empty, 0] = fa.canary_block(1, 1)[0, 0]
    with pytest.raises(AssertionError, match=rf"feature 0 \(vec\): 1 elements differ in 1 rows; first at bag {empty} column 0 .*got nan, want 0\.0"):
        fa.verify(res, fa.spec_expected(spec), disp, spec.dims)
    res.out[empty, 0] = -0.0  # bit for bit: a negative zero is not the oracle's +0.0
    with pytest.raises(AssertionError, match="got -0.0, want 0.0"):
        fa.verify(res, fa.spec_expected(spec), disp, spec.dims)
    res, disp = fa.standin_forward(tables, batch, spec.max_D, spec.pooling, stride=spec.stride)
    for kw, message in ((dict(outer_ok=False), "guard bytes"), (dict(tables_ok=False), "a table changed")):
        bad = fa.Result(res.out, res.errors, sum_D=spec.sum_D, **kw)
        assert not bad.guards_ok
        with pytest.raises(AssertionError, match=message):
            fa.verify(bad, fa.spec_expected(spec), disp, spec.dims)
