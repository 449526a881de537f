"""The HBM row cache (csrc/tbe_cache.hip) through the C ABI against the exact host model of tests/_cache_abi.py:
scripted sequences (LRU, staging, set conflicts, duplicates, mixed features and windows, the empty call, random) over the
geometries that select every branch of the row copy (vector and scalar, both loops' second trip, a host base 4 B off the
16-B grid, per-table D under a wider row_stride), 70 cached tables, keys above 32 bits and row totals of 2^k - 1 and 2^k.

After every call the model checks every byte the call may touch — tags, lru, counters, staging keys, remapped ids, the cache
rows and their state, the host tables and the canaries round all of them — bit for bit, and a failure names the step, the
set, the way and the path (hit, claimed-empty, claimed-evict, staged).  tests/test_cache_model.py is the CPU guard of the
premise: each sequence reaches its path and wrong replacement policies are told apart."""
import ctypes

import numpy as np
import pytest

import _paths  # noqa: F401
import _cache_abi as ca

pytestmark = pytest.mark.gpu

GEOMS = sorted(ca.GEOMETRIES)


@pytest.mark.parametrize("name", GEOMS)
def test_lru_sequence(name):
    ca.seq_lru(ca.make_case(**ca.GEOMETRIES[name]))


@pytest.mark.parametrize("name", ["G1_D64_state", "G4_D13"])
def test_lru_sequence_at_the_iteration_limit(name):
    """The module stops at iteration 2^25 - 1: (lru + 1) * 64 + way still fits 32 bits there."""
    infos = ca.seq_lru(ca.make_case(**ca.GEOMETRIES[name]), it0=ca.ITERATION_LIMIT - 8)
    assert infos[-1].it == ca.ITERATION_LIMIT - 3


@pytest.mark.parametrize("name", GEOMS)
def test_staging_sequence(name):
    ca.seq_staging(ca.make_case(**ca.GEOMETRIES[name]))


@pytest.mark.parametrize("num_sets", [1, 2, 5])
@pytest.mark.parametrize("name", GEOMS)
def test_random_sequence(name, num_sets):
    ca.seq_random(ca.make_case(**dict(ca.GEOMETRIES[name], num_sets=num_sets)), seed=GEOMS.index(name))


@pytest.mark.parametrize("D", [8, 13])
def test_set_conflicts_do_not_spill(D):
    ca.seq_conflicts(ca.make_case(tab_rows=[600, 100], tab_D=D, num_sets=3, state=True))


def test_duplicates_and_shared_table():
    ca.seq_duplicates(ca.make_case(**ca.DUP_GEOMETRY))


def test_mixed_features_and_window():
    ca.seq_mixed(ca.make_case(**ca.MIXED_GEOMETRY))


def test_empty_call():
    ca.seq_empty(ca.make_case(**ca.GEOMETRIES["G1_D64_state"]))


def test_seventy_cached_tables():
    ca.seq_many_tables(ca.make_case(**ca.GEOMETRIES["G6_70_tables"]))


ERRORS = {
    "staging_cap<N": (dict(staging_cap=39), ca.TBE_ERR_INVALID_ARGUMENT, "staging_cap"),
    "workspace_one_byte_short": (dict(ws_short=1), ca.TBE_ERR_WORKSPACE, "workspace too small"),
    "workspace_not_256B_aligned": (dict(ws_shift=128), ca.TBE_ERR_INVALID_ARGUMENT, "256-B aligned"),
    "key_bits_0": (dict(key_bits=0), ca.TBE_ERR_INVALID_ARGUMENT, "key_bits=0"),
    "key_bits_63": (dict(key_bits=63), ca.TBE_ERR_INVALID_ARGUMENT, "key_bits=63"),
    "iteration_2^25": (dict(it=ca.ITERATION_LIMIT), ca.TBE_ERR_INVALID_ARGUMENT, "iteration"),
    "tags_8B_off": (dict(tags_shift=8), ca.TBE_ERR_INVALID_ARGUMENT, "tags must be 16-B aligned"),
}


@pytest.mark.parametrize("which", sorted(ERRORS))
def test_argument_errors_change_no_byte(which):
    kw, code, text = ERRORS[which]
    kw = dict(kw)
    case = ca.make_case(**ca.GEOMETRIES["G1_D64_state"])
    case.train_step(case.take(30), 1)  # warm: counters 4 and 5 are non-zero, a reset would show
    be, before = case.be, case.snap
    indices, offsets = case.batch_of_pairs(case.pairs(case.take(40)))
    rc = be.prefetch(indices, offsets, kw.pop("it", 2), None, **kw)
    assert rc == code and text in be.last_error(), (rc, be.last_error())
    after = be.snapshot()
    for name in ca.Snap.FIELDS:
        np.testing.assert_array_equal(getattr(after, name).view(np.uint8), getattr(before, name).view(np.uint8), err_msg=name)
    assert (be._rem.cpu().numpy() == ca.I_CANARY).all(), "remapped_indices was written"
    if which == "tags_8B_off":  # the descriptor check is shared by the other two entries
        d = be.desc(tags_shift=8)
        st = be._lib.stream_ptr(be.dev)
        assert be.lib.tbe_cache_flush(ctypes.byref(d), 1, st) == code and text in be.last_error()
        assert be.lib.tbe_cache_writeback_staging(ctypes.byref(d), st) == code and text in be.last_error()
        after = be.snapshot()
        for name in ca.Snap.FIELDS:
            np.testing.assert_array_equal(getattr(after, name).view(np.uint8), getattr(before, name).view(np.uint8), err_msg=name)
    case.train_step(np.concatenate([case.model.tags[:10], case.take(10)]), 2)  # the cache goes on as if nothing had been called
    case.finish()
