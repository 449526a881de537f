"""CPU guard of tests/test_cache_abi_gpu.py: the designed sequences, run through the host model of the row cache and a
numpy stand-in for the library (tests/_cache_abi.py), reach the paths they are for; three wrong replacement policies are
told apart from the model on the LRU sequence; the numpy set hash equals its restatement in Python integers.  Without
these the GPU file would prove less than it says."""
import numpy as np
import pytest

import _cache_abi as ca


def _sim(policy="lru", **geom):
    return ca.make_case(backend="sim", policy=policy, **geom)


def test_set_hash_matches_python_integers():
    rng = np.random.default_rng(0)
    keys = np.concatenate([np.arange(300), 2 ** np.arange(41, dtype=np.int64), 2 ** 33 + np.arange(200),
                           rng.integers(0, 2 ** 40, size=2000)]).astype(np.int64)
    for num_sets in (1, 2, 3, 5, 64, 1000003):
        got = ca.set_of(keys, num_sets)
        assert got.tolist() == [ca.set_of_int(k, num_sets) for k in keys.tolist()]
        assert got.min() >= 0 and got.max() < num_sets
    assert len(set(ca.set_of(keys, 5).tolist())) == 5


@pytest.mark.parametrize("it0", [1, ca.ITERATION_LIMIT - 8])
def test_lru_sequence_reaches_eviction_in_way_order_and_ties(it0):
    infos = ca.seq_lru(_sim(**ca.GEOMETRIES["G1_D64_state"]), it0)
    assert [i.M.size for i in infos] == [16, 16, 16, 16, 16, 20] and infos[4].H.size == 16
    assert [i.evicted.size for i in infos] == [0, 0, 0, 0, 16, 20]
    assert all(i.staged == 0 for i in infos)
    # the way order decides: the last claimed way's lru equals the first unclaimed candidate's (fill steps and the last)
    assert infos[0].tie and infos[5].tie and not infos[4].tie
    assert max(i.it for i in infos) < ca.ITERATION_LIMIT


def test_three_wrong_policies_claim_other_ways_on_the_lru_sequence():
    """Same state, same batch: the ways each wrong policy would claim differ from the model's at some step, so a kernel
    with that policy cannot pass the GPU test.  The stand-in run with each of them fails with a named way."""
    case = _sim(**ca.GEOMETRIES["G1_D64_state"])
    differ = {p: [] for p in ca.POLICIES if p != "lru"}
    real_prefetch = case.prefetch

    def spy(indices, offsets, it, feat_window=None):
        keys, _ = case.g.linearize(indices, offsets, feat_window)
        right = case.model.predict(keys, it).claimed_slots.tolist()
        for p in differ:
            differ[p].append(case.model.predict(keys, it, policy=p).claimed_slots.tolist() != right)
        return real_prefetch(indices, offsets, it, feat_window)

    case.prefetch = spy
    ca.seq_lru(case)
    assert differ["mru"][4] and differ["hits_unprotected"][4] and differ["lowest_way"][5], differ
    for policy in differ:
        with pytest.raises(AssertionError, match=r"prefetch\(iteration \d+\), step \d+: set 0 way \d+, path (hit|claimed-evict|untouched)"):
            ca.seq_lru(_sim(policy=policy, **ca.GEOMETRIES["G1_D64_state"]))


def test_staging_sequence_stages_with_every_way_hit():
    infos = ca.seq_staging(_sim(**ca.GEOMETRIES["G4_D13"]))
    assert [i.staged for i in infos] == [36, 10, 0, 5]
    assert infos[1].full_set_more_misses and infos[3].full_set_more_misses and not infos[0].full_set_more_misses
    assert infos[1].evicted.size == 0 and infos[2].evicted.size == 46


def test_conflict_sequence_overflows_one_set_beside_spare_ways():
    infos = ca.seq_conflicts(_sim(tab_rows=[600, 100], tab_D=8, num_sets=3))
    assert infos[0].staged == 6 and infos[0].sets[1]["cand"].size == 64 and infos[0].sets[1]["claimed"].size == 10
    assert infos[1].full_set_more_misses and infos[1].staged == 4


@pytest.mark.parametrize("num_sets", [1, 2, 5])
def test_random_sequence_evicts_stages_and_hits(num_sets):
    infos = ca.seq_random(_sim(**dict(ca.GEOMETRIES["G5_stride66"], num_sets=num_sets)), seed=0)
    assert sum(i.evicted.size for i in infos) > 0 and sum(i.H.size for i in infos) > 0
    if num_sets == 1:
        assert sum(i.staged for i in infos) > 0


@pytest.mark.parametrize("name", sorted(ca.GEOMETRIES))
def test_every_geometry_carries_the_three_sequences(name):
    geom = ca.GEOMETRIES[name]
    ca.seq_lru(_sim(**geom))
    ca.seq_staging(_sim(**geom))
    ca.seq_random(_sim(**dict(geom, num_sets=2)), seed=1)
    g = ca.Geometry(**geom)
    if name.startswith("G7"):
        assert g.key_bits == 34 and g.key_base[1] > 2 ** 33
    if name.startswith("rows_"):
        assert g.total in (1023, 1024) and _sim(**geom).pool[0] == g.total - 1
        assert g.key_bits == (10 if g.total == 1023 else 11)


def test_other_sequences_run_on_the_stand_in():
    ca.seq_duplicates(_sim(**ca.DUP_GEOMETRY))
    ca.seq_mixed(_sim(**ca.MIXED_GEOMETRY))
    ca.seq_empty(_sim(**ca.GEOMETRIES["G1_D64_state"]))
    ca.seq_many_tables(_sim(**ca.GEOMETRIES["G6_70_tables"]))


def test_verifier_names_the_path_of_a_wrong_copy():
    """Faults injected into the stand-in: a stale row on insertion, a state copied to the next slot, a write-back to the
    wrong host row, a flush that skips the last slot — each is reported with its path."""
    geom = ca.GEOMETRIES["G4_D67"]

    class ShortCopy(ca.SimBackend):  # the row copy stops at column 64
        def _copy(self, key, slot, to_host):
            keep = self.g.dev_rows(self.devf)[slot, 64:67].copy()
            super()._copy(key, slot, to_host)
            if not to_host:
                self.g.dev_rows(self.devf)[slot, 64:67] = keep

    g = ca.Geometry(**geom)
    with pytest.raises(AssertionError, match=r"set 0 way 0, path claimed-empty: rows column 64"):
        ca.seq_lru(ca.CacheCase(g, ShortCopy(g)))

    class WrongHostRow(ca.SimBackend):  # evictions land one row further
        def _copy(self, key, slot, to_host):
            super()._copy(key + 1 if to_host and slot < self.g.slots else key, slot, to_host)

    g = ca.Geometry(**ca.GEOMETRIES["G1_D64_state"])
    with pytest.raises(AssertionError, match=r"path (claimed-evict|untouched): host"):
        ca.seq_lru(ca.CacheCase(g, WrongHostRow(g)))

    class StateNextSlot(ca.SimBackend):
        def _copy(self, key, slot, to_host):
            super()._copy(key, slot, to_host)
            if not to_host:
                st = self.g.dev_state(self.devf)
                st[slot + 1], st[slot] = st[slot], ca.F_CANARY

    with pytest.raises(AssertionError, match=r"set 0 way \d+, path claimed-empty: state"):
        ca.seq_lru(ca.CacheCase(g, StateNextSlot(g)))

    class FlushSkipsLast(ca.SimBackend):
        def flush(self, invalidate):
            last, self.tags[-1] = self.tags[-1], -1
            super().flush(0)
            self.tags[-1] = last
            if invalidate:
                self.tags[:] = -1
                self.lru[:] = -1
            return 0

    with pytest.raises(AssertionError, match=r"flush\(0\), step \d+: set 0 way 63, path flush: host"):
        ca.seq_lru(ca.CacheCase(g, FlushSkipsLast(g)))

    class StagedNotWritten(ca.SimBackend):
        def writeback_staging(self):
            self.counters[0] -= 1
            super().writeback_staging()
            self.counters[0] += 1
            return 0

    with pytest.raises(AssertionError, match=r"writeback_staging, step 1: set 0 staging slot 35, path staged: host"):
        ca.seq_staging(ca.CacheCase(g, StagedNotWritten(g)))
