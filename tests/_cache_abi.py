"""The HBM row cache (csrc/tbe_cache.hip) driven straight through the C ABI (include/tbe_hip.h) against an exact host model.

Everything the cache does is a copy or an integer decision, so every comparison here is bit for bit.

* `Geometry`, `Model`, `CacheCase`, `SimBackend` and the `seq_*` sequences use numpy only: the CPU guard
  (tests/test_cache_model.py) runs the designed sequences through them and shows that each reaches the path it is for.
  The model predicts, from the last verified device state, everything a `tbe_cache_prefetch` must do except which missed
  key lands in which claimed way (the compare-and-swap race decides that; it cannot change WHICH ways are claimed: a way
  only ever leaves the candidates, so the smallest (lru, way) a wave sees is the true smallest whenever its CAS succeeds).
  The observed key -> way assignment is verified to be a legal one and adopted.
* `GpuBackend` lays every buffer between canary values and calls the library.  `SimBackend` is a numpy restatement of the
  kernels' contract with a choice of (wrong) replacement policies: it exists to test the verifier, not the library.

Values are integers in float32 (initial rows, the per-step deltas of `update`), so sums are exact.
"""
import numpy as np

WAYS = 64
TBE_ID_SKIP = -(2 ** 63)
HASH_MUL = 0x9E3779B97F4A7C15
GUARD = 64  # canary elements before and after every array
F_CANARY = np.float32(-12345.5)
I_CANARY = 0x5A5A5A5A5A5A5A5A
LOCAL, FOREIGN, BAD, UNCACHED = 0, 1, 2, 3
TBE_ERR_INVALID_ARGUMENT, TBE_ERR_WORKSPACE = -1, -3
ITERATION_LIMIT = 1 << 25


def set_of(keys, num_sets):
    """(((key * 0x9E3779B97F4A7C15) mod 2^64) >> 32) % num_sets in uint64 arithmetic (arrays wrap silently)."""
    k = np.atleast_1d(np.asarray(keys, dtype=np.int64)).astype(np.uint64)
    h = (k * np.uint64(HASH_MUL)) >> np.uint64(32)
    return (h % np.uint64(num_sets)).astype(np.int64)


def set_of_int(key, num_sets):
    """The same in Python integers."""
    return (((int(key) * HASH_MUL) % (1 << 64)) >> 32) % int(num_sets)


# ---- replacement policies: (lru of the set before this call, lru after the hits are marked, it) -> victim ways in order
def _order_lru(old, marked, it):
    w = np.nonzero(marked < it)[0]
    return w[np.lexsort((w, marked[w]))]


def _order_mru(old, marked, it):
    w = np.nonzero(marked < it)[0]
    return w[np.lexsort((w, -marked[w].astype(np.int64)))]


def _order_way(old, marked, it):
    return np.nonzero(marked < it)[0]


def _order_hits_unprotected(old, marked, it):
    w = np.arange(WAYS)
    return w[np.lexsort((w, old))]


POLICIES = {"lru": _order_lru, "mru": _order_mru, "lowest_way": _order_way, "hits_unprotected": _order_hits_unprotected}


class Geometry:
    """Cached tables, features and the element layout of every buffer.

    tab_rows are the DECLARED rows (they make the keys); tab_alloc the rows that exist in host memory (ids must stay
    below them).  host_off[t] floats are added to table t's 16-B aligned start.  feat_ctab[f] is a cached table or -1;
    feat_window[f] = (first global row, global rows) as in tbe_hip.h, None = no feature has a window."""

    def __init__(self, tab_rows, tab_D, row_stride=None, num_sets=1, state=False, host_off=None, tab_alloc=None,
                 staging_cap=512, feat_ctab=None, feat_rows=None, feat_window=None, must_include_last=False):
        self.tab_rows = [int(r) for r in tab_rows]
        self.Tc = len(self.tab_rows)
        self.tab_D = [int(d) for d in (tab_D if isinstance(tab_D, (list, tuple)) else [tab_D] * self.Tc)]
        self.row_stride = int(row_stride) if row_stride is not None else max(self.tab_D)
        assert max(self.tab_D) <= self.row_stride
        self.num_sets, self.state, self.staging_cap = int(num_sets), bool(state), int(staging_cap)
        self.host_off = list(host_off) if host_off is not None else [0] * self.Tc
        self.tab_alloc = [int(a) for a in tab_alloc] if tab_alloc is not None else list(self.tab_rows)
        base = [0]
        for r in self.tab_rows:
            base.append(base[-1] + r)
        self.key_base = np.array(base, dtype=np.int64)
        self.total = base[-1]
        self.key_bits = max(1, int(self.total).bit_length())  # the all-ones sentinel is >= total > every key
        self.feat_ctab = list(feat_ctab) if feat_ctab is not None else list(range(self.Tc))
        self.F = len(self.feat_ctab)
        self.feat_rows = (list(feat_rows) if feat_rows is not None
                          else [self.tab_rows[c] if c >= 0 else 0 for c in self.feat_ctab])
        self.feat_window = None if feat_window is None else [tuple(int(x) for x in w) for w in feat_window]
        self.must_include_last = must_include_last
        self.slots = self.num_sets * WAYS
        self.n_slots = self.slots + self.staging_cap
        # device floats: guard | rows | guard | state | guard
        self.rows_off = GUARD
        self.rows_len = self.n_slots * self.row_stride
        self.state_off = (self.rows_off + self.rows_len + GUARD + 3) // 4 * 4
        self.devf_len = self.state_off + self.n_slots + GUARD
        # host floats: guard | table 0 | guard | table 1 | ...
        off, self.tab_off = GUARD, []
        for t in range(self.Tc):
            off = (off + 3) // 4 * 4 + self.host_off[t]
            self.tab_off.append(off)
            off += self.tab_alloc[t] * self.tab_D[t] + GUARD
        self.host_len = off
        off, self.hs_off = GUARD, []
        for t in range(self.Tc):
            self.hs_off.append(off)
            off += self.tab_alloc[t] + GUARD
        self.hs_len = off
        self.sk_off, self.sk_len = GUARD, self.staging_cap + 2 * GUARD

    # -- views into flat buffers
    def host_rows(self, buf, t):
        o, n, d = self.tab_off[t], self.tab_alloc[t], self.tab_D[t]
        return buf[o:o + n * d].reshape(n, d)

    def host_state_rows(self, buf, t):
        return buf[self.hs_off[t]:self.hs_off[t] + self.tab_alloc[t]]

    def dev_rows(self, buf):
        return buf[self.rows_off:self.rows_off + self.rows_len].reshape(self.n_slots, self.row_stride)

    def dev_state(self, buf):
        return buf[self.state_off:self.state_off + self.n_slots]

    def staging_keys(self, buf):
        return buf[self.sk_off:self.sk_off + self.staging_cap]

    # -- values
    def table_of(self, keys):
        return np.searchsorted(self.key_base, np.asarray(keys, dtype=np.int64), side="right") - 1

    def initial_host(self):
        buf = np.full(self.host_len, F_CANARY, dtype=np.float32)
        for t in range(self.Tc):
            keys = int(self.key_base[t]) + np.arange(self.tab_alloc[t], dtype=np.int64)
            self.host_rows(buf, t)[...] = ((keys[:, None] * 7 + np.arange(self.tab_D[t])[None, :] * 3) % 1021).astype(np.float32)
        return buf

    def initial_host_state(self):
        buf = np.full(self.hs_len, F_CANARY, dtype=np.float32)
        for t in range(self.Tc):
            keys = int(self.key_base[t]) + np.arange(self.tab_alloc[t], dtype=np.int64)
            self.host_state_rows(buf, t)[...] = (keys % 97 + 1).astype(np.float32)
        return buf

    @staticmethod
    def delta(keys, step, D):
        keys = np.asarray(keys, dtype=np.int64)
        return ((keys % 7 + step % 5 + 1)[:, None] + (np.arange(D) % 3)[None, :]).astype(np.float32)

    # -- what cache_linearize_kernel computes
    def window_array(self):
        return None if self.feat_window is None else np.array(self.feat_window, dtype=np.int64).reshape(-1)

    def linearize(self, indices, offsets, feat_window=None):
        """(key per position or -1, class per position).  Feature of p = the largest f with offsets[f*B] <= p."""
        indices = np.asarray(indices, dtype=np.int64)
        N = indices.size
        B = (len(offsets) - 1) // self.F
        fb = np.asarray(offsets, dtype=np.int64)[::B][:self.F]
        f = np.searchsorted(fb, np.arange(N), side="right") - 1
        ctab = np.array(self.feat_ctab, dtype=np.int64)[f]
        rows = np.array(self.feat_rows, dtype=np.int64)[f]
        if feat_window is None:
            lo, glob = np.zeros(N, dtype=np.int64), rows
        else:
            w = np.asarray(feat_window, dtype=np.int64).reshape(-1, 2)
            lo, glob = w[f, 0], w[f, 1]
        u = indices.astype(np.uint64)
        local = u - lo.astype(np.uint64)  # wraps like the kernel's unsigned subtraction
        is_local = local < rows.astype(np.uint64)
        is_foreign = ~is_local & ((indices == TBE_ID_SKIP) | (u < glob.astype(np.uint64)))
        cls = np.where(ctab < 0, UNCACHED, np.where(is_local, LOCAL, np.where(is_foreign, FOREIGN, BAD)))
        key = np.full(N, -1, dtype=np.int64)
        sel = cls == LOCAL
        key[sel] = self.key_base[ctab[sel]] + local[sel].astype(np.int64)
        return key, cls


class Snap:
    """Every byte a cache call may touch, read back."""
    FIELDS = ("tags", "lru", "counters", "skeys", "devf", "host", "hstate")

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Pred:
    pass


class Model:
    """tags / lru / totals, the logical tables (what a row's value IS) and the host image (what host memory must hold:
    stale for rows that are dirty in the cache)."""

    def __init__(self, g):
        self.g = g
        self.tags = np.full(g.slots, -1, dtype=np.int64)
        self.lru = np.full(g.slots, -1, dtype=np.int32)
        self.hits = self.misses = self.evictions = 0
        self.host, self.hstate = g.initial_host(), g.initial_host_state()
        self.logical = [g.host_rows(self.host, t).copy() for t in range(g.Tc)]
        self.logical_state = [g.host_state_rows(self.hstate, t).copy() for t in range(g.Tc)]

    def local_of(self, keys):
        keys = np.asarray(keys, dtype=np.int64)
        t = self.g.table_of(keys)
        return t, keys - self.g.key_base[t]

    def make_logical(self, host, hstate, keys):
        """host / hstate images with the rows of `keys` brought up to their logical values."""
        t, r = self.local_of(keys)
        for tt, rr in zip(t.tolist(), r.tolist()):
            self.g.host_rows(host, tt)[rr] = self.logical[tt][rr]
            if self.g.state:
                self.g.host_state_rows(hstate, tt)[rr] = self.logical_state[tt][rr]

    def predict(self, pos_keys, it, policy="lru"):
        g, p = self.g, Pred()
        p.it = int(it)
        p.U = np.unique(pos_keys[pos_keys >= 0])
        where = {k: s for s, k in enumerate(self.tags.tolist()) if k >= 0}
        is_hit = np.array([k in where for k in p.U.tolist()], dtype=bool)
        p.H, p.M = p.U[is_hit], p.U[~is_hit]
        p.hit_slots = np.array([where[k] for k in p.H.tolist()], dtype=np.int64)
        p.lru = self.lru.copy()
        p.lru[p.hit_slots] = it
        marked = p.lru.copy()
        msets = set_of(p.M, g.num_sets)
        p.sets, p.claimed_slots, p.evicted, p.staged = {}, [], [], 0
        p.tie = p.full_set_more_misses = False
        for s in range(g.num_sets):
            Ms = p.M[msets == s]
            sl = slice(s * WAYS, (s + 1) * WAYS)
            cand = POLICIES[policy](self.lru[sl], marked[sl], it)
            n = min(Ms.size, cand.size)
            claimed = cand[:n]
            p.sets[s] = dict(M=Ms, cand=cand, claimed=claimed, staged=Ms.size - n)
            p.staged += Ms.size - n
            p.claimed_slots.extend((s * WAYS + claimed).tolist())
            if 0 < n < cand.size and marked[sl][cand[n - 1]] == marked[sl][cand[n]]:
                p.tie = True
            if Ms.size > 0 and int((marked[sl] == it).sum()) == WAYS:
                p.full_set_more_misses = True
        p.claimed_slots = np.array(sorted(p.claimed_slots), dtype=np.int64)
        p.lru[p.claimed_slots] = it
        old = self.tags[p.claimed_slots]
        p.evicted = old[old >= 0]
        p.counters = [p.staged, self.hits + p.H.size, self.misses + p.M.size, self.evictions + p.evicted.size, p.U.size, p.M.size]
        return p


class CacheCase:
    """One cache (geometry + backend) with its model.  Every method runs one call, verifies every byte and raises an
    AssertionError naming the step, the set, the way and the path (hit, claimed-empty, claimed-evict, staged)."""

    def __init__(self, g, backend, seed=0):
        self.g, self.be, self.model = g, backend, Model(g)
        self.step_no = 0
        self.last = None
        self.unwritten = False  # staged rows were updated and not written back yet
        self.snap = backend.snapshot()
        exp = self._expected(self.snap)
        exp.host, exp.hstate = self.model.host, self.model.hstate
        self._compare("initial state", exp, self.snap, None)
        # the keys a sequence may draw, each once, in a fixed shuffled order
        rng = np.random.default_rng([seed, g.total % 1000003, g.Tc])
        self.feat_of_tab = {}
        for f, c in enumerate(g.feat_ctab):
            if c >= 0 and c not in self.feat_of_tab:
                self.feat_of_tab[c] = f
        keys = np.concatenate([int(g.key_base[t]) + np.arange(g.tab_alloc[t], dtype=np.int64) for t in sorted(self.feat_of_tab)])
        rng.shuffle(keys)
        if g.must_include_last:
            last = g.total - 1
            keys = np.concatenate([[last], keys[keys != last]])
        self.pool, self._taken = keys, 0

    # -- building batches
    def take(self, n):
        assert self._taken + n <= self.pool.size, "the geometry has too few rows for this sequence"
        out = self.pool[self._taken:self._taken + n]
        self._taken += n
        return out

    def pairs(self, keys, feature=None):
        """(feature, id) of every key, through the first feature of its table (or `feature`)."""
        t, r = self.model.local_of(keys)
        out = []
        for tt, rr in zip(t.tolist(), r.tolist()):
            f = self.feat_of_tab[tt] if feature is None else feature
            lo = self.g.feat_window[f][0] if self.g.feat_window is not None else 0
            out.append((f, rr + lo))
        return out

    def batch(self, per_feature, B=2):
        """indices / offsets of F*B bags: feature f's ids in order, cut into B bags of near-equal length."""
        lengths, ids = [], []
        for f in range(self.g.F):
            n = len(per_feature[f])
            ids.extend(per_feature[f])
            lengths.extend(n // B + (1 if b < n % B else 0) for b in range(B))
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        return np.array(ids, dtype=np.int64), offsets

    def batch_of_pairs(self, pairs, B=2):
        per = [[] for _ in range(self.g.F)]
        for f, i in pairs:
            per[f].append(i)
        return self.batch(per, B)

    # -- verification helpers
    def _expected(self, snap):
        return Snap(**{k: getattr(snap, k).copy() for k in Snap.FIELDS})

    def _way_name(self, slot, key=None):
        g = self.g
        if slot < g.slots:
            return "set %d way %d" % (slot // WAYS, slot % WAYS)
        s = "" if key is None or key < 0 else "set %d " % set_of_int(key, g.num_sets)
        return s + "staging slot %d" % (slot - g.slots)

    def _fail(self, what, where, path, msg):
        raise AssertionError("%s, step %d: %s, path %s: %s" % (what, self.step_no, where, path, msg))

    def _slot_path(self, slot, pred):
        if pred is None:
            return "none"
        if slot in pred.path_of_slot:
            return pred.path_of_slot[slot]
        return "untouched"

    def _compare(self, what, exp, got, pred):
        g = self.g
        for name in Snap.FIELDS:
            e, a = getattr(exp, name), getattr(got, name)
            assert e.shape == a.shape and e.dtype == a.dtype, (name, e.shape, a.shape, e.dtype, a.dtype)
            eb = e.view(np.uint32) if e.dtype == np.float32 else e
            ab = a.view(np.uint32) if a.dtype == np.float32 else a
            bad = np.nonzero(eb != ab)[0]
            if bad.size == 0:
                continue
            i = int(bad[0])
            detail = "%s[%d] is %r, expected %r (%d elements differ)" % (name, i, a[i].item(), e[i].item(), bad.size)
            if name == "devf":
                if g.rows_off <= i < g.rows_off + g.rows_len:
                    slot, col = divmod(i - g.rows_off, g.row_stride)
                    self._fail(what, self._way_name(slot, self._key_at(got, slot)), self._slot_path(slot, pred),
                               "rows column %d: %s" % (col, detail))
                if g.state_off <= i < g.state_off + g.n_slots:
                    slot = i - g.state_off
                    self._fail(what, self._way_name(slot, self._key_at(got, slot)), self._slot_path(slot, pred), "state: " + detail)
                self._fail(what, "outside rows and state", "guard", detail)
            if name in ("host", "hstate"):
                offs, width = (g.tab_off, g.tab_D) if name == "host" else (g.hs_off, [1] * g.Tc)
                for t in range(g.Tc):
                    if offs[t] <= i < offs[t] + g.tab_alloc[t] * width[t]:
                        row, col = divmod(i - offs[t], width[t])
                        key = int(g.key_base[t]) + row
                        where, path = "no slot", "untouched"
                        if pred is not None and key in pred.slot_of_written_key:
                            slot = pred.slot_of_written_key[key]
                            where, path = self._way_name(slot, key), pred.write_path
                        self._fail(what, where, path, "host %s of table %d row %d (key %d) column %d: %s"
                                   % ("state" if name == "hstate" else "row", t, row, key, col, detail))
                self._fail(what, "outside every host table", "guard", detail)
            if name in ("tags", "lru"):
                self._fail(what, self._way_name(i), self._slot_path(i, pred), detail)
            self._fail(what, "-", "guard" if name == "skeys" else "counters", detail)

    def _key_at(self, snap, slot):
        g = self.g
        if slot < g.slots:
            return int(snap.tags[slot])
        k = slot - g.slots
        return int(g.staging_keys(snap.skeys)[k]) if k < int(snap.counters[0]) else -1

    def check_guards(self):
        """Canaries round every host table, the host state, rows, state and staging_keys, and columns
        max(tab_D) .. row_stride of every slot."""
        g, s = self.g, self.snap
        gap = np.ones(g.host_len, dtype=bool)
        for t in range(g.Tc):
            gap[g.tab_off[t]:g.tab_off[t] + g.tab_alloc[t] * g.tab_D[t]] = False
        assert (s.host[gap].view(np.uint32) == F_CANARY.view(np.uint32)).all(), "canary round a host table damaged"
        gap = np.ones(g.hs_len, dtype=bool)
        for t in range(g.Tc):
            gap[g.hs_off[t]:g.hs_off[t] + g.tab_alloc[t]] = False
        assert (s.hstate[gap].view(np.uint32) == F_CANARY.view(np.uint32)).all(), "canary round the host state damaged"
        gap = np.ones(g.devf_len, dtype=bool)
        gap[g.rows_off:g.rows_off + g.rows_len] = False
        if g.state:
            gap[g.state_off:g.state_off + g.n_slots] = False
        assert (s.devf[gap].view(np.uint32) == F_CANARY.view(np.uint32)).all(), "canary round rows / state damaged"
        tail = g.dev_rows(s.devf)[:, max(g.tab_D):]
        assert (tail.view(np.uint32) == F_CANARY.view(np.uint32)).all(), "columns D..row_stride of a slot damaged"
        sk = s.skeys
        assert (sk[:g.sk_off] == I_CANARY).all() and (sk[g.sk_off + g.staging_cap:] == I_CANARY).all(), "canary round staging_keys damaged"
        assert self.be.remapped_guards_ok(), "canary round remapped_indices damaged"

    # -- the four calls
    def prefetch(self, indices, offsets, it, feat_window=None):
        g, m = self.g, self.model
        assert not self.unwritten, "harness misuse: update() of staged rows without writeback_staging()"
        self.step_no += 1
        what = "prefetch(iteration %d)" % it
        indices = np.asarray(indices, dtype=np.int64)
        if feat_window is None:
            feat_window = g.window_array()
        before = self.snap
        pos_keys, cls = g.linearize(indices, offsets, feat_window)
        pred = m.predict(pos_keys, it)
        rc = self.be.prefetch(indices, offsets, it, feat_window)
        assert rc == 0, "%s returned %d: %s" % (what, rc, self.be.last_error())
        got = self.be.snapshot()
        remapped = self.be.remapped()
        # paths of the slots the prediction names (claimed ways are fixed; which key each holds is read back)
        pred.path_of_slot = {int(s): "hit" for s in pred.hit_slots}
        for s in pred.claimed_slots.tolist():
            pred.path_of_slot[s] = "claimed-empty" if m.tags[s] < 0 else "claimed-evict"
        for k in range(pred.staged):
            pred.path_of_slot[g.slots + k] = "staged"
        pred.write_path = "claimed-evict"
        pred.slot_of_written_key = {int(m.tags[s]): s for s in pred.claimed_slots.tolist() if m.tags[s] >= 0}
        # tags / lru: unclaimed ways keep their tag, lru = it exactly on hit and claimed ways
        claimed = np.zeros(g.slots, dtype=bool)
        claimed[pred.claimed_slots] = True
        bad = np.nonzero(~claimed & (got.tags != m.tags))[0]
        if bad.size:
            s = int(bad[0])
            self._fail(what, self._way_name(s), self._slot_path(s, pred), "the tag of a way the policy does not claim changed from %d to %d"
                       % (m.tags[s], got.tags[s]))
        bad = np.nonzero(got.lru != pred.lru)[0]
        if bad.size:
            s = int(bad[0])
            self._fail(what, self._way_name(s), self._slot_path(s, pred), "lru is %d, expected %d" % (got.lru[s], pred.lru[s]))
        staged_keys = g.staging_keys(got.skeys)[:pred.staged].copy()
        for s, d in pred.sets.items():
            new = got.tags[s * WAYS + d["claimed"]]
            for w, k in zip(d["claimed"].tolist(), new.tolist()):
                if k not in d["M"]:
                    slot = s * WAYS + w
                    self._fail(what, self._way_name(slot), self._slot_path(slot, pred), "new tag %d is not a missed key of this set" % k)
            if np.unique(new).size != new.size:
                self._fail(what, "set %d" % s, "claimed", "one missed key was inserted into two ways: %r" % sorted(new.tolist()))
        landed = np.sort(np.concatenate([got.tags[pred.claimed_slots], staged_keys]))
        if not np.array_equal(landed, pred.M):
            self._fail(what, "-", "claimed + staged", "the claimed ways' new tags and staging_keys[0:%d] do not partition the missed keys: %r vs %r"
                       % (pred.staged, landed.tolist(), pred.M.tolist()))
        live = np.concatenate([got.tags[got.tags >= 0], staged_keys])
        if np.unique(live).size != live.size:
            self._fail(what, "-", "any", "a key appears twice in tags + staging_keys")
        vs = np.nonzero(got.tags >= 0)[0]
        wrong = vs[set_of(got.tags[vs], g.num_sets) != vs // WAYS]
        if wrong.size:
            s = int(wrong[0])
            self._fail(what, self._way_name(s), self._slot_path(s, pred), "tag %d belongs to set %d" % (got.tags[s], set_of_int(got.tags[s], g.num_sets)))
        # counters (after the ways, so that a wrong victim is reported by its way)
        for i, name in enumerate(("staged rows", "hits", "misses", "evictions", "unique rows", "misses of this batch")):
            if int(got.counters[i]) != pred.counters[i]:
                self._fail(what, "-", "counters", "counters[%d] (%s) is %d, expected %d" % (i, name, got.counters[i], pred.counters[i]))
        # remapped ids
        assert remapped.shape == indices.shape
        slot_key = np.concatenate([got.tags, staged_keys, np.full(g.staging_cap - pred.staged, -2, dtype=np.int64)])
        passthrough = np.where(cls == UNCACHED, indices, np.where(cls == FOREIGN, TBE_ID_SKIP, -1))
        for p in np.nonzero(cls != LOCAL)[0].tolist():
            if remapped[p] != passthrough[p]:
                self._fail(what, "position %d" % p, ("local", "foreign", "bad", "uncached")[cls[p]],
                           "id %d was remapped to %d, expected %d" % (indices[p], remapped[p], passthrough[p]))
        for p in np.nonzero(cls == LOCAL)[0].tolist():
            slot = int(remapped[p])
            if not (0 <= slot < g.n_slots) or slot_key[slot] != pos_keys[p]:
                inside = 0 <= slot < g.n_slots
                self._fail(what, self._way_name(slot, int(pos_keys[p])) if inside else "position %d" % p,
                           self._slot_path(slot, pred), "position %d (key %d) was remapped to slot %d, which holds key %s"
                           % (p, pos_keys[p], slot, slot_key[slot] if inside else "nothing"))
        # rows / state: inserted slots hold the logical row in columns 0..D, every other float is unchanged
        exp = self._expected(before)
        exp.tags, exp.lru, exp.counters = got.tags, got.lru, got.counters  # verified above
        g.staging_keys(exp.skeys)[:pred.staged] = staged_keys
        rows, state = g.dev_rows(exp.devf), g.dev_state(exp.devf)
        ins_slots = np.concatenate([pred.claimed_slots, g.slots + np.arange(pred.staged, dtype=np.int64)])
        ins_keys = slot_key[ins_slots]
        t, r = m.local_of(ins_keys)
        for slot, tt, rr in zip(ins_slots.tolist(), t.tolist(), r.tolist()):
            rows[slot, :g.tab_D[tt]] = m.logical[tt][rr]
            if g.state:
                state[slot] = m.logical_state[tt][rr]
        m.make_logical(exp.host, exp.hstate, pred.evicted)
        self._compare(what, exp, got, pred)
        # hit slots: unchanged by the call (above) and still the logical row
        t, r = m.local_of(pred.H)
        got_rows, got_state = g.dev_rows(got.devf), g.dev_state(got.devf)
        for slot, tt, rr in zip(pred.hit_slots.tolist(), t.tolist(), r.tolist()):
            D = g.tab_D[tt]
            if not np.array_equal(got_rows[slot, :D].view(np.uint32), m.logical[tt][rr].view(np.uint32)) or (
                    g.state and got_state[slot] != m.logical_state[tt][rr]):
                self._fail(what, self._way_name(slot), "hit", "the cached row of key %d is not the logical row" % m.tags[slot])
        # adopt
        m.tags, m.lru = got.tags.copy(), got.lru.copy()
        m.hits, m.misses, m.evictions = pred.counters[1:4]
        m.host, m.hstate = exp.host, exp.hstate
        self.snap = got
        pred.slot_key, pred.staged_keys = slot_key, staged_keys
        pred.touched = np.unique(remapped[cls == LOCAL])
        pred.remapped, pred.cls, pred.pos_keys = remapped, cls, pos_keys
        self.last = pred
        self.check_guards()
        return pred

    def update(self, step):
        """Stands in for the backward: an integer delta from (key, step) on columns 0..D of every touched slot, +1 on
        its state; the same on the logical tables."""
        g, m, last = self.g, self.model, self.last
        what = "update(%d)" % step
        slots = last.touched
        keys = last.slot_key[slots]
        t, r = m.local_of(keys)
        exp = self._expected(self.snap)
        rows, state = g.dev_rows(exp.devf), g.dev_state(exp.devf)
        for tt in np.unique(t).tolist():
            sel = t == tt
            D = g.tab_D[tt]
            d = g.delta(keys[sel], step, D)
            self.be.add_rows(slots[sel], D, d)
            rows[slots[sel], :D] += d
            m.logical[tt][r[sel]] += d
            if g.state:
                m.logical_state[tt][r[sel]] += 1
        if g.state and slots.size:
            self.be.add_state(slots)
            state[slots] += 1
        got = self.be.snapshot()
        self._compare(what, exp, got, last)
        self.snap = got
        self.unwritten = last.staged > 0

    def writeback_staging(self):
        m, last = self.model, self.last
        exp = self._expected(self.snap)
        m.make_logical(exp.host, exp.hstate, last.staged_keys)
        last.write_path = "staged"
        last.slot_of_written_key = {int(k): self.g.slots + i for i, k in enumerate(last.staged_keys.tolist())}
        rc = self.be.writeback_staging()
        assert rc == 0, "writeback_staging returned %d: %s" % (rc, self.be.last_error())
        got = self.be.snapshot()
        self._compare("writeback_staging", exp, got, last)
        m.host, m.hstate, self.snap, self.unwritten = exp.host, exp.hstate, got, False
        self.check_guards()

    def flush(self, invalidate):
        g, m = self.g, self.model
        assert not self.unwritten, "harness misuse: flush() before writeback_staging()"
        exp = self._expected(self.snap)
        valid = np.nonzero(m.tags >= 0)[0]
        m.make_logical(exp.host, exp.hstate, m.tags[valid])
        pred = Pred()
        pred.path_of_slot = {int(s): "flush" for s in valid}
        pred.write_path = "flush"
        pred.slot_of_written_key = {int(m.tags[s]): int(s) for s in valid}
        if invalidate:
            exp.tags[:] = -1
            exp.lru[:] = -1
        rc = self.be.flush(int(invalidate))
        assert rc == 0, "flush returned %d: %s" % (rc, self.be.last_error())
        got = self.be.snapshot()
        self._compare("flush(%d)" % invalidate, exp, got, pred)
        m.host, m.hstate, self.snap = exp.host, exp.hstate, got
        m.tags, m.lru = got.tags.copy(), got.lru.copy()
        self.check_guards()

    def finish(self):
        """flush(0) then flush(1); afterwards host memory holds every logical row."""
        self.flush(0)
        self.flush(1)
        for t in range(self.g.Tc):
            assert np.array_equal(self.g.host_rows(self.snap.host, t).view(np.uint32), self.model.logical[t].view(np.uint32))
            if self.g.state:
                assert np.array_equal(self.g.host_state_rows(self.snap.hstate, t), self.model.logical_state[t])

    def train_step(self, keys, it, step=None, update=True, B=2):
        """prefetch of one id per key (through the first feature of its table), update, writeback_staging."""
        indices, offsets = self.batch_of_pairs(self.pairs(keys), B)
        info = self.prefetch(indices, offsets, it)
        if update:
            self.update(self.step_no if step is None else step)
            self.writeback_staging()
        return info


# ---- the numpy stand-in for the library ---------------------------------------------------------------------------------
class SimBackend:
    """The cache's contract restated in numpy, with a replacement policy to choose and missed keys handed to the claimed
    ways in DESCENDING key order (any assignment is legal).  Tests the verifier; proves nothing about the library."""

    def __init__(self, g, policy="lru"):
        self.g, self.policy = g, policy
        self.tags = np.full(g.slots, -1, dtype=np.int64)
        self.lru = np.full(g.slots, -1, dtype=np.int32)
        self.counters = np.zeros(8, dtype=np.int32)
        self.skeys = np.full(g.sk_len, I_CANARY, dtype=np.int64)
        self.devf = np.full(g.devf_len, F_CANARY, dtype=np.float32)
        self.host, self.hstate = g.initial_host(), g.initial_host_state()
        self._remapped = np.zeros(0, dtype=np.int64)

    def last_error(self):
        return ""

    def remapped_guards_ok(self):
        return True

    def remapped(self):
        return self._remapped.copy()

    def snapshot(self):
        return Snap(**{k: getattr(self, k).copy() for k in Snap.FIELDS})

    def _copy(self, key, slot, to_host):
        g = self.g
        t = int(g.table_of(key))
        r = int(key - g.key_base[t])
        D = g.tab_D[t]
        h, d = g.host_rows(self.host, t), g.dev_rows(self.devf)
        if to_host:
            h[r] = d[slot, :D]
        else:
            d[slot, :D] = h[r]
        if g.state:
            hs, ds = g.host_state_rows(self.hstate, t), g.dev_state(self.devf)
            if to_host:
                hs[r] = ds[slot]
            else:
                ds[slot] = hs[r]

    def prefetch(self, indices, offsets, it, feat_window):
        g, c = self.g, self.counters
        c[0] = c[4] = c[5] = 0
        indices = np.asarray(indices, dtype=np.int64)
        self._remapped = np.zeros(indices.size, dtype=np.int64)
        if indices.size == 0:
            return 0
        keys, cls = g.linearize(indices, offsets, feat_window)
        out = np.where(cls == UNCACHED, indices, np.where(cls == FOREIGN, TBE_ID_SKIP, -1))
        U = np.unique(keys[keys >= 0])
        c[4] = U.size
        old = self.lru.copy()
        where = {int(k): s for s, k in enumerate(self.tags.tolist()) if k >= 0}
        slot_of, miss = {}, []
        for k in U.tolist():
            if k in where:
                slot_of[k] = where[k]
                self.lru[where[k]] = it
                c[1] += 1
            else:
                miss.append(k)
        c[5] = len(miss)
        marked = self.lru.copy()
        msets = set_of(miss, g.num_sets) if miss else np.zeros(0, dtype=np.int64)
        for s in range(g.num_sets):
            Ms = sorted((k for k, ss in zip(miss, msets.tolist()) if ss == s), reverse=True)
            sl = slice(s * WAYS, (s + 1) * WAYS)
            cand = POLICIES[self.policy](old[sl], marked[sl], it).tolist()
            for i, k in enumerate(Ms):
                c[2] += 1
                if i < len(cand):
                    slot = s * WAYS + cand[i]
                    if self.tags[slot] >= 0:
                        self._copy(int(self.tags[slot]), slot, True)
                        c[3] += 1
                    self.tags[slot], self.lru[slot] = k, it
                else:
                    slot = g.slots + int(c[0])
                    g.staging_keys(self.skeys)[c[0]] = k
                    c[0] += 1
                self._copy(k, slot, False)
                slot_of[k] = slot
        sel = cls == LOCAL
        out[sel] = [slot_of[k] for k in keys[sel].tolist()]
        self._remapped = out
        return 0

    def add_rows(self, slots, width, delta):
        self.g.dev_rows(self.devf)[slots, :width] += delta

    def add_state(self, slots):
        self.g.dev_state(self.devf)[slots] += 1

    def writeback_staging(self):
        g = self.g
        for k in range(int(self.counters[0])):
            self._copy(int(g.staging_keys(self.skeys)[k]), g.slots + k, True)
        return 0

    def flush(self, invalidate):
        for s in range(self.g.slots):
            if self.tags[s] >= 0:
                self._copy(int(self.tags[s]), s, True)
        if invalidate:
            self.tags[:] = -1
            self.lru[:] = -1
        return 0


# ---- the library ----------------------------------------------------------------------------------------------------------
class GpuBackend:
    """Host tables in pinned memory (torch.zeros(...).pin_memory(), addresses passed as the module's _RowCache.desc does),
    device buffers between canaries, `tags` 16-B aligned; every call synchronises before it returns."""

    def __init__(self, g):
        import torch
        from fbgemm_gpu import _lib

        self.g, self.torch, self._lib, self.lib = g, torch, _lib, _lib.load()
        self.dev = torch.device("cuda", 0)
        dev = self.dev
        self.host = torch.zeros(g.host_len, dtype=torch.float32).pin_memory()
        self.host.copy_(torch.from_numpy(g.initial_host()))
        self.hstate = torch.zeros(g.hs_len, dtype=torch.float32).pin_memory()
        self.hstate.copy_(torch.from_numpy(g.initial_host_state()))
        assert self.host.data_ptr() % 16 == 0
        for t in range(g.Tc):
            assert (self.host.data_ptr() + 4 * g.tab_off[t]) % 16 == 4 * g.host_off[t]
        self.devf = torch.full((g.devf_len,), float(F_CANARY), dtype=torch.float32, device=dev)
        assert (self.devf.data_ptr() + 4 * g.rows_off) % 16 == 0
        self.tags_buf = torch.full((g.slots + 2,), -1, dtype=torch.int64, device=dev)
        assert self.tags_buf.data_ptr() % 16 == 0
        self.tags = self.tags_buf[:g.slots]
        self.lru = torch.full((g.slots,), -1, dtype=torch.int32, device=dev)
        self.counters = torch.zeros(8, dtype=torch.int32, device=dev)
        self.skeys = torch.full((g.sk_len,), I_CANARY, dtype=torch.int64, device=dev)
        self.tab_key_base = torch.from_numpy(g.key_base).to(dev)
        self.tab_weights = torch.tensor([self.host.data_ptr() + 4 * o for o in g.tab_off], dtype=torch.int64).to(dev)
        self.tab_state = torch.tensor([self.hstate.data_ptr() + 4 * o for o in g.hs_off], dtype=torch.int64).to(dev) if g.state else None
        self.tab_D = torch.tensor(g.tab_D, dtype=torch.int32).to(dev)
        self.feat_ctab = torch.tensor(g.feat_ctab, dtype=torch.int32).to(dev)
        self.feat_rows = torch.tensor(g.feat_rows, dtype=torch.int64).to(dev)
        self._rem = torch.full((2 * GUARD,), I_CANARY, dtype=torch.int64, device=dev)
        self._n = 0
        torch.cuda.synchronize()

    def desc(self, staging_cap=None, tags_shift=0):
        g, p = self.g, self._lib.ptr
        return self._lib.CacheDesc(
            p(self.tags) + tags_shift, p(self.lru), p(self.devf) + 4 * g.rows_off, (p(self.devf) + 4 * g.state_off) if g.state else None,
            p(self.skeys) + 8 * g.sk_off, p(self.counters), p(self.tab_key_base), p(self.tab_weights), p(self.tab_state),
            p(self.tab_D), g.num_sets, g.row_stride, g.staging_cap if staging_cap is None else staging_cap, g.Tc)

    def last_error(self):
        msg = self.lib.tbe_last_error()
        return msg.decode() if msg else ""

    def _done(self):
        self.torch.cuda.synchronize()
        assert self._lib.fault_count() == self._faults, "the pair sort gave up on a spin-wait"

    def prefetch(self, indices, offsets, it, feat_window, staging_cap=None, ws_short=0, ws_shift=0, key_bits=None, tags_shift=0):
        import ctypes

        torch, g, p = self.torch, self.g, self._lib.ptr
        N = int(np.asarray(indices).size)
        B = (len(offsets) - 1) // g.F
        ind = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int64)).to(self.dev)
        off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(self.dev)
        win = None if feat_window is None else torch.from_numpy(np.ascontiguousarray(feat_window, dtype=np.int64)).to(self.dev)
        rem = torch.full((N + 2 * GUARD,), I_CANARY, dtype=torch.int64, device=self.dev)
        nbytes = int(self.lib.tbe_cache_prefetch_workspace_bytes(N, g.key_bits))
        assert nbytes > 0
        raw = torch.full((nbytes + 768,), 0xFF, dtype=torch.uint8, device=self.dev)
        ws = (raw.data_ptr() + 255) // 256 * 256 + ws_shift
        self._faults = self._lib.fault_count()
        d = self.desc(staging_cap, tags_shift)
        rc = self.lib.tbe_cache_prefetch(ctypes.byref(d), p(self.feat_ctab), p(self.feat_rows), g.F, B, p(ind), N, p(off),
                                         g.key_bits if key_bits is None else key_bits, int(it), rem.data_ptr() + 8 * GUARD, ws,
                                         nbytes - ws_short, p(win), self._lib.stream_ptr(self.dev))
        self._done()
        self._rem, self._n = rem, N
        return rc

    def remapped(self):
        return self._rem[GUARD:GUARD + self._n].cpu().numpy().copy()

    def remapped_guards_ok(self):
        r = self._rem.cpu().numpy()
        return bool((r[:GUARD] == I_CANARY).all() and (r[GUARD + self._n:] == I_CANARY).all())

    def writeback_staging(self):
        import ctypes

        self._faults = self._lib.fault_count()
        d = self.desc()
        rc = self.lib.tbe_cache_writeback_staging(ctypes.byref(d), self._lib.stream_ptr(self.dev))
        self._done()
        return rc

    def flush(self, invalidate):
        import ctypes

        self._faults = self._lib.fault_count()
        d = self.desc()
        rc = self.lib.tbe_cache_flush(ctypes.byref(d), int(invalidate), self._lib.stream_ptr(self.dev))
        self._done()
        return rc

    def _rows(self):
        g = self.g
        return self.devf[g.rows_off:g.rows_off + g.rows_len].view(g.n_slots, g.row_stride)

    def add_rows(self, slots, width, delta):
        idx = self.torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).to(self.dev)
        d = self.torch.from_numpy(np.ascontiguousarray(delta, dtype=np.float32)).to(self.dev)
        rows = self._rows()
        rows[idx, :width] = rows[idx, :width] + d  # slots are unique
        self.torch.cuda.synchronize()

    def add_state(self, slots):
        g = self.g
        idx = self.torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).to(self.dev) + g.state_off
        self.devf[idx] = self.devf[idx] + 1
        self.torch.cuda.synchronize()

    def snapshot(self):
        self.torch.cuda.synchronize()
        return Snap(tags=self.tags.cpu().numpy().copy(), lru=self.lru.cpu().numpy().copy(), counters=self.counters.cpu().numpy().copy(),
                    skeys=self.skeys.cpu().numpy().copy(), devf=self.devf.cpu().numpy().copy(), host=self.host.numpy().copy(),
                    hstate=self.hstate.numpy().copy())


def make_case(backend="gpu", policy="lru", seed=0, **geometry):
    g = Geometry(**geometry)
    return CacheCase(g, GpuBackend(g) if backend == "gpu" else SimBackend(g, policy), seed=seed)


# ---- geometries (keyword arguments of Geometry; num_sets is set by the sequence) ---------------------------------------
G6_ROWS = [2 + t % 4 for t in range(70)]
GEOMETRIES = {
    "G1_D64_state": dict(tab_rows=[300, 41], tab_D=64, state=True),
    "G2_D260": dict(tab_rows=[300, 41], tab_D=260),
    "G3_D12_host_4B_off": dict(tab_rows=[300, 41], tab_D=12, host_off=[1, 1]),
    "G4_D13": dict(tab_rows=[300, 41], tab_D=13, state=True),
    "G4_D67": dict(tab_rows=[300, 41], tab_D=67),
    "G4_D1": dict(tab_rows=[300, 41], tab_D=1, state=True),
    "G5_stride64": dict(tab_rows=[150, 120, 90], tab_D=[8, 64, 20], row_stride=64),
    "G5_stride66": dict(tab_rows=[150, 120, 90], tab_D=[8, 64, 20], row_stride=66),
    "G6_70_tables": dict(tab_rows=G6_ROWS, tab_D=8, state=True),
    "G7_keys_above_2^32": dict(tab_rows=[2 ** 33 + 100, 40], tab_alloc=[512, 40], tab_D=16, state=True),
    "rows_2^10-1": dict(tab_rows=[1000, 23], tab_D=8, must_include_last=True),
    "rows_2^10": dict(tab_rows=[1000, 24], tab_D=8, must_include_last=True),
}


# ---- sequences: each returns the Pred of its prefetches --------------------------------------------------------------
def ways_of(case, keys):
    tags = case.model.tags
    return sorted(int(np.nonzero(tags == k)[0][0]) % WAYS for k in np.asarray(keys).tolist())


def seq_lru(case, it0=1):
    """num_sets = 1.  Four generations of 16 keys fill the ways in way order; a step that hits generation 0 and misses 16
    must take generation 1's ways; a step that misses 20 takes generation 2's ways and the first four of generation 3's."""
    assert case.g.num_sets == 1
    infos, gens = [], []
    for j in range(4):
        gens.append(case.take(16))
        infos.append(case.train_step(gens[j], it0 + j))
        assert ways_of(case, gens[j]) == list(range(16 * j, 16 * j + 16)), "generation %d does not sit in ways %d.." % (j, 16 * j)
    new = case.take(16)
    info = case.train_step(np.concatenate([gens[0], new]), it0 + 4)
    infos.append(info)
    assert info.sets[0]["claimed"].tolist() == list(range(16, 32)) and sorted(info.evicted.tolist()) == sorted(gens[1].tolist())
    assert ways_of(case, new) == list(range(16, 32)) and ways_of(case, gens[0]) == list(range(16))
    oldest = case.model.tags[32:52].copy()
    info = case.train_step(case.take(20), it0 + 5)
    infos.append(info)
    assert info.sets[0]["claimed"].tolist() == list(range(32, 52)) and sorted(info.evicted.tolist()) == sorted(oldest.tolist())
    assert set(gens[2].tolist()) <= set(oldest.tolist()) and len(set(gens[3].tolist()) & set(oldest.tolist())) == 4  # two ages
    case.finish()
    return infos


def seq_staging(case, it0=1):
    """num_sets = 1.  100 keys at an empty cache (64 cached, 36 staged); all 64 hit + 10 misses (10 staged, no candidate);
    the 46 staged keys again (they come back from the host, updated); a forward-only step that stages."""
    assert case.g.num_sets == 1
    infos = []
    first = case.take(100)
    infos.append(case.train_step(first, it0))
    assert infos[-1].staged == 36 and infos[-1].evicted.size == 0
    cached = case.model.tags.copy()
    assert (cached >= 0).all()
    ten = case.take(10)
    infos.append(case.train_step(np.concatenate([cached, ten]), it0 + 1))
    assert infos[-1].staged == 10 and infos[-1].evicted.size == 0 and infos[-1].sets[0]["cand"].size == 0
    assert infos[-1].H.size == 64
    again = np.concatenate([np.setdiff1d(first, cached), ten])
    assert again.size == 46
    infos.append(case.train_step(again, it0 + 2))
    assert infos[-1].H.size == 0 and infos[-1].evicted.size == 46 and infos[-1].staged == 0
    infos.append(case.train_step(np.concatenate([case.model.tags, np.setdiff1d(cached, case.model.tags)[:5]]), it0 + 3, update=False))
    assert infos[-1].staged == 5 and infos[-1].H.size == 64
    case.finish()
    return infos


def seq_random(case, seed, steps=12):
    rng = np.random.default_rng([seed, case.g.num_sets, case.g.Tc])
    domain = case.pool[:min(case.pool.size, 3 * case.g.slots + 50)]
    infos, it = [], 0
    for step in range(steps):
        n = int(rng.integers(1, 301))
        keys = domain[(rng.random(n) ** 2 * domain.size).astype(np.int64)]  # skewed: hits, duplicates
        it += int(rng.integers(1, 4))
        infos.append(case.train_step(keys, it, update=step % 4 != 3, B=int(rng.integers(1, 4))))
        if step % 4 == 3 and step % 8 == 3:
            case.writeback_staging()  # after a forward-only step: rewrites unchanged rows
    case.finish()
    return infos


def seq_conflicts(case):
    """num_sets = 3: set A receives 70 keys (64 ways + 6 staged) while set B receives 10 and set C none."""
    g = case.g
    assert g.num_sets == 3
    s = set_of(case.pool, 3)
    a, b = case.pool[s == 0], case.pool[s == 1]
    infos = [case.train_step(np.concatenate([a[:70], b[:10]]), 1)]
    assert infos[0].sets[0]["staged"] == 6 and infos[0].sets[1]["staged"] == 0 and infos[0].staged == 6
    tags = case.model.tags
    assert (tags[:64] >= 0).all() and (tags[64:128] >= 0).sum() == 10 and (tags[128:] == -1).all()
    # all of set A hit, four more misses there (staged although B and C have spare ways), twenty into B
    infos.append(case.train_step(np.concatenate([tags[:64], a[70:74], b[10:30]]), 2))
    assert infos[1].sets[0]["staged"] == 4 and infos[1].staged == 4 and infos[1].evicted.size == 0
    tags = case.model.tags
    assert (tags[64:128] >= 0).sum() == 30 and (tags[128:] == -1).all()
    case.finish()
    return infos


DUP_GEOMETRY = dict(tab_rows=[200, 30], tab_D=8, feat_ctab=[0, 1, 0], feat_rows=[200, 30, 200], state=True)


def seq_duplicates(case):
    """Features 0 and 2 share table 0; one key occurs 50 times across both."""
    hot = 17
    per = [[hot] * 27 + [3, 4, 5, 3], [1, 2, 1], [hot] * 23 + [5, 6, 199]]
    indices, offsets = case.batch(per, B=4)
    info = case.prefetch(indices, offsets, 1)
    assert info.U.size == 6 + 2 and int(case.snap.counters[4]) == 8
    hot_slots = np.unique(info.remapped[(info.pos_keys == hot)])
    assert (info.pos_keys == hot).sum() == 50 and hot_slots.size == 1
    case.update(1)
    case.writeback_staging()
    info2 = case.prefetch(indices, offsets, 2)
    assert info2.H.size == 8 and info2.M.size == 0
    case.update(2)
    case.writeback_staging()
    case.finish()
    return [info, info2]


MIXED_GEOMETRY = dict(
    tab_rows=[300, 50, 200], tab_D=8, state=True, feat_ctab=[0, -1, 1, 2, 0], feat_rows=[300, 50, 50, 200, 300],
    feat_window=[(0, 300), (0, 50), (0, 50), (100, 1000), (0, 300)])


def seq_mixed(case):
    """An uncached feature between cached ones (ids pass unchanged, negative and out-of-range ones included), an empty
    feature, a cached feature whose window [100, 300) of 1000 global rows gets local, foreign, bad and TBE_ID_SKIP ids."""
    S = TBE_ID_SKIP
    per = [
        list(range(0, 40, 2)) + [300, -1, S, 299],
        [3, -1, 49, 50, 10 ** 12, -(2 ** 40), 0],
        list(range(10)),
        [100, 299, 150, 0, 99, 300, 999, 1000, -3, 2 ** 40, S, 150, 101],
        [0, 2, 298, 7],
    ]
    indices, offsets = case.batch(per, B=3)
    info = case.prefetch(indices, offsets, 1)
    assert np.bincount(info.cls, minlength=4).tolist() == [40, 6, 5, 7]  # local, foreign, bad, uncached
    case.update(1)
    case.writeback_staging()
    per2 = [[1, 299, 0], [], [], [S, 100, 250, 5, 1001], [298, 11]]  # features 1 and 2 are empty
    indices, offsets = case.batch(per2, B=3)
    info2 = case.prefetch(indices, offsets, 2)
    assert info2.H.size > 0 and info2.M.size > 0
    case.update(2)
    case.writeback_staging()
    case.finish()
    return [info, info2]


def seq_empty(case):
    """N == 0 after a warm step: counters 0, 4, 5 reset, the totals and every other byte unchanged."""
    info = case.train_step(case.take(30), 1)
    assert int(case.snap.counters[4]) == 30
    empty = case.prefetch(np.zeros(0, dtype=np.int64), np.zeros(case.g.F * 2 + 1, dtype=np.int64), 2)
    c = case.snap.counters
    assert c[0] == 0 and c[4] == 0 and c[5] == 0 and c[2] == 30
    case.finish()
    return [info, empty]


def seq_many_tables(case):
    """70 cached tables: hits and misses in tables 0, 63, 64 and 69 (both ballot trips of table_of, first and last lane)."""
    g = case.g
    tabs = [0, 63, 64, 69, 5, 33]
    row0 = np.array([int(g.key_base[t]) for t in tabs], dtype=np.int64)
    a = case.train_step(row0, 1)
    assert a.M.size == len(tabs)
    b = case.train_step(np.concatenate([row0, row0 + 1]), 2)
    assert b.H.size == len(tabs) and b.M.size == len(tabs)
    fill = np.setdiff1d(case.pool, np.concatenate([row0, row0 + 1]))[:64]
    c = case.train_step(fill, 3)  # evicts all twelve
    assert set(np.concatenate([row0, row0 + 1]).tolist()) <= set(c.evicted.tolist())
    d = case.train_step(np.concatenate([row0, row0 + 1]), 4)  # they come back from the host, updated
    assert d.M.size == 2 * len(tabs)
    case.finish()
    return [a, b, c, d]
