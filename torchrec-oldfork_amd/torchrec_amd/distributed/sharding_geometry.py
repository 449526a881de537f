"""Who holds what in a ShardedEmbeddingBagCollection, for ALL ranks at once: plain lists and ints computed from the table
configs and the plan alone — no tensor, no device, no process group — so that what rank s packs for rank r can be checked
against what r unpacks without spawning a world (tests/test_sharding_geometry.py).  embeddingbag.py turns the few lists
the kernels read into tensors and builds the lookups."""
import itertools
from typing import Dict, List, Optional, Tuple

from ..modules.embedding_configs import EmbeddingBagConfig, pooling_type_to_pooling_mode
from .planner import rw_block_size, rw_shard_rows
from .types import ParameterSharding, ShardingType


class _LocalTable:
    """One table of a rank's fused lookup: a whole table (table-wise), a row block (row-wise) or ONE column shard of a
    column-wise table (`column_shard` = (shard number in column order, shards of the table); columns
    [col_offset, col_offset + cols) of every row)."""

    def __init__(self, cfg: EmbeddingBagConfig, local_rows: int, row_offset: int, row_wise: bool,
                 compute_kernel: str = "batched_fused", col_offset: int = 0, cols: Optional[int] = None,
                 column_shard: Optional[Tuple[int, int]] = None) -> None:
        self.cfg, self.local_rows, self.row_offset, self.row_wise = cfg, local_rows, row_offset, row_wise
        self.compute_kernel = compute_kernel
        self.col_offset, self.cols = col_offset, (cfg.embedding_dim if cols is None else cols)
        self.column_shard = column_shard


def _column_shards(name: str, cfg: EmbeddingBagConfig, ps: ParameterSharding, W: int) -> List[Tuple[int, int, int]]:
    """[(first column, width, rank)] of a column-wise table in column order, validated: the shards tile [0, D) without
    gaps or overlap, every shard has all rows, every rank exists.  ValueError names the table otherwise."""
    spec, ranks = ps.sharding_spec, ps.ranks
    if not spec or ranks is None or len(ranks) != len(spec):
        raise ValueError(f"table {name}: a column-wise plan needs one rank per shard of its sharding_spec "
                         f"({0 if ranks is None else len(ranks)} ranks, {len(spec or [])} shards)")
    shards = []
    for sm, r in zip(spec, ranks):
        if list(sm.shard_offsets)[0] != 0 or list(sm.shard_sizes)[0] != cfg.num_embeddings:
            raise ValueError(f"table {name}: column shard at {list(sm.shard_offsets)} of size {list(sm.shard_sizes)} does not "
                             f"hold all {cfg.num_embeddings} rows")
        if not 0 <= int(r) < W:
            raise ValueError(f"table {name}: column shard at column {sm.shard_offsets[1]} is placed on rank {r}, "
                             f"outside the world of {W}")
        shards.append((int(sm.shard_offsets[1]), int(sm.shard_sizes[1]), int(r)))
    shards.sort(key=lambda x: x[0])
    col = 0
    for c, w, _ in shards:
        if c != col or w <= 0:
            raise ValueError(f"table {name}: column shards {[(c, w) for c, w, _ in shards]} do not tile [0, {cfg.embedding_dim}) "
                             f"(gap or overlap at column {col})")
        col += w
    if col != cfg.embedding_dim:
        raise ValueError(f"table {name}: column shards {[(c, w) for c, w, _ in shards]} do not tile [0, {cfg.embedding_dim})")
    return shards


class ShardingGeometry:
    """What sharding_geometry() returns; every list is the same on every rank.  Per FEATURE (the collection's output
    order): feature_names, feature_table, feature_dim, out_col (+ D_total), dp_feats / sharded_feats / rw_feats (feature
    numbers).  Per TABLE: table_kind (-3 column-wise, -2 replicated, -1 row-wise, else owning rank), cw_shards.  Per PIECE
    (feature, column shard): piece_feat / _col / _dim / _kind / _shard, piece_out_col, feat_src, feat_slab_col.  Per RANK:
    local_pieces, D_local_per_rank, send_feats_per_rank, tw_per_rank (+ its prefix sums tw_first); send_feature_order and
    tw_send_order concatenate the ranks' lists; local_tables(rank) has the rank's lookup."""

    def local_tables(self, rank: int) -> Tuple[List[_LocalTable], List[int]]:
        """(tables of rank's fused lookup, table of each of its local pieces): one table per table-wise table, row block
        or column shard held."""
        W, tables = self.world_size, []
        index: Dict[Tuple[int, int], int] = {}  # (table, column shard) -> local TBE table
        for p in self.local_pieces[rank]:
            t = self.feature_table[self.piece_feat[p]]
            if (t, self.piece_shard[p]) in index:
                continue
            c, ck = self.cfgs[t], self.compute_kernels[t]
            if self.table_kind[t] == -1:
                tables.append(_LocalTable(c, rw_shard_rows(c.num_embeddings, W)[rank], rank * rw_block_size(c.num_embeddings, W),
                                          True, ck))
            elif self.table_kind[t] == -3:  # each local column shard is its own TBE table [rows, width]
                tables.append(_LocalTable(c, c.num_embeddings, 0, False, ck, self.piece_col[p], self.piece_dim[p],
                                          (self.piece_shard[p], len(self.cw_shards[t]))))
            else:
                tables.append(_LocalTable(c, c.num_embeddings, 0, False, ck))
            index[(t, self.piece_shard[p])] = len(tables) - 1
        return tables, [index[(self.feature_table[self.piece_feat[p]], self.piece_shard[p])] for p in self.local_pieces[rank]]


def sharding_geometry(cfgs: List[EmbeddingBagConfig], table_name_to_parameter_sharding: Dict[str, ParameterSharding], W: int,
                      variable_batch: bool = False, rw_input_dist: str = "auto",
                      optimizer_name: Optional[str] = None) -> ShardingGeometry:
    """The layout of a collection over W ranks; raises for the combinations the collection refuses."""
    g = ShardingGeometry()
    g.world_size, g.cfgs = W, list(cfgs)
    g.compute_kernels = [table_name_to_parameter_sharding[c.name].compute_kernel for c in cfgs]
    # ---- global feature list, in the collection's output order -----------------------------
    g.feature_names, g_table = [], []
    for t, c in enumerate(cfgs):
        for f in c.feature_names:
            g.feature_names.append(f)
            g_table.append(t)
    Fg = len(g.feature_names)
    g.feature_table = g_table
    g_dim = g.feature_dim = [cfgs[t].embedding_dim for t in g_table]
    g.D_total = sum(g_dim)
    # ---- who holds what --------------------------------------------------------------------
    kind: List[int] = []  # per table: -3 column-wise, -2 replicated, -1 row-wise, else owning rank
    cw_shards: Dict[int, List[Tuple[int, int, int]]] = {}  # column-wise table -> [(first column, width, rank)]
    for t, c in enumerate(cfgs):
        ps = table_name_to_parameter_sharding[c.name]
        if ps.sharding_type == ShardingType.DATA_PARALLEL.value:
            kind.append(-2)
        elif ps.sharding_type == ShardingType.ROW_WISE.value:
            if variable_batch:
                raise NotImplementedError(
                    f"table {c.name}: row_wise sharding in a variable_batch_size collection (the reference has no "
                    "variable-batch row-wise sharding either); shard it table-wise or column-wise, or replicate it")
            kind.append(-1)
        elif ps.sharding_type == ShardingType.TABLE_WISE.value:
            kind.append(int(ps.ranks[0]))
        elif ps.sharding_type in (ShardingType.COLUMN_WISE.value, ShardingType.TABLE_COLUMN_WISE.value):
            # (one node, no host hierarchy: the two types are the same thing here)
            kind.append(-3)
            cw_shards[t] = _column_shards(c.name, c, ps, W)
            if (ps.compute_kernel == "batched_fused_uvm_caching" and len({w for _, w, _ in cw_shards[t]}) > 1):
                raise NotImplementedError(
                    f"table {c.name}: column shards of different widths {[w for _, w, _ in cw_shards[t]]} behind the HBM row "
                    "cache (batched_fused_uvm_caching): the cache holds rows of ONE width; choose a min_partition that "
                    "divides the embedding dim, or another compute kernel")
        else:
            raise NotImplementedError(f"sharding type {ps.sharding_type} is outside the MI355X hot path "
                                      "(table_wise / row_wise / column_wise / data_parallel)")
    g.table_kind, g.cw_shards = kind, cw_shards
    # LAMB, PARTIAL_ROWWISE_LAMB and LARS_SGD scale a row's step by norms over the WHOLE row, PARTIAL_ROWWISE_ADAM keeps
    # one second moment per row: a column shard sees only its columns, so the result would depend on the sharding
    # (table-wise and row-wise shards hold whole rows and are invariant).  Gradient clipping is element-wise: allowed.
    if cw_shards and optimizer_name in ("LAMB", "PARTIAL_ROWWISE_ADAM", "PARTIAL_ROWWISE_LAMB", "LARS_SGD"):
        raise NotImplementedError(
            f"column-wise table(s) {[cfgs[t].name for t in cw_shards]} with optimizer {optimizer_name}: its row norms / row-wise "
            "state are taken over a whole row, which a column shard does not hold; shard these tables table-wise or "
            "row-wise, or use an element-wise optimizer")
    if cw_shards and rw_input_dist == "bucketize":
        raise NotImplementedError(
            "rw_input_dist='bucketize' with column-wise tables "
            f"({[cfgs[t].name for t in cw_shards]}): the bucketized input dist is not built for column shards; use "
            "'windows' (or 'auto', which does) for such collections")
    # ---- pieces: the unit of everything below.  A piece is (feature, column shard); tables that are not column-wise
    #      have ONE piece per feature, so piece number == feature number for them and every list is what it was -------
    p_feat: List[int] = []   # feature of the piece
    p_col: List[int] = []    # first column of the piece inside its feature
    p_dim: List[int] = []    # width
    p_kind: List[int] = []   # -2 replicated, -1 row-wise, else owning rank
    p_shard: List[int] = []  # column shard number (0 for whole-width pieces)
    for f in range(Fg):
        t = g_table[f]
        for i, (c0, w, r) in enumerate(cw_shards[t] if kind[t] == -3 else [(0, g_dim[f], kind[t])]):
            p_feat.append(f)
            p_col.append(c0)
            p_dim.append(w)
            p_kind.append(r)
            p_shard.append(i)
    P = len(p_feat)
    g.piece_feat, g.piece_col, g.piece_dim, g.piece_kind, g.piece_shard = p_feat, p_col, p_dim, p_kind, p_shard
    # local piece list of every rank: row-wise features first (same columns on every rank).  The ids of a feature
    # travel to every rank that holds one of its pieces — twice to a rank that holds two (the reference duplicates the
    # feature per shard too: sharding/cw_sharding.py _id_list_features_per_rank)
    rw_pieces = [p for p in range(P) if p_kind[p] == -1]
    g.dp_feats = [f for f in range(Fg) if kind[g_table[f]] == -2]
    g.sharded_feats = [f for f in range(Fg) if kind[g_table[f]] != -2]
    local = g.local_pieces = [rw_pieces + [p for p in range(P) if p_kind[p] == r] for r in range(W)]
    g.D_local_per_rank = [sum(p_dim[p] for p in lf) for lf in local]
    g.send_feature_order = [p_feat[p] for lf in local for p in lf]
    g.send_feats_per_rank = [len(lf) for lf in local]
    # bucketized row-wise input dist: row-wise features (bucketized, one block per destination) and the table-wise
    # features in destination order travel as separate pieces of one exchange
    g.rw_feats = [p_feat[p] for p in rw_pieces]
    g.tw_send_order = [p_feat[p] for r in range(W) for p in local[r] if p_kind[p] != -1]
    g.tw_per_rank = [sum(1 for p in local[r] if p_kind[p] != -1) for r in range(W)]
    g.tw_first = [0] + list(itertools.accumulate(g.tw_per_rank))  # first table-wise feature of each destination
    g.rw_block_sizes = [rw_block_size(cfgs[g_table[f]].num_embeddings, W) for f in g.rw_feats]
    g.rw_mean = any(pooling_type_to_pooling_mode(cfgs[g_table[f]].pooling) == 1 for f in g.rw_feats)
    if g.rw_mean and rw_input_dist == "bucketize":
        raise NotImplementedError(
            "rw_input_dist='bucketize' with MEAN-pooled row-wise tables: a rank would divide its partial sum by the number "
            "of ids in ITS row block, not by the bag length; use 'windows' (or 'auto', which does) for such collections")
    # exchange descriptors (batch-independent part), one entry per piece: the kernels (csrc/pooled_exchange.hip) copy
    # column ranges and do not care whether a range is a whole feature
    g.feat_src, g.feat_slab_col = [0] * P, [0] * P
    for r in range(W):
        col = 0
        for p in local[r]:
            if p_kind[p] == -1:
                g.feat_src[p], g.feat_slab_col[p] = -1, col
            elif p_kind[p] == r:
                g.feat_src[p], g.feat_slab_col[p] = r, col
            col += p_dim[p]
    for p in range(P):
        if p_kind[p] == -2:
            g.feat_src[p] = -2
    g.out_col = [0]
    for d in g_dim:
        g.out_col.append(g.out_col[-1] + d)
    # the pieces of a feature are consecutive in the output matrix: out_col(piece) = out_col(feature) + first column
    g.piece_out_col = [g.out_col[p_feat[p]] + p_col[p] for p in range(P)]
    g.vec_ok = all(d % 4 == 0 for d in p_dim)
    return g
