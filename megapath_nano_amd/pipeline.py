"""Integer-coded fast path of the reference's step 3 (`step_placement_to_species`,
/root/reference/bin/megapath_nano.py:1253-1310): Align (:1262) -> Reassign (:1281) -> best alignment per read
(:1287) -> aligned bp per species (:1289) -> reads per name (:3664-3667), without going through DataFrames.
The DataFrame-level mirrors (aligner.Align, reassignment.Reassign) call the same C-ABI entry points; this module is
what bench.py times and what a multi-GPU run executes per rank.
"""
import pickle
import random
import time

import numpy as np

from . import dist as mdist
from . import mapper
from .reassignment import ReassignPlan


def random_block(rnd, n):
    """The next n values of `rnd.random()` (a random.Random, or the random module) as a float64 array, leaving `rnd` where
    n calls would have left it.  Python's generator and numpy's RandomState are the same MT19937 with the same 53-bit
    double construction, so the state is lent to numpy for the block instead of making n Python-level calls."""
    ver, st, gauss = rnd.getstate()
    rs = np.random.RandomState()
    rs.set_state(('MT19937', np.array(st[:-1], dtype=np.uint32), int(st[-1])))
    out = rs.random_sample(int(n))
    _, key, pos = rs.get_state()[:3]
    rnd.setstate((ver, tuple(int(x) for x in key) + (int(pos),), gauss))
    return out


def sharded_tiebreak(rnd, n_rows, shard, allreduce):
    """Tiebreakers for this rank's rows such that the concatenation over ranks equals ONE `random.random()` stream drawn
    in global row order (the reference draws them row by row over the whole table, aligner.py:334-335).  Every rank
    seeds `rnd` identically; ranks hold contiguous read ranges in rank order; the row counts are exchanged as one small
    all-reduce, the draws of the ranks before this one are skipped and those of the ranks after it consumed, so that
    the generator is in the same state on every rank afterwards.  shard = (rank, world)."""
    rank, world = shard
    if world <= 1 or allreduce is None:
        return random_block(rnd, n_rows)
    counts = np.zeros(world, dtype=np.int64)
    counts[rank] = n_rows
    allreduce(counts)
    before, after = int(counts[:rank].sum()), int(counts[rank + 1:].sum())
    random_block(rnd, before)
    out = random_block(rnd, n_rows)
    random_block(rnd, after)
    return out


class Taxonomy:
    """Per target sequence: dense species-name code (reassignment.py:69-71) and dense species_tax_id code."""

    def __init__(self, name_code, n_names, species_code, n_species):
        self.name_code = np.asarray(name_code, dtype=np.int32)
        self.species_code = np.asarray(species_code, dtype=np.int32)
        self.n_names, self.n_species = int(n_names), int(n_species)


class ShardedIndex:
    """This rank's share of a target set whose index parts are sharded over the ranks of each read group.

    World W = R x S; rank r is shard s = r % S of read group g = r // S and holds the parts of block s of
    dist.assign_parts (contiguous, in target order).  Every rank of a group maps the group's whole batch against its own parts;
    the hits of owner sub-range t go to shard t of the group (mpn_hits_export, dist.exchange_bytes), which imports the blocks
    in shard order and merges them (mpn_hits_import, mpn_hits_finish).  Because the blocks are contiguous and imported in
    shard order, the merged accumulator is the one a single process holding every part would have built: same part order,
    same target ids, the largest rep_len.  The per-shard target lists and part counts are gathered once, here."""

    def __init__(self, parts, rank, world, n_shards, groups=None):
        """parts: this rank's resident mapper.Index parts, in target order.  groups: dist.shard_groups(world, n_shards), created
        by every rank (a collective); made here when not given."""
        self.group_id, self.shard = mdist.index_shard_layout(rank, world, n_shards)
        self.rank, self.world, self.n_shards = rank, world, n_shards
        self.parts = list(parts)
        if groups is None:
            groups = mdist.shard_groups(world, n_shards)
        self.group = groups[self.group_id]
        mine = ([n for p in self.parts for n in p.names], [int(x) for p in self.parts for x in p.lens], len(self.parts))
        if n_shards == 1:
            got = [mine]
        else:
            blob = np.frombuffer(pickle.dumps(mine), dtype=np.uint8)
            got = [pickle.loads(b.tobytes()) for b in mdist.exchange_bytes([blob] * n_shards, self.group)]
        self.targets = [(names, np.asarray(lens, dtype=np.int32)) for names, lens, _ in got]
        self.n_parts = [int(k) for _, _, k in got]
        self.times = {}

    def all_targets(self):
        """(names, lens) of the whole target set: the shards' lists in shard order, = the single-process target order"""
        return [n for names, _ in self.targets for n in names], np.concatenate([lens for _, lens in self.targets])

    def owner_ranges(self, lens):
        """The S owner sub-ranges of a group batch with read lengths `lens` (batch indices)."""
        return mdist.shard_bounds(lens, self.n_shards)

    def map_owned(self, opt, packed, use_device=True):
        """packed: the whole batch of this rank's read group (the same on every shard of the group).  -> the finished columns of
        the reads this rank owns (sub-range `shard` of the batch), read_idx relative to the sub-range.  Every rank takes part
        in the exchange, also with an empty sub-range.  self.times: seconds of map / export / exchange / import / finish, and
        the bytes this rank sent."""
        t = {}
        t0 = time.perf_counter()
        subs = self.owner_ranges(packed.lens)
        hits = mapper.Hits(packed, want_text=False)
        try:
            hits.add_parts(self.parts, opt, use_device=use_device)
            t1 = time.perf_counter()
            blocks = [hits.export(lo, hi) for lo, hi in subs]
        finally:
            hits.close()
        t2 = time.perf_counter()
        got = blocks if self.n_shards == 1 else mdist.exchange_bytes(blocks, self.group)
        t3 = time.perf_counter()
        lo, hi = subs[self.shard]
        acc = mapper.Hits(packed.sub(lo, hi), want_text=False)
        try:
            for s, blk in enumerate(got):
                acc.import_block(blk, self.n_parts[s], *self.targets[s])
            t4 = time.perf_counter()
            _, _, c = acc.finish(opt, want_paf=False, want_cols=True)
        finally:
            acc.close()
        t5 = time.perf_counter()
        self.times = dict(map_s=t1 - t0, export_s=t2 - t1, exchange_s=t3 - t2, import_s=t4 - t3, finish_s=t5 - t4,
                          sent_bytes=sum(len(b) for s, b in enumerate(blocks) if s != self.shard), owned=(lo, hi))
        return c

    def close(self):
        for p in self.parts:
            p.close()
        self.parts = []


def own_saved_parts(path, rank, world, n_shards):
    """The parts of a saved multi-part index (Index.save(append=True), minimap2 -d) that shard `rank` holds: every part is
    placed from its header alone (Index.part_info), only this shard's block is loaded.  -> list of mapper.Index"""
    info = mapper.Index.part_info(path)
    _, shard = mdist.index_shard_layout(rank, world, n_shards)
    a, b = mdist.assign_parts([bases for _, _, bases in info], n_shards)[shard]
    return [mapper.Index.load_at(path, info[p][0])[0] for p in range(a, b)]


def own_target_parts(make_parts, rank, world, n_shards, k=15, w=10):
    """The parts cut from a target stream (aligner.iter_target_parts) that shard `rank` holds.  make_parts() starts the stream
    anew: a first pass only counts the bases of every part, the second builds this shard's block and skips the rest.
    -> list of mapper.Index"""
    bases = [sum(len(s) for _, s in part) for part in make_parts()]
    _, shard = mdist.index_shard_layout(rank, world, n_shards)
    a, b = mdist.assign_parts(bases, n_shards)[shard]
    out = []
    for p, part in enumerate(make_parts()):
        if a <= p < b:
            out.append(mapper.Index(part, k=k, w=w))
        elif p >= b:
            break
    return out


def align_and_assign(idx, opt, packed, tax, error_rate=0.05, ratio=0.05, as_threshold=0.0, min_alignment_score=0,
                     allreduce=None, rng=None, reassign=True, shard=(0, 1), use_device=True):
    """One step of the hot path for one batch of reads.  Returns dict(read_count, aligned_bp, n_rows, n_relations).
    With shard=(rank, world) and an all-reduce, `rng` must be seeded identically on every rank (see sharded_tiebreak).
    idx: one Index, a list of resident parts, or a ShardedIndex; with the latter, `packed` is the whole batch of this rank's
    read group and the rows that follow are those of the reads this rank owns."""
    if isinstance(idx, ShardedIndex):
        c = idx.map_owned(opt, packed, use_device=use_device)   # columns of this rank's owned reads, merged over every shard
    elif isinstance(idx, (list, tuple)):
        # a target set held as several index parts (minimap2 -I): every part is mapped, the hits are merged per read like
        # minimap2 --split-prefix merges them (mapper.Hits); column `rid` indexes the concatenated target list
        hits = mapper.Hits(packed, want_text=False)
        try:
            hits.add_parts(list(idx), opt, use_device=use_device)      # all parts are resident: one call, one pipeline
            _, _, c = hits.finish(opt, want_paf=False, want_cols=True)
        finally:
            hits.close()
    else:
        _, c = mapper.map_batch_ex(idx, opt, packed, want_paf=False, want_cols=True, use_device=use_device)
    keep = c['as_'] >= min_alignment_score                                   # aligner.py:311-312
    read_idx = c['read_idx'][keep]
    rid = c['rid'][keep]
    score = c['as_'][keep]
    aligned_bp = (c['re'][keep] - c['rs'][keep]).astype(np.int64)
    n_rows = len(read_idx)
    tiebreak = sharded_tiebreak(rng if rng is not None else random, n_rows, shard, allreduce)  # aligner.py:334-335
    read_count = np.zeros(tax.n_names, dtype=np.int64)
    bp = np.zeros(tax.n_species, dtype=np.int64)
    nrel = 0
    if n_rows:
        plan = ReassignPlan(read_idx, tax.name_code[rid], score, tiebreak, aligned_bp, tax.species_code[rid], tax.n_names,
                            tax.n_species)
        try:
            all_count, u_count, n_multi = plan.counts()
            if allreduce is not None:
                allreduce(all_count), allreduce(u_count), allreduce(n_multi)
            rank = np.arange(tax.n_names, dtype=np.int32)
            if not reassign:  # --no-reassignment: an empty relation leaves every name untouched
                error_rate = -1.0
            _, _, _, read_count, bp, nrel = plan.apply(all_count, u_count, rank, error_rate, ratio, as_threshold)
        finally:
            plan.close()
    elif allreduce is not None:
        z = np.zeros(tax.n_names, dtype=np.int64)
        allreduce(z), allreduce(z.copy()), allreduce(np.zeros(1, dtype=np.int64))
    if allreduce is not None:
        allreduce(read_count), allreduce(bp)                                 # the taxon-count all-reduce
    return dict(read_count=read_count, aligned_bp=bp, n_rows=n_rows, n_relations=nrel)
