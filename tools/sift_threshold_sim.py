#!/usr/bin/env python3
"""tools/sift_threshold_sim.py [CONFIG ...] — what tier 0's sift lets through, counted on the host (no GPU).

Replays k_join_part's cycle packing (pdl_join_part.h) from the CPU oracle's dictionary: rows in task order, drawn eight at a
time; a cycle of the first form takes up to 4 consecutive rows, <= 960 ranges and <= 4096 walked lookups (the postings behind
the row's own record in every rank group: the upper triangle); a row that alone exceeds 4096 lookups is a cycle of its own in the
second form (<= 8192).  For every cycle the lookups that survive the sift, and the table slots they touch, are counted for

  (a) two 32-Kbit bitmaps, "seen" / "seen twice" on the top 15 bits of h(column)      (the sift before the counters)
  (b) 4096 counters on the top 12 bits of h, threshold T = clamp(min(tc_min, min pc_min of the cycle's rows), 2, 255);
      a lookup with a count >= 2 on either side adds T
  (c) the same counters with T = 2
  (x) no collisions at all: the lookups of (row, column) pairs with at least T sightings — the floor for (b)

Not replayed: the retry of a cycle whose rows overflow their part of the table (the touched slots per cycle say how near that is:
a row's part takes 768 / rows of the cycle), and the reference's fold of the globally last record into the group before it.
Default configs: the bench set, 16x1000x300, and the bench set plus one short gene that brings the threshold down to 2, 3, 4, 5.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PT_RB, PT_ROWS, PT_BATCH, PT_HEAVY_CAP = 960, 4, 8, 64
LMAX1, LMAX2 = 4096, 8192
HASH_MUL = 0x9E3779B1 & 0x3FFFFF
BENCH_SET = "mycoplasma64_standin"
EXTRA_SETS = {"synthetic_16x1000x300": dict(genomes=16, genes_per_genome=1000, mean_len=300, sub_rate=0.08, seed=7)}      # (tests/golden: synth_16x1000x300_k5)


def min_numerator(threshold: np.float32, denom: int) -> int:
    """pdl_join.hip's min_numerator, in float32 as on the device"""
    d = np.float32(denom)
    n = int(np.float32(threshold * d))
    n = n - 2 if n > 2 else 0
    while np.float32(n) / d < threshold:
        n += 1
    return n


def simulate(name: str, gs, k: int) -> dict:
    from oracle import binding as ob
    t0 = time.time()
    ora = ob.Oracle(gs.residues, gs.offsets, gs.genome_of, k)
    D = ora.dictionary()
    kseq = ora.kseq_lengths().astype(np.int64)
    ora.close()
    D = D[np.lexsort((D["seq"], D["rank"]))]                          # (rank, gene) order; the reference leaves its very last record out of place
    rank, seq, cnt = D["rank"], D["seq"].astype(np.int64), D["count"].astype(np.int64)
    n = len(D)
    new_group = np.concatenate([[True], rank[1:] != rank[:-1]])
    gstart = np.nonzero(new_group)[0]
    gend = np.repeat(np.concatenate([gstart[1:], [n]]), np.diff(np.concatenate([gstart, [n]])))
    after = gend - np.arange(n) - 1                                   # postings behind the record in its group
    order = np.argsort(seq, kind="stable")                            # a row's records, in rank order
    order = order[after[order] > 0]                                   # (a range without a posting is not listed)
    N = len(kseq)
    row_off = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(seq[order], minlength=N), out=row_off[1:])
    row_ranges = np.diff(row_off)
    row_look = np.zeros(N, np.int64)
    np.add.at(row_look, seq[order], after[order])
    threshold = np.float32(1.0) / np.float32(2.0 * k)
    min_kseq = int(kseq.min())
    assert min_kseq > 2 * k, "tier 0 is not selected on a set with a gene of <= 2k k-mers"
    tc_min = min_numerator(threshold, min_kseq)
    pc_cache: dict = {}

    def pc_min(r):
        v = int(kseq[r])
        if v not in pc_cache:
            pc_cache[v] = min_numerator(threshold, v)
        return pc_cache[v]

    tot = {f: {"cycles": 0, "rows": 0, "lookups": 0, "heavy": 0, "void": 0, "t_sum": 0,
               "surv": {c: 0 for c in "abcx"}, "slots": {c: 0 for c in "abcx"}} for f in ("first", "second")}
    handed_on = 0

    def cycle(form, r0, r1):
        rec = order[row_off[r0]:row_off[r1]]
        lens = after[rec]
        total = int(lens.sum())
        excl = np.cumsum(lens) - lens
        idx = np.repeat(rec + 1 - excl, lens) + np.arange(total)
        col = seq[idx]
        heavy = (cnt[idx] >= 2) | np.repeat(cnt[rec] >= 2, lens)
        slot = np.repeat(seq[rec] - r0, lens)
        h = (col * HASH_MUL) & 0x3FFFFF
        T = max(2, min(255, min(tc_min, min(pc_min(r) for r in range(r0, r1)))))
        s = tot[form]
        s["cycles"] += 1; s["rows"] += r1 - r0; s["lookups"] += total; s["heavy"] += int(heavy.sum()); s["t_sum"] += T
        if int(heavy.sum()) > PT_HEAVY_CAP:
            s["void"] += 1
        pair = (slot << 22) | col
        keep = {}
        b15 = h >> 7
        keep["a"] = np.bincount(b15, weights=1 + heavy, minlength=1 << 15)[b15] >= 2
        b12 = h >> 10
        for c, t in (("b", T), ("c", 2)):
            keep[c] = np.bincount(b12, weights=np.where(heavy, t, 1), minlength=1 << 12)[b12] >= t
        u, inv = np.unique(pair, return_inverse=True)
        keep["x"] = np.bincount(inv, weights=np.where(heavy, T, 1))[inv] >= T
        for c, kp in keep.items():
            s["surv"][c] += int(kp.sum())
            s["slots"][c] += len(np.unique(pair[kp]))

    second = []
    for w0 in range(0, N, PT_BATCH):
        bn = min(PT_BATCH, N - w0)
        j = 0
        while j < bn:
            r = w0 + j
            if row_ranges[r] == 0:
                j += 1; continue
            if row_ranges[r] > PT_RB or kseq[r] <= 2 * k:
                handed_on += 1; j += 1; continue
            ns, nb, jj = 0, 0, j                                      # consecutive ordinary rows while their ranges fit
            while ns < PT_ROWS and jj < bn:
                q = w0 + jj
                if row_ranges[q] == 0 or row_ranges[q] > PT_RB or kseq[q] <= 2 * k or nb + row_ranges[q] > PT_RB:
                    break
                nb += row_ranges[q]; ns += 1; jj += 1
            keep_rows, look = 0, 0
            for s_ in range(ns):                                      # the leading rows whose lookups fit the cycle together
                look += row_look[r + s_]
                if look <= LMAX1:
                    keep_rows = s_ + 1
            if keep_rows == 0:
                second.append(r); j += 1; continue
            cycle("first", r, r + keep_rows)
            j += keep_rows
    for r in second:
        if row_look[r] > LMAX2:
            handed_on += 1
        else:
            cycle("second", r, r + 1)

    out = {"config": name, "k": k, "genes": int(N), "min_kseq": min_kseq, "tc_min": tc_min, "handed_to_tier1": handed_on,
           "seconds": round(time.time() - t0, 1), "forms": {}}
    for f, s in tot.items():
        cy, lk = max(s["cycles"], 1), max(s["lookups"], 1)
        out["forms"][f] = {"cycles": s["cycles"], "rows_per_cycle": round(s["rows"] / cy, 3), "lookups_per_cycle": round(s["lookups"] / cy, 1),
                           "lookups": s["lookups"], "heavy_lookups": s["heavy"], "cycles_over_heavy_cap": s["void"], "mean_T": round(s["t_sum"] / cy, 2),
                           "survivor_share": {c: round(s["surv"][c] / lk, 4) for c in "abcx"},
                           "touched_slots_per_cycle": {c: round(s["slots"][c] / cy, 1) for c in "abcx"}}
    return out


def with_short_gene(gs, kmers: int, k: int):
    """the set plus ONE unrelated gene of `kmers` k-mers at its end: nothing changes but min_kseq, and with it tc_min and the threshold"""
    from pandelos_amd.synth import ALPHABET, GeneSet
    rng = np.random.Generator(np.random.PCG64(kmers))
    gene = ALPHABET[rng.integers(0, 20, kmers + k - 1)]
    return GeneSet(np.concatenate([gs.residues, gene]), np.concatenate([gs.offsets, [gs.offsets[-1] + np.uint64(len(gene))]]).astype(np.uint64),
                   np.concatenate([gs.genome_of, gs.genome_of[-1:]]), np.concatenate([gs.family_of, [-1]]))


def main(argv):
    """CONFIG or CONFIG+N (the config plus one gene of N k-mers: a set whose threshold is low by nature, 2 for N in (2k, 4k])"""
    from pandelos_amd.calculate_k import calculate_k
    from pandelos_amd.synth import CONFIGS, make_gene_set
    for name in argv or [BENCH_SET, "synthetic_16x1000x300", BENCH_SET + "+11", BENCH_SET + "+25", BENCH_SET + "+35", BENCH_SET + "+45"]:
        base, _, extra = name.partition("+")
        gs = make_gene_set(**(EXTRA_SETS.get(base) or CONFIGS[base]))
        k = int(calculate_k(gs.residues))
        if extra:
            gs = with_short_gene(gs, int(extra), k)
        r = simulate(name, gs, k)
        print(json.dumps(r))
        for f, s in r["forms"].items():
            if s["cycles"]:
                print(f"# {name} {f} form: {s['cycles']} cycles of {s['rows_per_cycle']} rows / {s['lookups_per_cycle']} lookups, mean T {s['mean_T']}: "
                      + "  ".join(f"({c}) {100 * s['survivor_share'][c]:.1f} % survive, {s['touched_slots_per_cycle'][c]} slots" for c in "abcx"), file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
