"""Small launches that share one (option "fused_glue" 1, the default; 0: each its own launch).

  k_kseq_lengths ("fused_glue" n > 1 only: measured, it does not pay) the k-mers per gene, their prefix and the cleared per-gene
                 costs with the clearing of the control block in front (k_zero_u64 and the three-launch scan of KseqFlag /
                 KseqApply), for up to min(n, 65 536) genes: 1024 threads and 4096 genes per workgroup, each adding up the genes in
                 front of its own
  k_open_pass    the row / gene descriptors (k_row_desc) and the clearing of the maxima, counters and mirror bookkeeping
                 (k_zero_ranges) that open the first scoring pass over a task layout; a repeated pass clears alone
  k_close_build  the genes' places among the sorted ranges (k_seq_offsets) and the per-genome costs with the k-mer statistics
                 (k_genome_cost) that close a build's range stage; pdl_ensure_costs and the multi-GPU build keep them apart

The last two split their grid by workgroup index, 256 genes or rows per workgroup.  Every case runs under 65 536, 1 and 0: the dictionary,
the k-mers per gene, the per-gene and per-genome costs, "Total cost" and the Scores must be the CPU oracle's."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K = 3
KLEN = 65536                                             # "fused_glue" n > 1: as 1, and K-len in one launch for up to n genes (at most 65 536)
FUSED = [KLEN, 1, 0]
BODY = np.array([c for c in H.LETTERS if c not in b"KLM"], dtype=np.uint8)


def _set(n, genomes=3, seed=11, short=()):
    """n genes, genome by genome, in families of `genomes` members; the genes listed in `short` are given (length) residues:
    shorter than k or empty, they have no k-mer"""
    rng = np.random.default_rng(seed + n)
    fams = max(1, n // genomes)
    bases = [BODY[rng.integers(0, len(BODY), int(rng.integers(25, 36)))] for _ in range(fams)]
    short = dict(short)
    genes, gen = [], []
    for i in range(n):
        s = bases[i % fams].copy()
        m = rng.random(len(s)) < 0.1
        s[m] = BODY[rng.integers(0, len(BODY), int(m.sum()))]
        genes.append(s[:short[i]] if i in short else s)
        gen.append(min(i * genomes // n, genomes - 1) if n >= genomes else i)
    return H._as_gene_set(genes, gen, [-1] * n)


@functools.lru_cache(maxsize=None)
def _case(n, short=()):
    return H.OracleCase(_set(n, short=short), K)


def _short_set(n, genomes=3, seed=23):
    """n genes of 3 to 6 residues, genome by genome"""
    rng = np.random.default_rng(seed + n)
    genes = [BODY[rng.integers(0, len(BODY), int(rng.integers(3, 7)))] for _ in range(n)]
    gen = [min(i * genomes // n, genomes - 1) if n >= genomes else i for i in range(n)]
    return H._as_gene_set(genes, gen, [-1] * n)


@functools.lru_cache(maxsize=None)
def _short_case(n):
    return H.OracleCase(_short_set(n), K)


def _open(fused, options=(), flags=0):
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open(flags=flags)
    nat.set_option("fused_glue", fused)
    for name, v in options:
        nat.set_option(name, v)
    return nat


def _assert_build(nat, c, label):
    ranks, seqs, counts = nat.dictionary()
    d = c.dictionary
    assert np.array_equal(ranks, d["rank"]) and np.array_equal(seqs, d["seq"]) and np.array_equal(counts, d["count"]), f"{label}: dictionary"
    assert nat.cost.total_cost == c.total_cost, f"{label}: Total cost"
    assert [nat.genome_cost(g) for g in range(c.genomes)] == c.genome_cost, f"{label}: genome costs"
    cost, kl = nat.sequence_costs()
    assert np.array_equal(kl, c.kseq), f"{label}: k-mers per gene"
    assert np.array_equal(cost, c.total_visited), f"{label}: per-gene lookups"


def _assert_scores(nat, c, label):
    for g in range(c.genomes):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), c.want[g], f"{label} genome {g}")


def _check(c, fused, label, options=()):
    nat = _open(fused, options)
    nat.preprocess(c.k, *c.arrays)
    _assert_scores(nat, c, label)            # (first: the costs are made on demand, behind the scoring pass)
    _assert_build(nat, c, label)
    nat.close()


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 512, 513])
def test_gene_counts_around_a_workgroup(n, fused):
    """256 genes per workgroup in both halves of both launches; N + 1 offsets, so 255 and 256 genes differ too"""
    _check(_case(n), fused, f"{n} genes, fused_glue {fused}")


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("n", [1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 77])
def test_gene_counts_around_the_klen_kernels_threads_and_span(n, fused):
    """1024 threads of four genes: 4096 genes per workgroup; 4097 genes: a second workgroup adds up a whole one in front, 8269: the
    third two of them"""
    _check(_short_case(n), fused, f"{n} short genes, fused_glue {fused}")


@pytest.mark.parametrize("n", [299, 300, 301, 4097])
def test_above_a_lowered_bound_the_scan_stays(n):
    """"fused_glue" 300: K-len's one launch for up to 300 genes, the clearing launch and the three-launch scan beyond; the other shared
    launches as with 1"""
    _check(_short_case(n), 300, f"{n} short genes, fused_glue 300")


@pytest.mark.parametrize("fused", FUSED)
def test_genes_without_a_kmer_at_the_front_in_the_middle_and_at_the_end(fused):
    n = 300
    short = ((0, 0), (1, 2), (149, 1), (150, 0), (151, 2), (298, 2), (299, 0))
    c = _case(n, short)
    assert all(c.kseq[i] == 0 for i, _ in short)
    _check(c, fused, f"short and empty genes, fused_glue {fused}")


@pytest.mark.parametrize("fused", FUSED)
def test_no_gene_has_a_kmer(fused):
    from pandelos_amd import _lib
    gs = H._as_gene_set([BODY[:2], BODY[:0], BODY[3:5], BODY[:1]], [0, 0, 1, 1], [-1] * 4)
    nat = _open(fused)
    with pytest.raises(_lib.PdlError) as e:
        nat.preprocess(K, gs.residues, gs.offsets, gs.genome_of)
    assert e.value.code == _lib.PDL_ERR_EMPTY
    c = _case(257)                                       # ... and the context goes on
    nat.preprocess(c.k, *c.arrays)
    _assert_scores(nat, c, f"after PDL_ERR_EMPTY, fused_glue {fused}")
    nat.close()


@pytest.mark.parametrize("fused", FUSED)
def test_offsets_that_do_not_ascend_to_the_residue_count(fused):
    from pandelos_amd import _lib
    c = _case(257)
    res, off, gen = c.arrays
    for bad in (np.r_[off[:100], off[101], off[100], off[102:]], np.r_[off[:255], off[256], off[255], off[257:]]):
        nat = _open(fused)
        with pytest.raises(_lib.PdlError) as e:
            nat.preprocess(c.k, res, bad.astype(np.uint64), gen)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT
        nat.close()


@pytest.mark.parametrize("fused", FUSED)
def test_a_repeated_pass_and_a_second_build(fused):
    """staging_cap 16: the first pass overflows, the second clears without the descriptors' half"""
    c = _case(257)
    label = f"fused_glue {fused}"
    nat = _open(fused, [("staging_cap", 16)])
    nat.preprocess(c.k, *c.arrays)
    _assert_scores(nat, c, label + ", tiny staging")
    c2 = _case(513)
    nat.set_option("staging_cap", 0)
    nat.preprocess(c2.k, *c2.arrays)
    _assert_scores(nat, c2, label + ", second build")
    _assert_build(nat, c2, label + ", second build")
    nat.close()


@pytest.mark.parametrize("fused", FUSED)
def test_a_shard_has_fewer_rows_than_genes(fused):
    """the descriptors' half covers max(rows, genes); a shard set before the build, then another one (reshard)"""
    c = _case(513)
    nat = _open(fused)
    nat.set_genome_shard([1])
    nat.preprocess(c.k, *c.arrays)
    H.assert_scores_equal(nat.generate_scores_part(1).as_dict(), c.want[1], f"shard [1], fused_glue {fused}")
    nat.set_genome_shard([0, 2])
    for g in (0, 2):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), c.want[g], f"shard [0, 2], fused_glue {fused}, genome {g}")
    nat.close()


@pytest.mark.parametrize("fused", FUSED)
def test_device_input(fused):
    """pdl_preprocess_device: the genome layout arrives while K-len runs"""
    import torch
    from tests.test_gpu_dist import _device_inputs
    c = _case(513)
    t_res, t_off, t_gen = _device_inputs(*c.arrays)
    nat = _open(fused)
    nat.preprocess_device(c.k, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), len(c.gs.genome_of), len(c.gs.residues), keepalive=(t_res, t_off, t_gen))
    torch.cuda.synchronize()
    _assert_scores(nat, c, f"device input, fused_glue {fused}")
    _assert_build(nat, c, f"device input, fused_glue {fused}")
    nat.close()


@pytest.mark.parametrize("fused", FUSED)
def test_ingested_file(fused, tmp_path):
    res, off, gen, k, fx = H.load_small("synth_5x60x80_k3")
    path = tmp_path / "set.faa"
    path.write_bytes(fx["faa"].tobytes())
    nat = _open(fused)
    ing = nat.ingest_faa(path)
    assert ing["sequences"] == len(gen)
    nat.preprocess_ingested(k)
    assert nat.cost.total_cost == int(fx["total_cost"])
    H.assert_scores_equal_fixture(lambda g: nat.generate_scores_part(g).as_dict(), fx, nat.cost.genomes, f"ingested, fused_glue {fused}")
    assert [nat.genome_cost(g) for g in range(nat.cost.genomes)] == [int(x) for x in fx["genome_cost"]]
    nat.close()


@functools.lru_cache(maxsize=None)
def _four_genomes():
    full = H.OracleCase(_set(260, genomes=4), K)
    res, off, gen = full.arrays
    n3 = int(np.searchsorted(gen, 3))
    cut = int(off[n3])
    base = H.OracleCase(H._as_gene_set([res[int(off[i]):int(off[i + 1])] for i in range(n3)], gen[:n3], [-1] * n3), K)
    last = (res[cut:], (off[n3:] - off[n3]).astype(np.uint64))
    return full, base, last


@pytest.mark.parametrize("fused", FUSED)
def test_append_and_remove_on_four_genomes(fused):
    """both rebuild the range stage behind their own clearing of the control block"""
    full, base, last = _four_genomes()
    label = f"fused_glue {fused}"
    nat = _open(fused)
    nat.preprocess(base.k, *base.arrays)
    _assert_scores(nat, base, label + ", three genomes")
    nat.append(*last)
    _assert_scores(nat, full, label + ", the fourth appended")
    _assert_build(nat, full, label + ", the fourth appended")
    nat.remove([3])
    _assert_scores(nat, base, label + ", the fourth removed")
    _assert_build(nat, base, label + ", the fourth removed")
    nat.close()


@pytest.mark.parametrize("fused", FUSED)
def test_only_complexity(fused):
    """no range lists: k_seq_offsets does not run, K-cost has a launch of its own"""
    c = _case(513)
    nat = _open(fused)
    nat.preprocess(c.k, *c.arrays, only_complexity=True)
    assert nat.cost.total_cost == c.total_cost
    assert [nat.genome_cost(g) for g in range(c.genomes)] == c.genome_cost
    cost, kl = nat.sequence_costs()
    assert np.array_equal(kl, c.kseq) and np.array_equal(cost, c.total_visited)
    nat.close()


@pytest.mark.parametrize("ranges", ["sender", "owner"])
@pytest.mark.parametrize("fused", FUSED)
def test_two_ranks(fused, ranges):
    """the multi-GPU build runs k_seq_offsets and k_genome_cost apart; its scoring passes open with k_open_pass"""
    from pandelos_amd.distributed import LocalRanks
    from tests.test_gpu_dist import _device_inputs
    c = _case(513)
    label = f"W=2, {ranges} ranges, fused_glue {fused}"
    lr = LocalRanks(2, sender_ranges=ranges == "sender")
    for nat in lr.ranks:
        nat.set_option("fused_glue", fused)
    lr.preprocess(c.k, *_device_inputs(*c.arrays), len(c.gs.genome_of), len(c.gs.residues))
    assert lr.total_cost == c.total_cost, label
    lr.score_all()
    for g in range(c.genomes):
        H.assert_scores_equal(lr.generate_scores_part(g).as_dict(), c.want[g], f"{label} genome {g}")
    lr.close()
