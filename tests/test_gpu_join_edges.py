"""The join tiers with a row ON each of their limits: a table's key count, a staging batch, the walk's chunk and step boundaries, a
tier-0 cycle, a wave's part of the put-aside list.  The rows are planted (tests/join_edge_sets.py: every range, column and count
is decided by an incidence, and tests/test_join_edge_sets_cpu.py holds every set used here to its plan on the CPU oracle).

Every case: each genome's block against the oracle, bit for bit and IN EMISSION ORDER (so the first-touch tracking and the
reference's 2 048-column chunks are compared too), the total cost, aside_reloads == 0 and aside_repeats == 0.  Where the code decides
which tier takes the planted row, that is asserted as well, through the counter of the tier behind (J.Form.handed_on); the
expectations are read off claim() (pdl_join.hip:239-252), the put-aside test (:566) and the cycle rules of pdl_join_part.h:
  keys < LIMIT    the row stays: the counter is 0
  keys > LIMIT    exactly the planted row is handed on — every other gene shares k-mers with fewer genes than LIMIT (checked per set)
  keys == LIMIT   EITHER: the LIMIT-th insert passes the count check at LIMIT - 1 and the row stays, unless a thread that read a slot
                  as empty just before another thread filled it with the same column comes to claim() with the count at LIMIT and
                  gives up.  The cells are asserted, the tier is not.
DESIGN.md section 3 ("The tiers at their limits") lists which test holds which limit."""
import numpy as np
import pytest

from tests import helpers as H
from tests import join_edge_sets as J

pytestmark = pytest.mark.gpu


def _score(name, options, shard=None):
    """Build, compare the blocks with the oracle -> the timings"""
    from tests.test_gpu_query import _native
    case, label = J.case(name), J.ident(name)
    nat = _native(case.k, *case.arrays, options=list(options), shard=shard)
    if shard is None:
        assert nat.cost.total_cost == case.total_cost, label
    for g in (range(case.genomes) if shard is None else shard):
        H.assert_scores_equal(nat.generate_scores_part(g).as_dict(), case.want[g], f"{label} genome {g}")
    tm = nat.timings()
    nat.close()
    assert tm["aside_reloads"] == 0 and tm["aside_repeats"] == 0, label
    return tm


def _expect_tier(name, form, keys, tm, own_posting=0):
    """the planted row has `keys` distinct columns that get a key in `form`; every other row stays (asserted: their partners < LIMIT).
    own_posting = 1: a shard, where every row is a posting of its own ranges and takes a key too (`keys` counts the planted row's)"""
    assert J.planted(name).unplanted_partners + own_posting < form.limit, "the set does not keep its unplanted rows inside this table"
    handed = tm[form.handed_on]
    if keys < form.limit:
        assert handed == 0, f"{J.ident(name)}: {keys} keys < LIMIT {form.limit}, yet {handed} rows left the table"
    elif keys > form.limit:
        assert handed == 1, f"{J.ident(name)}: {keys} keys > LIMIT {form.limit}: the planted row alone leaves, {handed} rows did"
    # keys == LIMIT: either (see the head of this file)


# ---- A: table hand-over, forms without the filter ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.names_a(), ids=J.ident)
def test_a_row_at_the_key_limit_of_an_unfiltered_table(name):
    """every column gets its key at its first sighting: keys = columns.  At TOUCH_CAP and TOUCH_CAP + 1 up to T threads have passed
    the count check together: the table is as full as it ever gets."""
    form = J.FORMS[name[1]]
    _expect_tier(name, form, name[3], _score(name, form.options))


# ---- B: the filter forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.names_b_spread() + J.names_b_unfiltered(), ids=J.ident)
def test_a_row_at_the_key_limit_of_a_filter_table(name):
    """every column has exactly two light sightings in two ranges: it gets its key at the second (a bitmap collision only makes the
    key arrive at the first), so keys = columns again; N >= 2K + 64 gives every wave's part of the put-aside list room.
    "unfiltered": one gene of 2k k-mers switches the filter off (pdl_join.hip:522) and every lookup gets its key at once."""
    form = J.FORMS[name[1]]
    case = J.case(name)
    assert (case.kseq.min() <= 2 * J.K) == (name[2] == "unfiltered") and case.gs.genes >= 2 * name[3] + 64
    _expect_tier(name, form, name[3], _score(name, form.options))


@pytest.mark.parametrize("name", J.names_b_front(), ids=J.ident)
def test_a_front_loaded_row_leaves_through_the_put_aside_list(name):
    """LIMIT - 1 columns, all first sightings before all second ones, no padding: a wave's part of the list is (N + 64) / waves
    entries and the first wave's segment alone holds more first sightings than that — the row goes to tier 2 through nd_w > wcap
    (pdl_join.hip:566), not through the table, which it would fit."""
    form, pl = J.FORMS[name[1]], J.planted(name)
    row = pl.rows[0]
    seg = -(-(-(-row.lookups // 64)) // form.waves) * 64
    part = J.defer_cap(pl.gs.genes) // form.waves
    firsts = min(seg, len(row.columns))                  # wave 0 walks first sightings only; a bit shared with another column makes it one fewer
    bits = J.bitmap_bit(form, pl.column_gene[row.columns])
    assert firsts - (len(bits) - len(np.unique(bits))) > part and len(row.columns) < form.limit
    tm = _score(name, form.options)
    assert tm[form.handed_on] == 1


@pytest.mark.parametrize("fname", J.B_FORMS)
def test_a_wave_s_part_of_the_put_aside_list_exactly_full(fname):
    """Eight sets that differ in their padding alone: the part of a wave goes through eight sizes in a row around the number of first
    sightings wave 0 files (J.exactly_full: known up to the few bits another wave may set first).  The row stays where the part
    holds them — exactly full included — and is handed on where it is one short.  (The padding moves by `waves` genes a step: the
    part is (N + 64) / waves.)"""
    form = J.FORMS[fname]
    stayed = []
    for i in range(8):
        name = ("B", fname, "full", i)
        note = J.planted(name).note
        tm = _score(name, form.options)
        handed = tm[form.handed_on]
        print(f"{J.ident(name)}: part {note['part']}, wave 0 files {note['filed_lo']}..{note['filed_hi']}, handed on {handed}")
        assert handed in (0, 1)
        if note["part"] >= note["filed_hi"]:
            assert handed == 0, f"{J.ident(name)}: a part of {note['part']} holds {note['filed_hi']} first sightings"
        if note["part"] < note["filed_lo"]:
            assert handed == 1, f"{J.ident(name)}: a part of {note['part']} cannot hold {note['filed_lo']} first sightings"
        stayed.append(handed == 0)
    assert any(stayed) and not all(stayed)


# ---- C: staging batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.names_c(), ids=J.ident)
def test_a_row_of_exactly_so_many_staging_batches(name):
    """RB - 1, RB, RB + 1, 2 RB and 2 RB + 1 ranges of one or two postings over fewer columns than LIMIT, each sighted twice or more:
    the row stays.  At RB + 1 and 2 RB + 1 the last batch is a single range."""
    form = J.FORMS[name[1]]
    row = J.planted(name).rows[0]
    assert row.nr == name[2] and len(row.columns) < form.limit
    _expect_tier(name, form, len(row.columns), _score(name, form.options))


# ---- D: the walk's lane-to-range mapping ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.names_d(), ids=J.ident)
def test_the_walk_maps_lanes_to_ranges(name):
    """Range-length patterns that put a range start on every lane, on a chunk boundary and one lane either side of it, on the end
    of a 4- or 8-chunk step (12 x 256, 6 x 512: `vw <= f_hi` at equality in the count of ranges a step passes, pdl_join.hip:429),
    with the 64th following range on the end of the step (64 x 4, 64 x 8, and 700 x 1 in its last chunk: readlane(vw, 63) >= f_hi at
    equality, :406) and one lookup short of it (63 x 4 + 3 + 1), past the staged batch (the 0xffffffff filler of s_cum) — all light, and with about a tenth of the lookups heavy.  The columns are LIMIT - 1 of the form or fewer (two sightings
    each where the pattern has the lookups): the row stays.  "tier3": 600 columns behind the tiny tier 2, for the HBM kernel."""
    fname = name[1]
    row = J.planted(name).rows[0]
    assert bool(row.heavy.any()) == bool(name[3])
    if fname == "tier3":
        tm = _score(name, J.FORMS["tiny2"].options)
        assert tm["overflow_rows"] >= 1
        return
    form = J.FORMS[fname]
    _expect_tier(name, form, len(row.columns), _score(name, form.options))


# ---- E: tier 0 forced on ----------------------------------------------------------------------------------------------------------------
# (a set with a short gene runs the bitmap form only with the rule on: "sift_threshold" 0 launches the counters whatever the set's threshold)
E_CASES = [(name, s) for name in J.names_e() for s in (0, 1) if not (name[4] and s == 0)]


@pytest.mark.parametrize("name,sift_threshold", E_CASES, ids=[f"{J.ident(n)}-sift{s}" for n, s in E_CASES])
def test_a_tier_0_cycle_at_its_limits(name, sift_threshold):
    """Planted rows are genes 0-3: the first workgroup's first cycle.  Ranges per cycle (960), lookups per cycle (4 096; 8 192 in
    the 512-thread form), a row's part of the table (768, 384, 192 keys in a cycle of 1, 2, 4 rows), the heavy list (64).  The sift
    lets through what its counters or bitmaps say, so the keys of a row are not exactly its columns: the cells are asserted, and
    the tier only where the code leaves no choice —
      961 ranges       more than a cycle stages: handed to the filter tier (pdl_join_part.h:174)
      8 193 lookups    more than the 512-thread form's cycle: handed on by both forms (:254-257)
      4 097 lookups    more than the 256-thread form's cycle, so the 512-thread form takes it: 512 columns fit its table and the
                       columns' own rows are short, so NO row reaches the filter tier
      65 heavy lookups one more than the side list holds: the cycle is void (:458) and its single row handed on (:506-507);
                       with 63 and 64 the list holds them and no row reaches the filter tier
    The four-row sets keep every row's columns within the 192 keys of its part (checked on the CPU): a cycle whose part overflows is
    thrown away and its rows run again one by one, and the packed cycle would go uncompared.
    A set with one gene of 5k k-mers has a sift threshold below PT_SIFT_T_MIN: the bitmap form of the kernel runs (with the rule on;
    those sets are not run with "sift_threshold" 0, which launches the counters)."""
    _, kind, a, b, short = name
    case = J.case(name)
    assert H.sift_form(int(case.kseq.min()), case.k, sift_threshold) == ("bitmaps" if short else "counters") and case.kseq.min() > 2 * J.K
    tm = _score(name, [("join_tier0", 1), ("sift_threshold", sift_threshold)])
    assert tm["tier1_rows"] <= tm["scored_rows"]
    if (kind, a, b) in (("ranges", 1, 961), ("lookups", 1, 8193)):
        assert tm["tier1_rows"] >= 1
    if (kind, a, b) == ("lookups", 1, 4097):
        assert tm["tier1_rows"] == 0
    if kind == "heavy":
        assert (tm["tier1_rows"] >= 1) if b > J.PT_HEAVY_CAP else (tm["tier1_rows"] == 0)


# ---- F: the 16-byte ranges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.names_f(), ids=J.ident)
def test_unpacked_ranges_at_the_same_edges(name):
    """A genome shard set before the build: uint4 ranges {first posting, postings, own count, group size}, whole groups
    (pdl_dict.hip:923, MODE 0).  The planted row opens the middle genome, half of its columns lie below it; the row itself is a
    posting of each of its ranges and takes a key.  The key-limit sets therefore plant LIMIT - 2 and LIMIT columns — LIMIT - 1 keys:
    the row stays; LIMIT + 1: it alone is handed on — in the layouts of section A (tier 2) and B (form 10).  In the walk patterns a
    range is one posting longer than its name says; there the cells are asserted and the tier is not."""
    fname = name[1]
    case = J.case(name)
    assert J.planted(name).middle and case.genomes == 3
    tm = _score(name, J.FORMS[fname].options, shard=[1])
    if name[0] == "FA":
        _expect_tier(name, J.FORMS[fname], name[3] + 1, tm, own_posting=1)
