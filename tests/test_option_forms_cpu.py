"""tests/option_forms.py without a device: its option names and defaults are the library's, every "same results" row of README's
option table has a form, its regime constants are the kernels', its sets lie beyond them, and scenarios x forms is complete."""
import re
from pathlib import Path

import numpy as np

from tests import option_forms as F

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pandelos_amd" / "csrc"


def _set_option_source():
    text = (CSRC / "pdl_api.hip").read_text()
    body = text[text.index("int pdl_set_option("):]
    return body[:body.index("\n}\n")]


def test_option_names_and_defaults_are_the_librarys():
    body = _set_option_source()
    taken = set(re.findall(r'n == "(\w+)"', body))
    named = set(F.DEFAULTS) | {name for form in F.FORMS.values() for name, _ in form}
    assert named <= taken, named - taken
    assert named == set(F.DEFAULTS)                                   # every option of a form has its default listed
    common = (CSRC / "pdl_common.h").read_text()
    for name, value in F.DEFAULTS.items():
        field = re.search(r'n == "' + name + r'"\)(?:\s*\{[^}]*?)?\s*c->(opt_\w+) =', body, re.S).group(1)
        init = re.search(r"\b(?:bool|int|uint32_t|uint64_t) " + field + r" = (\w+);", common).group(1)
        assert {"true": 1, "false": 0}.get(init, init) in (value, str(value)), (name, field, init)
    for name, form in F.FORMS.items():
        assert any(F.DEFAULTS[o] != v for o, v in form), f"form {name} is the default"


def test_every_same_results_row_of_the_readme_has_a_form():
    rows = [r for r in (ROOT / "README.md").read_text().splitlines() if r.startswith("| `") and "same results" in r.lower()]
    assert len(rows) >= 4
    in_forms = {name for form in F.FORMS.values() for name, _ in form}
    for r in rows:
        option = re.match(r"\| `(\w+)`", r).group(1)
        assert option in in_forms, f"README calls `{option}` a form with the same results; tests/option_forms.py has no form of it"


def _constants(*files):
    """name -> value of every `constexpr <type> A = expr, B = expr;` of the files (and PDL_WAVE), products and quotients resolved"""
    raw = {"PDL_WAVE": re.search(r"#define PDL_WAVE (\d+)", (CSRC / "pdl_common.h").read_text()).group(1)}
    for f in files:
        for decl in re.findall(r"^constexpr \w+ ([^;]+);", (CSRC / f).read_text(), re.M):
            for part in decl.split(","):
                if "=" in part:
                    name, expr = part.split("=", 1)
                    raw[name.strip()] = expr.strip()

    def value(name):
        expr = re.sub(r"[A-Za-z_]\w*", lambda m: str(value(m.group(0))), raw[name])
        assert re.fullmatch(r"[\d\s*/()+-]+", expr), (name, expr)
        return int(eval(expr.replace("/", "//")))                     # (digits and arithmetic only)
    return value


def test_the_regime_constants_are_the_kernels():
    value = _constants("pdl_scan.h", "pdl_sort.hip", "pdl_dict.hip")
    for name in ("SCAN_TILE", "LB_CHUNK", "SCAN_INLINE_TILES", "RS_TILE", "RLE_TILE"):
        assert value(name) == getattr(F, name), name
    assert F.MIN_GENES == F.SCAN_TILE and F.MIN_CELLS == F.SCAN_TILE and F.MIN_EDGES == F.SCAN_TILE and F.MIN_QUERY_GENES == F.SCAN_TILE
    assert F.MIN_KMERS == F.LB_CHUNK * F.SCAN_TILE == 64 * F.RLE_TILE == 32 * F.RS_TILE
    assert F.MIN_LARGE_KMERS == F.SCAN_INLINE_TILES * F.SCAN_TILE


def test_the_mid_size_contexts_lie_beyond_every_constant():
    """every context a scenario builds or leaves: the set, what an append starts from, what a removal leaves"""
    for name in ("mid", "mid-last", "mid-two", "mid-middle"):
        ref = F.reference(name)
        U = len(ref.dictionary())
        edges = len(F.network(name)[0])
        assert ref.sequences > F.MIN_GENES, (name, ref.sequences)
        assert ref.kmer_occurrences > F.MIN_KMERS and U > F.MIN_KMERS, (name, ref.kmer_occurrences, U)
        assert ref.kmer_occurrences == int(ref.kseq.sum())
        assert ref.cells > F.MIN_CELLS and edges > F.MIN_EDGES, (name, ref.cells, edges)
    assert F.reference("mid").genomes == F.MID_GENOMES and 0 < F.MIDDLE < F.MID_GENOMES - 1
    assert F.reference("mid-middle").genomes == F.reference("mid-last").genomes == F.MID_GENOMES - 1


def test_the_held_out_genomes_reach_their_regimes():
    k = F.mid_k()
    res, off = F.big_query()
    lens = np.diff(off.astype(np.int64))
    assert len(lens) > F.MIN_QUERY_GENES and lens.min() >= k and abs(float(lens.mean()) - F.BIG_QUERY_LEN) < 2
    big = F.reference("mid+big")
    assert int(big.scores(F.MID_GENOMES)["scoresCount"]) > F.MIN_CELLS and len(F.edges("mid+big", F.MID_GENOMES)[0]) > F.MIN_EDGES
    pl = F.placement("big")
    assert int(pl["is_node"].sum()) > F.MIN_QUERY_GENES and pl["joined"] > 0        # K-place labels more than a tile of query genes
    base_letters = set(np.unique(F.arrays("mid")[0]).tolist())
    for q in ("9", "10", "11", "big"):
        assert set(np.unique(F.QUERIES[q]()[0]).tolist()) <= base_letters, q
        assert int(F.reference(f"mid+{q}").scores(F.MID_GENOMES)["scoresCount"]) > 0
    assert set(np.unique(F.QUERIES["x"]()[0]).tolist()) - base_letters == {ord("X")}
    assert (len(base_letters) + 1) ** k < 1 << 64                      # the union's ranks stay the plain polynomial


def test_the_rekey_scenario_writes_more_than_a_look_back_chunk_of_keys_again():
    """X comes with genome 9 of "mid+x" and with no other: the append re-keys the mid-size set's stream, the removal the union's"""
    from pandelos_amd.remove import remaining_input
    res, off, gen = F.arrays("mid+x")
    holds_x = np.add.reduceat((res == ord("X")).astype(np.int64), off[:-1].astype(np.int64)) > 0
    assert holds_x.any() and set(gen[holds_x].tolist()) == {F.MID_GENOMES} and ord("X") not in F.arrays("mid")[0]
    grown, base = F.reference("mid+x"), F.reference("mid")
    assert grown.genomes == F.MID_GENOMES + 1 and grown.sequences > base.sequences > F.MIN_GENES
    assert grown.kmer_occurrences > base.kmer_occurrences > F.MIN_KMERS          # the keys written again: the base's, then the union's
    assert len(grown.dictionary()) - len(base.dictionary()) > F.SCAN_TILE         # the newcomer's records: more than a tile to merge, to compact
    for got, want in zip(remaining_input(res, off, gen, [F.MID_GENOMES]), F.arrays("mid")):
        assert np.array_equal(got, want)                              # what the removal leaves is the mid-size set


def test_the_profile_and_the_large_set_reach_their_regimes():
    f, g, G, prof, _ = F.profile_case()
    assert len(f) > F.MIN_KMERS and G == F.PROFILE_GENOMES           # both profile scans run over the genes: they cross a look-back chunk
    assert prof["families"] > F.SCAN_TILE                             # the matrix's extras scan has more than one tile
    from tests import matrix_cases as MC
    assert len(MC.slab_plan(prof)) == 2 and len(MC.slab_plan(prof, F.PROFILE_SLAB_BYTES)) > 2
    import json
    d = json.loads((F.H.GOLDEN / "digests_baseline.json").read_text())[F.LARGE]
    shape = d["shape"]
    # at least (mean_len / 2 - k) k-mers per gene would do; the set has sequences x about mean_len of them
    assert d["sequences"] * (shape["mean_len"] // 2 - d["k"]) > F.MIN_LARGE_KMERS
    assert d["sequences"] // d["genomes"] * (d["genomes"] - 1) * (shape["mean_len"] // 2 - d["k"]) > F.MIN_LARGE_KMERS      # the 63-genome base too


def test_scenarios_times_forms_is_complete():
    run = set(F.PAIRS)
    assert len(run) == len(F.PAIRS)
    for s in F.SCENARIOS:
        for f in F.FORMS:
            assert ((s, f) in run) != ((s, f) in F.NOT_RUN), f"({s}, {f}) is neither run nor named in NOT_RUN, or both"
    assert run | set(F.NOT_RUN) == {(s, f) for s in F.SCENARIOS for f in F.FORMS}
    assert all(reason.strip() for reason in F.NOT_RUN.values())
    # NOT_RUN: the large set under the forms that do not change its scans, sorts and record passes, and the pairs a form cannot reach
    unreachable = {("profile_matrix", f) for f in F.SCORING_ONLY} | {("place", "no_host_mirror"), ("place_batch", "no_host_mirror")}
    assert set(F.NOT_RUN) == {("large_append_remove", f) for f in F.FORMS if f not in F.LARGE_FORMS} | unreachable
    for f in F.SCORING_ONLY:                                          # ... which are forms of the scoring pass and its readers alone
        assert {o for o, _ in F.FORMS[f]} <= {"order_subwave", "order_wide_merged", "order_offsets", "host_mirror", "stage_timers"}
    api = (CSRC / "pdl_api.hip").read_text()
    assert len(re.findall(r"c->opt_host_mirror\b(?! =)", api)) == 1 and "use_mirror = need <= PDL_MIRROR_LIMIT && c->opt_host_mirror" in api
    assert not any("opt_host_mirror" in p.read_text() for p in CSRC.iterdir() if p.name not in ("pdl_api.hip", "pdl_common.h"))
    assert {f for s, f in run if s == "large_append_remove"} == set(F.LARGE_FORMS) == {"onepass_scan", "full_radix", "former_records", "all_former"}
    assert set(F.LATE_FORMS) <= set(F.FORMS) and set(F.LATE_SCENARIOS) <= set(F.SCENARIOS)
    assert len(F.LATE_CASES) == len(F.LATE_FORMS) * len(F.LATE_SCENARIOS) * 2
    for form in F.LATE_FORMS:
        for direction in F.DIRECTIONS:
            options, late = F.late_options(form, direction)
            ends = dict(F.in_force(options, late))
            assert ends == ({**F.DEFAULTS, **dict(F.FORMS[form])} if direction == "to" else F.DEFAULTS)
    expected = {"append", "remove", "rekey", "query", "query_batch", "place", "place_batch", "edges_families", "profile_matrix", "batches",
                "dist", "large_append_remove"}
    assert set(F.SCENARIOS) == expected


def test_the_gpu_file_never_skips():
    text = (Path(__file__).with_name("test_gpu_option_forms.py")).read_text() + Path(F.__file__).read_text()
    assert "pytest.skip" not in text and "mark.skip" not in text and "xfail" not in text
