"""A single query is a batch of one: pdl_query_scores and pdl_query_batch([q]) share their host driver and their result view
(pandelos_amd/csrc/pdl_query.h: q_join_and_order, pdl_query_cells), so on ONE context query_scores(q), query_batch([q]) and
query_scores(q) again give the same block byte for byte and the same sizes, record counts and genome cost — on the smallest query
fixture of tests/golden/query and on the planted row of tests/query_join_sets.py that must leave the LDS table.  There the batch of
one lays the HBM tables out for the same N + n columns as the single query, so the third call finds them clean."""
import numpy as np
import pytest

from tests import helpers as H
from tests import query_join_sets as S
from tests.test_query_golden import QDIR, assert_block, load_case

pytestmark = pytest.mark.gpu
SAME = ("residues", "kmer_occurrences", "records", "matched_records", "genome_cost")


def _three_calls(nat, q, label):
    """-> the join's books of the three calls; the blocks and the per-query reports are compared here"""
    blocks, infos, books = [], [], []
    for call in ("query_scores", "query_batch", "query_scores again"):
        if call == "query_batch":
            (b,) = nat.query_batch([q])
            assert nat.last_query_batch_info["chunks"] == 1, label
            infos.append(nat.last_query_batch_info["queries"][0])
        else:
            b = nat.query_scores(*q)
            infos.append(nat.last_query_info)
        blocks.append(b.as_dict())
        books.append(nat.last_query_join_info)
    for call, b, i in zip(("query_batch", "query_scores again"), blocks[1:], infos[1:]):
        assert b["scoresCount"] == blocks[0]["scoresCount"], f"{label}: {call}"
        for f in H.FIELDS:
            x, y = np.ascontiguousarray(b[f]), np.ascontiguousarray(blocks[0][f])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{label}: {call}, field {f} differs from the first query_scores"
        assert {f: i[f] for f in SAME} == {f: infos[0][f] for f in SAME}, f"{label}: {call}"
    return blocks[0], books


def test_smallest_fixture():
    from pandelos_amd.pangene_native import PangeneNative
    name = min(QDIR.glob("*.npz"), key=lambda p: p.stat().st_size).stem
    fx, base, query, k, G = load_case(name)
    nat = PangeneNative(k, base)
    block, books = _three_calls(nat, query.flatten()[:2], name)
    assert_block(block, fx, name)
    assert books[0] == books[1] == books[2], (name, books)
    nat.close()


def test_planted_row_on_the_hbm_tables():
    from pandelos_amd.pangene_native import PangeneNative
    name = f"A-single-{S.MUST_LEAVE}"
    c = S.case(name)
    nat = PangeneNative.open()
    nat.preprocess(S.K, *c.base)
    _, books = _three_calls(nat, c.query(0), name)
    print(name, books)
    for b in books:
        assert b["overflow_rows"] == 1 and b["hbm_launches"] == 1 and b["hbm_workgroups"] == 1 and b["rows"] == len(c.queries[0]), (name, books)
    assert books[0]["hbm_clears"] == 1, (name, books)              # (a fresh context: the tables are laid out once)
    assert books[1]["hbm_clears"] == 0 and books[2]["hbm_clears"] == 0, f"{name}: the tables a batch of one leaves clean are the single query's: {books}"
    nat.close()
