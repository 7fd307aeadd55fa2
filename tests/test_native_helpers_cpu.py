"""The argument helpers of PangeneNative without a GPU, through its public methods and a stub library: the shape of offsets,
the one-genome check of a PangeneIData, the shapes of an edge list.  A refusal here comes before the library is called."""
import numpy as np
import pytest

from pandelos_amd import _lib
from pandelos_amd.pangene_idata import PangeneIData
from pandelos_amd.pangene_native import PangeneNative


class _NoLib:
    """Stands in for libpandelos_amd.so: any call is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.fixture
def nat():
    n = PangeneNative.__new__(PangeneNative)
    n._lib, n._ctx = _NoLib(), None
    n.cost = _lib.PdlCost(genomes=3)
    return n


RES = np.frombuffer(b"ACDEFGHIK", np.uint8)
OFF = np.array([0, 4, 9], np.uint64)


@pytest.mark.parametrize("offsets", [[], np.zeros((2, 2), np.uint64)], ids=["empty", "two dimensions"])
def test_wrong_offsets_shapes_are_refused_with_each_method_s_message(nat, offsets):
    def message(fn):
        with pytest.raises(_lib.PdlError) as e:
            fn()
        assert e.value.code == _lib.PDL_ERR_ARGUMENT
        return str(e.value)
    assert message(lambda: nat.query_scores(RES, offsets)).endswith(": offsets must hold n_query + 1 entries")
    assert message(lambda: nat.place_query(RES, offsets)).endswith(": offsets must hold n_query + 1 entries")
    assert message(lambda: nat.append(RES, offsets)).endswith(": offsets must hold n + 1 entries")
    assert message(lambda: nat.query_batch([(RES, OFF), (RES, offsets)])).endswith(": query 1: offsets must hold n + 1 entries")
    assert message(lambda: PangeneNative.pack_queries([(RES, offsets)])).endswith(": query 0: offsets must hold n + 1 entries")


def test_an_append_checks_genome_of_against_the_offsets(nat):
    with pytest.raises(_lib.PdlError, match="genome_of must hold one id per gene") as e:
        nat.append(RES, OFF, [3, 3, 4])
    assert e.value.code == _lib.PDL_ERR_ARGUMENT


def test_a_two_genome_idata_is_no_query(nat):
    one = PangeneIData.from_arrays(RES, OFF, [0, 0])
    two = PangeneIData.from_arrays(RES, OFF, [0, 1])
    with pytest.raises(ValueError) as e:
        nat.query_idata(two)
    assert str(e.value) == "a query holds exactly one genome, this data holds 2"
    with pytest.raises(ValueError) as e:
        nat.place_idata(two)
    assert str(e.value) == "a query holds exactly one genome, this data holds 2"
    with pytest.raises(ValueError) as e:
        nat.query_batch_idata([one, one, two])
    assert str(e.value) == "a query holds exactly one genome, query 2 holds 2"
    with pytest.raises(ValueError) as e:
        nat.query_idata(PangeneIData())
    assert str(e.value) == "a query holds exactly one genome, this data holds 0"
    with pytest.raises(AssertionError, match="the library was called"):          # one genome: the check lets the call through
        nat.query_idata(one)


@pytest.mark.parametrize("src, dst, genome_of", [([0, 1, 2], [1, 2], [0, 0, 1]), ([[0, 1]], [[1, 2]], [0, 0, 1]), ([0, 1], [1, 2], [[0, 0, 1]])],
                         ids=["src longer than dst", "two dimensions", "genome_of in two dimensions"])
def test_mismatched_edge_arrays_are_refused(nat, src, dst, genome_of):
    want = "src and dst must be two vectors of one length, genome_of a vector"
    with pytest.raises(_lib.PdlError) as e:
        nat.families_of_edges(src, dst, genome_of)
    assert e.value.code == _lib.PDL_ERR_ARGUMENT and str(e.value).endswith(": " + want)
    with pytest.raises(_lib.PdlError) as e:
        nat.placement_of_edges({}, genome_of, 1, src, dst)                       # (refused before the base is looked at)
    assert e.value.code == _lib.PDL_ERR_ARGUMENT and str(e.value).endswith(": " + want)
