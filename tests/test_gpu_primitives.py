"""The three generic device primitives against numpy, through the test hooks (pandelos_amd/csrc/pdl_hooks.hip) on a context
without a build: scan_and_apply in its three-launch and one-launch forms, pdl_radix_offsets, pdl_sort_pairs, pdl_merge_streams.
The cases, their inputs and the references are tests/primitive_cases.py's (checked on the CPU by test_primitive_cases_cpu.py);
every comparison is exact.

Device buffers are torch tensors, longer than needed and filled with a poison word; inputs behind the counted length are poison
too (flags of 0xffffffff, maximal keys).  Every run asserts that nothing behind the counted length was written and — by the
exact comparison — that no poison reached a result.  A mismatch names the first wrong element and the tile it lies in."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import primitive_cases as P

pytestmark = pytest.mark.gpu

PAD = 333                                # elements behind every buffer's counted length


def _torch():
    import torch
    return torch


def _open(**options):
    from pandelos_amd.pangene_native import PangeneNative
    nat = PangeneNative.open()
    for name, value in options.items():
        nat.set_option(name, value)
    return nat


_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _dev(arr, pad=PAD, lead=0):
    """arr on the device between `lead` poison elements and `pad` of them -> (tensor, address of arr's first element)"""
    torch = _torch()
    a = np.ascontiguousarray(arr)
    t = torch.full((lead + len(a) + pad,), -1, dtype=torch.int32 if a.dtype.itemsize == 4 else torch.int64, device="cuda")
    if len(a):
        t[lead:lead + len(a)] = torch.from_numpy(a.view(_SIGNED[a.dtype])).cuda()
    return t, t.data_ptr() + lead * a.dtype.itemsize


def _poison(n, itemsize=4):
    torch = _torch()
    return torch.full((n,), -1, dtype=torch.int32 if itemsize == 4 else torch.int64, device="cuda")


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _ok(nat, rc):
    nat._check(rc)


def _same(got, want, label, tile):
    if np.array_equal(got, want):
        return
    assert got.shape == want.shape, f"{label}: {got.shape} != {want.shape}"
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    raise AssertionError(f"{label}: {len(bad)} of {len(want)} differ, first at {i} (tile {i // tile}, place {i % tile}): "
                         f"got {int(got[i]):#x}, want {int(want[i]):#x}; last at {int(bad[-1])}")


def _untouched(tail, label):
    poison = np.iinfo(tail.dtype).max
    bad = np.flatnonzero(tail != poison)
    assert len(bad) == 0, f"{label}: {len(bad)} words behind the counted length were written, first {int(bad[0])} behind it"


# ---- scan ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _scan_want(case):
    flags = P.scan_flags(case)
    prefix, total = P.scan_reference(flags, case.count)
    return flags, prefix, total


def _run_scan(nat, case, two_phase, with_total2=True):
    torch = _torch()
    flags, want_prefix, want_total = _scan_want(case)
    n, count = case.n_bound, case.count
    label = f"scan {case.name} two_phase={two_phase}"
    d_flags, p_flags = _dev(flags[:count], pad=n - count + PAD)               # poison behind the count
    d_prefix, d_seen = _poison(n + PAD), _poison(n + PAD)
    d_total = _poison(2, 8)
    d_total2 = _poison(8)                                                     # the second total at word 1: addr % 8 == 4
    assert (d_total2.data_ptr() + 4) % 8 == 4
    d_n = None if case.d_n is None else torch.tensor([case.d_n], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _ok(nat, nat._lib.pdl_test_scan(nat._ctx, p_flags, n, None if d_n is None else d_n.data_ptr(), d_prefix.data_ptr(), d_seen.data_ptr(),
                                    int(two_phase), d_total.data_ptr(), d_total2.data_ptr() + 4 if with_total2 else None))
    totals = _host(d_total)
    assert int(totals[0]) == want_total, f"{label}: total {int(totals[0])}, want {want_total}"
    _untouched(totals[1:], f"{label} total")
    t2 = _host(d_total2)
    if with_total2:
        assert (int(t2[1]), int(t2[2])) == (want_total, 0), f"{label}: second total {int(t2[1])} | {int(t2[2])}, want {want_total}"
        _untouched(t2[[0, 3, 4, 5, 6, 7]], f"{label} second total")
    else:
        _untouched(t2, f"{label} second total")
    prefix, seen = _host(d_prefix), _host(d_seen)
    _same(prefix[:count], want_prefix, f"{label} prefix", P.SCAN_TILE)
    _same(seen[:count], flags[:count], f"{label} flag seen", P.SCAN_TILE)
    _untouched(prefix[count:], f"{label} prefix")
    _untouched(seen[count:], f"{label} flag seen")


@pytest.mark.parametrize("two_phase", [0, 1])
@pytest.mark.parametrize("case", P.SCAN_SIZE_CASES, ids=lambda c: c.name)
def test_scan_three_launches_at_every_switch(case, two_phase):
    nat = _open(onepass_scan=0)
    _run_scan(nat, case, two_phase, with_total2=case.kind == "small")
    nat.close()


@pytest.mark.parametrize("two_phase", [0, 1])
@pytest.mark.parametrize("case", P.SCAN_EDGE_CASES, ids=lambda c: c.name)
def test_scan_three_launches_edge_values(case, two_phase):
    nat = _open(onepass_scan=0)
    _run_scan(nat, case, two_phase)
    nat.close()


@pytest.mark.parametrize("two_phase", [0, 1])
@pytest.mark.parametrize("case", P.SCAN_COUNT_CASES, ids=lambda c: c.name)
def test_scan_three_launches_count_on_the_device(case, two_phase):
    nat = _open(onepass_scan=0)
    _run_scan(nat, case, two_phase)
    nat.close()


@pytest.mark.parametrize("onepass", [0, 1])
def test_scan_of_nothing(onepass):
    nat = _open(onepass_scan=onepass)
    for two_phase in (0, 1):
        _run_scan(nat, P.ScanCase("host_n0", 0, "zero"), two_phase)
    nat.close()


@pytest.mark.parametrize("case", P.ONEPASS_CASES + P.ONEPASS_COUNT_CASES, ids=lambda c: c.name)
def test_scan_one_launch(case):
    nat = _open(onepass_scan=1)
    for two_phase in (0, 1):                                                  # (the second run: a new epoch over the same words)
        _run_scan(nat, case, two_phase)
    nat.close()


def test_scan_one_launch_sequence_on_one_context():
    """epochs, look-back buffers that grow, a chunk_incl base that moves with the chunk count"""
    nat = _open(onepass_scan=1)
    for i, case in enumerate(P.ONEPASS_SEQUENCE):
        _run_scan(nat, case, i % 2)
    nat.close()


# ---- offsets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lean_radix,onepass", [(1, 0), (0, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("case", P.OFFSETS_CASES, ids=lambda c: c.name)
def test_radix_offsets(case, lean_radix, onepass):
    torch = _torch()
    nat = _open(lean_radix=lean_radix, onepass_scan=onepass)
    label = f"offsets {case.name} lean_radix={lean_radix} onepass_scan={onepass}"
    counts = P.offsets_counts(case)
    t = case.n_tiles
    d_counts, p_counts = _dev(counts.reshape(-1))
    d_offs, d_total, d_digit = _poison(counts.size + PAD), _poison(2, 8), _poison(P.RADIX_BINS + PAD)
    lean = C.c_int(-1)
    torch.cuda.synchronize()
    _ok(nat, nat._lib.pdl_test_radix_offsets(nat._ctx, p_counts, d_offs.data_ptr(), t, d_total.data_ptr(), d_digit.data_ptr(), C.byref(lean)))
    want_lean = P.offsets_lean_expected(t, lean_radix, onepass)
    assert lean.value == int(want_lean), f"{label}: out_lean {lean.value}"
    assert want_lean == (lean_radix == 1 and onepass == 0 and t <= 65536)
    want_offs, want_sum = P.offsets_reference(counts, want_lean)
    offs, total, digit = _host(d_offs), _host(d_total), _host(d_digit)
    # (first wrong element: row = digit, `tile` = the row's length)
    _same(offs[:counts.size], want_offs.reshape(-1), f"{label} offs (digit-major, rows of {t})", t)
    _untouched(offs[counts.size:], f"{label} offs")
    if want_lean:
        _same(digit[:P.RADIX_BINS], want_sum, f"{label} digit totals", 1)
        _untouched(digit[P.RADIX_BINS:], f"{label} digit totals")
        _untouched(total, f"{label} total (the scatter's to write)")
    else:
        assert int(total[0]) == want_sum, f"{label}: total {int(total[0])}, want {want_sum}"
        _untouched(total[1:], f"{label} total")
        _untouched(digit, f"{label} digit totals")
    nat.close()


# ---- sort ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _big_order(n, seed):
    """the stable order of a big case's 16-bit keys: the same for every width pair and both offsets forms"""
    return np.argsort(P._low16(n, seed), kind="stable")


def _sort_want(case, keys, vals):
    if case.n >= P.SORT_BIG_N[0]:
        order = _big_order(case.n, case.seed)
        return keys[order], order.astype(np.uint64 if case.val_bytes == 8 else np.uint32)
    return P.sort_reference(case, keys, vals)


def _run_sort(nat, case, label, first_counts=None):
    """-> (keys, values) of the counted prefix as the device left them, checked against the reference"""
    torch = _torch()
    keys = P.sort_keys(case)
    vals = None if case.iota else P.sort_values(case)
    n, count = case.n, case.count
    d_ka, p_ka = _dev(keys[:count], pad=n - count + PAD)                      # maximal keys behind the count
    d_kb = _poison(n + PAD, case.key_bytes)
    if vals is None:
        d_va = _poison(n + PAD, case.val_bytes)                               # iota_values: never read
    else:
        d_va, _ = _dev(vals[:count], pad=n - count + PAD)
    d_vb = _poison(n + PAD, case.val_bytes)
    d_n = None if case.d_n is None else torch.tensor([case.d_n], dtype=torch.int64, device="cuda")
    d_counts = None if first_counts is None else _dev(first_counts.reshape(-1))[0]
    in_b, total = C.c_int(-1), C.c_uint64(12345)
    torch.cuda.synchronize()
    _ok(nat, nat._lib.pdl_test_sort_pairs(nat._ctx, case.key_bytes, case.val_bytes, p_ka, d_kb.data_ptr(), d_va.data_ptr(), d_vb.data_ptr(), n,
                                          case.end_bit, int(case.iota), None if d_n is None else d_n.data_ptr(), case.begin_bit, int(case.below),
                                          None if d_counts is None else d_counts.data_ptr(), C.byref(in_b), C.byref(total)))
    passes = (min(max(case.end_bit, 1), case.key_bits) + 7) // 8 - case.begin_bit // 8
    assert in_b.value == passes % 2, f"{label}: result in buffer {'ab'[in_b.value]} after {passes} passes"
    assert total.value == count, f"{label}: total {total.value}, want {count}"
    got_k, got_v = (_host(d_kb), _host(d_vb)) if in_b.value else (_host(d_ka), _host(d_va))
    oth_k, oth_v = (_host(d_ka), _host(d_va)) if in_b.value else (_host(d_kb), _host(d_vb))
    want_k, want_v = _sort_want(case, keys, vals)
    _same(got_k[:count], want_k, f"{label} keys", P.RADIX_TILE)
    _same(got_v[:count], want_v, f"{label} values", P.RADIX_TILE)
    for name, buf in (("keys", got_k), ("values", got_v), ("other keys", oth_k), ("other values", oth_v)):
        _untouched(buf[count:], f"{label} {name}")
    return got_k[:count].copy(), got_v[:count].copy()


SORT_GROUPS = {"sizes": P.sort_size_cases, "end_bits": P.sort_end_bit_cases, "begin_bits": P.sort_begin_bit_cases, "patterns": P.sort_pattern_cases,
               "device_counts": P.sort_count_cases}


@pytest.mark.parametrize("lean_radix", [1, 0])
@pytest.mark.parametrize("widths", P.WIDTHS, ids=lambda w: f"k{w[0]}v{w[1]}")
@pytest.mark.parametrize("group", list(SORT_GROUPS))
def test_sort_pairs(group, widths, lean_radix):
    nat = _open(lean_radix=lean_radix)
    for case in SORT_GROUPS[group](*widths):
        _run_sort(nat, case, f"sort {case.name} lean_radix={lean_radix}")
    nat.close()


@pytest.mark.parametrize("lean_radix", [1, 0])
@pytest.mark.parametrize("widths", P.WIDTHS, ids=lambda w: f"k{w[0]}v{w[1]}")
def test_sort_pairs_first_counts_filed(widths, lean_radix):
    """the first pass's histogram from the caller: the same pairs as with the sort's own"""
    nat = _open(lean_radix=lean_radix)
    for case in P.sort_filed_cases(*widths):
        label = f"sort {case.name} lean_radix={lean_radix}"
        keys = P.sort_keys(case)
        own_k, own_v = _run_sort(nat, case, label + " (own histogram)")
        filed_k, filed_v = _run_sort(nat, case, label + " (filed histogram)", first_counts=P.sort_first_counts(case, keys))
        assert np.array_equal(own_k, filed_k) and np.array_equal(own_v, filed_v), label
    nat.close()


BIG_SORT = [(c, lean) for i in range(len(P.SORT_BIG_N)) for w in P.WIDTHS for lean in (1, 0) for c in (P.sort_big_cases(*w)[i],)]


@pytest.mark.parametrize("case,lean_radix", BIG_SORT, ids=lambda x: x.name if isinstance(x, P.SortCase) else f"lean{x}")
def test_sort_pairs_thousands_of_tiles(case, lean_radix):
    """4096 | 4097 | 8193 tiles: one, two and three trips of the one-launch offsets over a row"""
    nat = _open(lean_radix=lean_radix)
    _run_sort(nat, case, f"sort {case.name} lean_radix={lean_radix}")
    nat.close()


# ---- merge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.all_merge_cases(), ids=lambda c: c.name)
def test_merge_streams(case):
    torch = _torch()
    nat = _open()
    inp = P.merge_input(case)
    na, nb = len(inp.a_keys), len(inp.b_keys)
    label = f"merge {case.name}"
    # sources one element into their allocation: element-aligned only
    (d_ak, p_ak), (d_av, p_av) = _dev(inp.a_keys, lead=1), _dev(inp.a_vals, lead=1)
    (d_bk, p_bk), (d_bv, p_bv) = _dev(inp.b_keys, lead=1), _dev(inp.b_vals, lead=1)
    assert p_ak % 16 == case.key_bytes and p_av % 16 == 4 and p_bk % 16 == case.key_bytes and p_bv % 16 == 4
    d_ok, d_ov = _poison(na + nb + PAD, case.key_bytes), _poison(na + nb + PAD)
    assert d_ok.data_ptr() % 16 == 0 and d_ov.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    _ok(nat, nat._lib.pdl_test_merge(nat._ctx, case.key_bytes, p_ak, p_av, na, p_bk, p_bv, nb, inp.b_val_add, case.mask, d_ok.data_ptr(), d_ov.data_ptr()))
    want_k, want_v = P.merge_reference(inp, case.mask)
    got_k, got_v = _host(d_ok), _host(d_ov)
    _same(got_k[:na + nb], want_k, f"{label} keys", P.SCAN_TILE)
    _same(got_v[:na + nb], want_v, f"{label} values", P.SCAN_TILE)
    _untouched(got_k[na + nb:], f"{label} keys")
    _untouched(got_v[na + nb:], f"{label} values")
    nat.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _hook_calls(lib, ctx, bufs):
    """every hook with valid arguments on small buffers -> {name: callable(**what to replace) -> return code}"""
    p = {k: v.data_ptr() for k, v in bufs.items()}
    lean, in_b, total = C.c_int(0), C.c_int(0), C.c_uint64(0)

    def scan(**kw):
        a = dict(flags=p["a"], n=100, d_n=None, prefix=p["b"], seen=p["c"], two_phase=0, total=p["t"], total2=None); a.update(kw)
        return lib.pdl_test_scan(ctx, a["flags"], a["n"], a["d_n"], a["prefix"], a["seen"], a["two_phase"], a["total"], a["total2"])

    def offsets(**kw):
        a = dict(counts=p["a"], offs=p["b"], n_tiles=1, total=p["t"], digit=p["c"], lean=C.byref(lean)); a.update(kw)
        return lib.pdl_test_radix_offsets(ctx, a["counts"], a["offs"], a["n_tiles"], a["total"], a["digit"], a["lean"])

    def sort(**kw):
        a = dict(kb=4, vb=4, ka=p["a"], kb_=p["b"], va=p["c"], vb_=p["d"], n=100, end=32, begin=0, in_b=C.byref(in_b), total=C.byref(total)); a.update(kw)
        return lib.pdl_test_sort_pairs(ctx, a["kb"], a["vb"], a["ka"], a["kb_"], a["va"], a["vb_"], a["n"], a["end"], 0, None, a["begin"], 0, None,
                                       a["in_b"], a["total"])

    def merge(**kw):
        a = dict(kb=4, ak=p["a"], av=p["c"], na=50, bk=p["b"], bv=p["d"], nb=50, ok=p["e"], ov=p["f"]); a.update(kw)
        return lib.pdl_test_merge(ctx, a["kb"], a["ak"], a["av"], a["na"], a["bk"], a["bv"], a["nb"], 7, 0xFFFFFFFF, a["ok"], a["ov"])

    return {"pdl_test_scan": scan, "pdl_test_radix_offsets": offsets, "pdl_test_sort_pairs": sort, "pdl_test_merge": merge}


def _small_buffers():
    torch = _torch()
    bufs = {k: torch.zeros(1024, dtype=torch.int32, device="cuda") for k in "abcdef"}
    bufs["t"] = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return bufs


BAD_ARGUMENTS = [("pdl_test_scan", dict(flags=None)), ("pdl_test_scan", dict(prefix=None)), ("pdl_test_scan", dict(seen=None)), ("pdl_test_scan", dict(total=None)),
                 ("pdl_test_radix_offsets", dict(counts=None)), ("pdl_test_radix_offsets", dict(offs=None)), ("pdl_test_radix_offsets", dict(total=None)),
                 ("pdl_test_radix_offsets", dict(digit=None)), ("pdl_test_radix_offsets", dict(lean=None)),
                 ("pdl_test_sort_pairs", dict(ka=None)), ("pdl_test_sort_pairs", dict(kb_=None)), ("pdl_test_sort_pairs", dict(va=None)),
                 ("pdl_test_sort_pairs", dict(vb_=None)), ("pdl_test_sort_pairs", dict(in_b=None)), ("pdl_test_sort_pairs", dict(total=None)),
                 ("pdl_test_sort_pairs", dict(kb=8, vb=8)), ("pdl_test_sort_pairs", dict(kb=2)), ("pdl_test_sort_pairs", dict(vb=2)), ("pdl_test_sort_pairs", dict(begin=4)),
                 ("pdl_test_merge", dict(ak=None)), ("pdl_test_merge", dict(av=None)), ("pdl_test_merge", dict(bk=None)), ("pdl_test_merge", dict(bv=None)),
                 ("pdl_test_merge", dict(ok=None)), ("pdl_test_merge", dict(ov=None)), ("pdl_test_merge", dict(kb=2)), ("pdl_test_merge", dict(kb=16))]


def test_hooks_refuse_bad_arguments():
    from pandelos_amd import _lib
    nat = _open()
    bufs = _small_buffers()
    calls = _hook_calls(nat._lib, nat._ctx, bufs)
    for name, call in calls.items():
        assert call() == _lib.PDL_OK, name                                    # the valid call the refusals are variations of
    for name, change in BAD_ARGUMENTS:
        assert calls[name](**change) == _lib.PDL_ERR_ARGUMENT, (name, change)
        assert name in nat._lib.pdl_last_error(nat._ctx).decode(), (name, change)
    for name, call in _hook_calls(nat._lib, None, bufs).items():
        assert call() == _lib.PDL_ERR_ARGUMENT, name                          # no context
    for name, call in calls.items():
        assert call() == _lib.PDL_OK, name                                    # a refusal leaves the context as it was
    nat.close()


def test_hooks_refuse_a_built_context_and_leave_it_whole():
    from pandelos_amd import _lib
    from pandelos_amd.pangene_native import PangeneNative
    name = "synth_5x60x80_k3"
    res, off, gen, k, fx = H.load_small(name)
    nat = PangeneNative.from_arrays(k, res, off, gen)
    bufs = _small_buffers()
    for hook, call in _hook_calls(nat._lib, nat._ctx, bufs).items():
        assert call() == _lib.PDL_ERR_STATE, hook
        assert hook in nat._lib.pdl_last_error(nat._ctx).decode(), hook
    for t in bufs.values():
        assert not t.any(), "a refused hook wrote to its buffers"
    assert nat.cost.total_cost == int(fx["total_cost"])
    H.assert_scores_equal_fixture(lambda g: nat.generate_scores_part(g).as_dict(), fx, int(nat.cost.genomes), name)
    nat.close()
