"""Option "query_rekey" without a device: where the fixtures live, a model of Q-rebase (pdl_rekey.h: rk_one, k_q_rebase) in Python
integers on top of the re-key model of tests/test_rekey_cpu.py, and the generator of the random cases tests/test_gpu_query_rekey.py
runs — the CONSTRUCTION decides where a new letter falls, no category rests on chance."""
import tempfile
from pathlib import Path

import numpy as np

from pandelos_amd.pangene_idata import PangeneIData
from tests import helpers as H
from tests.test_rekey_cpu import family_genes, pack, rank_table, rekey_one, rekey_plan, with_letters

QRDIR = H.GOLDEN / "query_rekey"
CASES = sorted(p.stem for p in QRDIR.glob("*.npz"))
SEED0, SEEDS_DEFAULT = 23000, 60                       # the range tests/test_gpu_query_rekey.py runs by default


def load_case(name):
    """-> (fixture dict, base PangeneIData, query PangeneIData, k, G), as tests.test_query_golden.load_case over QRDIR"""
    fx = dict(np.load(QRDIR / f"{name}.npz"))
    with tempfile.TemporaryDirectory() as td:
        b, q = Path(td) / "base.faa", Path(td) / "query.faa"
        b.write_bytes(fx["base_faa"].tobytes())
        q.write_bytes(fx["query_faa"].tobytes())
        base, query = PangeneIData.read_from_file(b), PangeneIData.read_from_file(q)
    return fx, base, query, int(fx["k"]), int(fx["G"])


# ---- the model of Q-rebase ----------------------------------------------------------------------------------------------------------
def rebase_plan(base_letters, union_letters, k):
    """rk_query's second half: the plan union -> base (a new letter's entries stay 0) and the union's digits that are new letters"""
    plan = rekey_plan(union_letters, base_letters, k)
    union, base = rank_table(union_letters), rank_table(base_letters)
    plan["absent"] = {d for b, d in union.items() if b not in base}
    return plan


def rebase_one(x, plan):
    """k_q_rebase for one key: -> (the key in the base's alphabet, flag "holds a new letter").  The digits are taken as rekey_one
    takes them; the flag is the OR over the digits of the absent set."""
    B, k = plan["base"], plan["k"]
    digits, rest = [], int(x)
    for _ in range(k):
        digits.append(rest % B)
        rest //= B
    assert rest == 0, "a key at or above B'^k cannot come out of K-rank"
    y = rekey_one(x, plan, B ** k > 1 << 32)
    return y, any(d in plan["absent"] for d in digits)


def key_of(kmer, table, B):
    r = 0
    for b in kmer:
        r = r * B + table[b]
    return r


# ---- the random cases ---------------------------------------------------------------------------------------------------------------
POOL = b"DEFGHIKLMNPQRS"           # base letters come from here; 'A' '*' '#' lie below all of them, 'X' 'Z' above, 'U' above too
BELOW, ABOVE, SHORT_ONLY = b"A*#", b"XZ", b"U"


def query_rekey_case(seed):
    """-> dict(k, base (res, off, gen), query (res, off), query_genes, where, letters, short_letter).  seed % 4 picks where the
    new letter falls — 0 below every base letter, 1 between two, 2 above all, 3 two at once (one between, one outside); with
    seed % 8 >= 4 one more letter lives only in a query gene shorter than k.  At most 12 letters, k <= 8: always exact."""
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(POOL, np.uint8)
    mid = int(rng.integers(1, len(pool) - 1))                          # the letter kept OUT of the base: something below and above it stays
    between = bytes([pool[mid]])
    lower = rng.choice(pool[:mid], int(rng.integers(1, min(mid, 4) + 1)), replace=False)
    upper = rng.choice(pool[mid + 1:], int(rng.integers(1, min(len(pool) - mid - 1, 4) + 1)), replace=False)
    alphabet = bytes(sorted(int(x) for x in np.concatenate([lower, upper])))
    k = int(rng.integers(2, 9))
    where = ("below", "between", "above", "two")[seed % 4]
    outside_low, outside_high = bytes([BELOW[int(rng.integers(0, len(BELOW)))]]), bytes([ABOVE[int(rng.integers(0, len(ABOVE)))]])
    letters = {"below": outside_low, "between": between, "above": outside_high,
               "two": between + (outside_low if rng.random() < 0.5 else outside_high)}[where]
    genomes = int(rng.integers(3, 5))
    fam = family_genes(alphabet, genomes + 1, int(rng.integers(4, 9)), k + 2, k + 30, seed)
    fam[0][0] = alphabet + fam[0][0]                                   # every base letter is there, whatever the ancestor drew
    base = pack([g for gs in fam[:genomes] for g in gs], [i for i, gs in enumerate(fam[:genomes]) for _ in gs])
    q = [with_letters(g, letters, seed * 7 + j, every=8) if j % 2 == 0 else g for j, g in enumerate(fam[genomes])]
    for j, letter in enumerate(letters):                               # every new letter at least once inside a k-mer
        q[j % len(q)] = q[j % len(q)][:1] + bytes([letter]) + q[j % len(q)][2:]
    short_letter = b""
    if seed % 8 >= 4:
        short_letter = SHORT_ONLY
        q.insert(int(rng.integers(0, len(q) + 1)), (SHORT_ONLY * 8)[:int(rng.integers(1, k))])
    res, off, _ = pack(q, [0] * len(q))
    return dict(k=k, base=base, query=(res, off), query_genes=q, where=where, letters=letters, short_letter=short_letter, alphabet=alphabet)


def classify(case):
    """What the library must answer with the option on, from the inputs alone: 'supported', or 'inexact'."""
    k = case["k"]
    letters = len(set(case["base"][0].tolist()) | set(case["query"][0].tolist()))
    return "supported" if letters ** k < 1 << 64 and len(set(case["base"][0].tolist())) ** k < 1 << 64 else "inexact"
