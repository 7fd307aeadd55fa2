"""The multi-GPU entry points (pdl_dist_*) at the boundary where another process's bytes enter the library: called out of
order, with bad arguments, and with range tuples or cells a peer could not have made.

Every other suite drives them through LocalRanks or DistributedPangenes: the right calls, in the right order, on well-formed
data.  Here the calls are made one by one (``Ranks`` below: the steps of ``LocalRanks.preprocess`` / ``score_all``, W contexts in
one process on one device), one of them is made wrong, and every case asserts TWO things: the wrong call is refused with the
code and the message the header promises, and the same contexts then carry the protocol to its end and give the fixture's
Scores blocks bit for bit, every genome from its owner, with "Total cost" and every "Genome g cost".  A refusal that damages
the run is as bad as no refusal.

    a. call order          every entry point in every state that must refuse it                        PDL_ERR_STATE
    b. arguments           world / rank, alignments, NULLs, record counts that do not add up          PDL_ERR_ARGUMENT
    c. range tuples        a received key or range no peer could have made (counted on the device
                           BEFORE the gene sort, whose digits promise genes below N)                    PDL_ERR_ARGUMENT
    d. cells               a received cell no peer could have made; a cell for a rank without rows    PDL_ERR_ARGUMENT
    e. single-GPU calls    that a multi-GPU context refuses                                            PDL_ERR_STATE
    f. re-use              multi-GPU, single-GPU, multi-GPU again; owners' flow after senders' flow

Where a refused call leaves the build or the pass to be begun again, the case says so and does that."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

NAME = "synth_5x60x80_k3"                 # takes the senders' flow at W = 2 (tests/test_gpu_dist.py asserts it)
NO_SENDER = ("q1_fold", 3)                # ... and this one, over this many ranks, does not: a last run of ONE record
NO_ROWS = ("readme4_k2", 5)               # two genomes over five ranks: three ranks without a row


@pytest.fixture(scope="module")
def sets():
    """name -> (residues, offsets, genome_of, k, fixture, the three device tensors): loaded once, never written."""
    import torch
    dev = torch.device("cuda", 0)
    out = {}
    for name in (NAME, NO_SENDER[0], NO_ROWS[0]):
        res, off, gen, k, fx = H.load_small(name)
        t_res = torch.from_numpy(np.concatenate([res, np.zeros((-len(res)) % 16 + 16, np.uint8)])).to(dev)
        t_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        t_gen = torch.from_numpy(gen.astype(np.int32)).to(dev)
        out[name] = (res, off, gen, k, fx, (t_res, t_off, t_gen))
    return out


class Ranks:
    """W contexts driven step by step.  The good calls go through PangeneNative (they raise when refused); a call that is MEANT to
    be refused goes through ``refused``: the C ABI itself, its return code and pdl_last_error."""

    def __init__(self, sets, name=NAME, world=2):
        import torch
        from pandelos_amd.pangene_native import PangeneNative
        self.res, self.off, self.gen, self.k, self.fx, self.t = sets[name]
        self.name, self.W, self.N = name, world, len(self.gen)
        self.G = int(self.fx["genomes"])
        self.dev = torch.device("cuda", 0)
        self.nats = [PangeneNative.open() for _ in range(world)]
        self.lib = self.nats[0]._lib
        self.dummy = torch.zeros(16, dtype=torch.int64, device=self.dev)       # aligned device memory for calls that must not get as far as reading it
        self.runs = self.made = self.full = self.tuples = self.boxes = self.inboxes = None
        self.total = 0

    def close(self):
        for n in self.nats:
            n.close()

    # ---- the steps, as LocalRanks makes them ---------------------------------------------------------------------------
    def begin(self):
        t_res, t_off, t_gen = self.t
        self.made = self.full = self.tuples = self.boxes = self.inboxes = None
        self.runs = [n.dist_preprocess_begin(self.k, t_res.data_ptr(), t_off.data_ptr(), t_gen.data_ptr(), self.N, len(self.res), self.W, r, keepalive=self.t)
                     for r, n in enumerate(self.nats)]
        self.run_records = np.array([rec for _, rec, _ in self.runs], np.uint64)
        self.total = int(self.run_records.sum())
        self.weights = np.sum([n.run_weights for n in self.nats], axis=0).astype(np.uint64)
        self.costs = np.sum([n.run_costs for n in self.nats], axis=0).astype(np.uint64)

    def ranges(self):
        """-> True: every rank built and filed its tuples; False: every rank said "not available" (the owners build the lists)."""
        made = [n.dist_preprocess_ranges(self.run_records, self.weights, self.costs) for n in self.nats]
        assert all(m is None for m in made) or all(m is not None for m in made), "ranks disagree on who builds the range lists"
        self.made = None if made[0] is None else made
        return self.made is not None

    def gather(self):
        """Every rank's copy of every run (in the senders' flow AFTER ranges: it takes the head bits out of the runs)."""
        import torch
        offs = np.concatenate([[0], np.cumsum(self.run_records.astype(np.int64))])
        self.full = []
        for n in self.nats:
            full = torch.empty(max(self.total, 1), dtype=torch.int64, device=self.dev)
            for p, (ptr, rec, _) in enumerate(self.runs):
                if rec:
                    n.copy_device(full.data_ptr() + int(offs[p]) * 8, ptr, rec * 8)
            self.full.append(full)

    def exchange_tuples(self):
        import torch
        cmat = np.stack([m[2] for m in self.made])                # [src][dst]
        self.sums = np.sum([m[3] for m in self.made], axis=0).astype(np.uint64)
        self.tuples = []
        for d, n in enumerate(self.nats):
            n_in = int(cmat[:, d].sum())
            rk = torch.empty(max(n_in, 1), dtype=torch.int32, device=self.dev)
            rr = torch.empty(max(n_in, 1), dtype=torch.int64, device=self.dev)
            at = 0
            for s in range(self.W):
                cnt = int(cmat[s, d])
                if cnt:
                    o = int(cmat[s, :d].sum())
                    n.copy_device(rk.data_ptr() + at * 4, self.made[s][0] + o * 4, cnt * 4)
                    n.copy_device(rr.data_ptr() + at * 8, self.made[s][1] + o * 8, cnt * 8)
                    at += cnt
            self.tuples.append((rk, rr, n_in))

    def finish_ranges(self, only=None):
        for r, n in enumerate(self.nats):
            if only is None or r in only:
                rk, rr, n_in = self.tuples[r]
                n.dist_preprocess_finish_ranges(self.full[r].data_ptr(), self.total, rk.data_ptr(), rr.data_ptr(), n_in, self.sums, keepalive=(self.full[r], rk, rr))

    def finish(self):
        for n, full in zip(self.nats, self.full):
            n.dist_preprocess_finish(full.data_ptr(), self.total, genome_weights=self.weights, keepalive=full)

    def after_begin(self, sender=True):
        """From a begun build to a finished one -> True when it went the senders' way."""
        if sender and self.made is None:
            sender = self.ranges()
        sender = sender and self.made is not None
        if self.full is None:
            self.gather()
        if sender:
            if self.tuples is None:
                self.exchange_tuples()
            self.finish_ranges()
        else:
            self.finish()
        return sender

    def build(self, sender=True):
        self.begin()
        return self.after_begin(sender)

    def score_begin(self):
        self.inboxes = None
        self.boxes = [n.dist_score_begin(self.W) for n in self.nats]

    def exchange_cells(self):
        import torch
        from pandelos_amd import _lib
        cmat = np.stack([c for _, c in self.boxes])
        self.inboxes = []
        for d, n in enumerate(self.nats):
            n_in = int(cmat[:, d].sum())
            recv = torch.empty((max(n_in, 1), 6), dtype=torch.int32, device=self.dev)
            at = 0
            for s in range(self.W):
                cnt = int(cmat[s, d])
                if cnt:
                    o = int(cmat[s, :d].sum())
                    n.copy_device(recv.data_ptr() + at * _lib.DIST_CELL_BYTES, self.boxes[s][0] + o * _lib.DIST_CELL_BYTES, cnt * _lib.DIST_CELL_BYTES)
                    at += cnt
            self.inboxes.append((recv, n_in))

    def score_finish(self, only=None):
        for r, n in enumerate(self.nats):
            if only is None or r in only:
                recv, n_in = self.inboxes[r]
                n.dist_score_finish(recv.data_ptr(), n_in, keepalive=recv)

    def score(self):
        self.score_begin()
        self.exchange_cells()
        self.score_finish()

    # ---- the reference for "still correct": the fixture's own blocks -------------------------------------------------------
    def check(self, label):
        fx = self.fx
        owner = self.nats[0].dist_genome_owner()
        for n in self.nats[1:]:
            assert np.array_equal(n.dist_genome_owner(), owner), f"{label}: ranks disagree on the genome deal"
        assert all(int(x) < self.W for x in owner)
        assert sum(int(n.cost.total_cost) for n in self.nats) == int(fx["total_cost"]), f"{label}: total cost"
        for n in self.nats:
            assert (n.cost.sequences, n.cost.genomes, n.cost.dictionary_records) == (int(fx["sequences"]), self.G, self.total), label
        assert [self.nats[int(owner[g])].genome_cost(g) for g in range(self.G)] == [int(x) for x in fx["genome_cost"]], f"{label}: genome costs"
        H.assert_scores_equal_fixture(lambda g: self.nats[int(owner[g])].generate_scores_part(g).as_dict(), fx, self.G, f"{self.name} W={self.W} {label}")
        return owner

    def check_single(self, label):
        """... and the same from every context on its own, after a plain pdl_preprocess + pdl_score_all."""
        for r, n in enumerate(self.nats):
            assert int(n.cost.total_cost) == int(self.fx["total_cost"]), f"{label}: total cost, context {r}"
            assert [n.genome_cost(g) for g in range(self.G)] == [int(x) for x in self.fx["genome_cost"]], f"{label}: genome costs, context {r}"
            H.assert_scores_equal_fixture(lambda g: n.generate_scores_part(g).as_dict(), self.fx, self.G, f"{self.name} {label} context {r}")

    # ---- one entry point, through the C ABI, with arguments that are right wherever the protocol has got far enough to have them ----
    def refused(self, entry, r, **wrong):
        """-> (return code, message) of ``entry`` on rank r; ``wrong`` replaces single arguments."""
        from pandelos_amd import _lib
        nat = self.nats[r]
        t_res, t_off, t_gen = self.t
        full = self.full[r].data_ptr() if self.full else self.dummy.data_ptr()
        total = self.total if self.full else 1
        if entry == "pdl_dist_preprocess_begin":
            a = dict(res=t_res.data_ptr(), off=t_off.data_ptr(), gen=t_gen.data_ptr(), world=self.W, rank=r)
            a.update(wrong)
            rc = self.lib.pdl_dist_preprocess_begin(nat._ctx, a["res"], a["off"], a["gen"], self.N, len(self.res), self.k, a["world"], a["rank"], C.byref(_lib.PdlDistSlice()))
        elif entry == "pdl_dist_preprocess_finish":
            a = dict(full=full, total=total)
            a.update(wrong)
            w = self.weights if self.runs else np.zeros(self.G, np.uint64)
            rc = self.lib.pdl_dist_preprocess_finish(nat._ctx, a["full"], a["total"], w.ctypes.data, C.byref(_lib.PdlCost()))
        elif entry == "pdl_dist_preprocess_ranges":
            rr = (self.run_records if self.runs else np.ones(self.W, np.uint64)).copy()
            if "own_records" in wrong:
                rr[r] = wrong["own_records"]
            w, cs = (self.weights, self.costs) if self.runs else (np.zeros(self.G, np.uint64), np.zeros(self.G, np.uint64))
            rc = self.lib.pdl_dist_preprocess_ranges(nat._ctx, rr.ctypes.data, w.ctypes.data, cs.ctypes.data, C.byref(_lib.PdlDistRanges()))
        elif entry == "pdl_dist_preprocess_finish_ranges":
            if self.tuples:
                rk, rr, n_in = self.tuples[r]
                a = dict(full=full, total=total, keys=rk.data_ptr(), ranges=rr.data_ptr(), n=n_in, sums=self.sums.ctypes.data)
            else:                                                 # (no tuple to hand over: the state is what must refuse the call)
                a = dict(full=full, total=total, keys=None, ranges=None, n=0, sums=np.zeros(3, np.uint64).ctypes.data)
            a.update(wrong)
            rc = self.lib.pdl_dist_preprocess_finish_ranges(nat._ctx, a["full"], a["total"], a["keys"], a["ranges"], a["n"], a["sums"], C.byref(_lib.PdlCost()))
        elif entry == "pdl_dist_genome_owner":
            rc = self.lib.pdl_dist_genome_owner(nat._ctx, np.zeros(self.G, np.uint32).ctypes.data)
        elif entry == "pdl_dist_score_begin":
            rc = self.lib.pdl_dist_score_begin(nat._ctx, C.byref(_lib.PdlDistOutbox()))
        elif entry == "pdl_dist_score_finish":
            recv, n_in = self.inboxes[r] if self.inboxes else (self.dummy, 0)
            rc = self.lib.pdl_dist_score_finish(nat._ctx, recv.data_ptr(), n_in)
        elif entry == "pdl_score_all":
            rc = self.lib.pdl_score_all(nat._ctx)
        elif entry == "pdl_set_genome_shard":
            rc = self.lib.pdl_set_genome_shard(nat._ctx, np.array([0], np.uint32).ctypes.data, 1)
        elif entry == "pdl_get_dictionary":
            u = max(self.total, 1)
            rc = self.lib.pdl_get_dictionary(nat._ctx, np.zeros(u, np.uint64).ctypes.data, np.zeros(u, np.uint32).ctypes.data, np.zeros(u, np.uint32).ctypes.data)
        else:
            assert entry == "pdl_sequence_costs"
            rc = self.lib.pdl_sequence_costs(nat._ctx, np.zeros(self.N, np.uint64).ctypes.data, np.zeros(self.N, np.uint32).ctypes.data)
        return rc, self.lib.pdl_last_error(nat._ctx).decode()

    def refused_everywhere(self, entry, code, **wrong):
        """Every rank makes the wrong call (a driver's mistake is every rank's mistake) -> the messages."""
        msgs = []
        for r in range(self.W):
            rc, msg = self.refused(entry, r, **wrong)
            print(f"{entry} rank {r} {wrong or ''}: rc={rc} {msg!r}")
            assert rc == code, (entry, r, wrong, rc, msg)
            msgs.append(msg)
        return msgs


def _id(text):
    """A test id the shell does not have to quote."""
    out = "".join(ch if ch.isalnum() else "_" for ch in text.replace("<<", "shl").replace("|", "or").replace("==", "eq").replace("=", "eq"))
    while "__" in out:
        out = out.replace("__", "_")
    return out.strip("_")


def _names(msg, entry):
    """The message names the call: its name, not merely a longer one's that begins alike (…_finish / …_finish_ranges)."""
    at = msg.find(entry)
    while at >= 0:
        if not msg[at + len(entry):at + len(entry) + 1] == "_":
            return True
        at = msg.find(entry, at + 1)
    return False


# ---- a. call order ------------------------------------------------------------------------------------------------------
# state -> how the contexts get there (on a fresh Ranks) and how they go on from there to a finished build
def _to_fresh(rk):
    pass


def _to_plain(rk):
    for n in rk.nats:
        n.preprocess(rk.k, rk.res, rk.off, rk.gen)


def _to_begun(rk):
    rk.begin()


def _to_ranged(rk):
    rk.begin()
    assert rk.ranges(), "this fixture takes the senders' flow"


def _to_unavailable(rk):
    rk.begin()
    assert not rk.ranges(), "this fixture over this many ranks leaves the range lists to the owners"


def _to_finished(rk):
    assert rk.build(), "this fixture takes the senders' flow"


def _to_scored(rk):
    _to_finished(rk)
    rk.score()


STATES = {
    # state: (set-up, the right continuation up to a finished build, (fixture, world))
    "fresh context": (_to_fresh, lambda rk: rk.build(), (NAME, 2)),
    "after a plain pdl_preprocess": (_to_plain, lambda rk: rk.build(), (NAME, 2)),            # (begin: a single-GPU dictionary is no run)
    "after begin, without a ranges call": (_to_begun, lambda rk: rk.after_begin(), (NAME, 2)),
    "after ranges said available": (_to_ranged, lambda rk: rk.after_begin(), (NAME, 2)),      # gather, the tuples, finish_ranges: the run is as ranges left it
    "after ranges said not available": (_to_unavailable, lambda rk: rk.after_begin(), NO_SENDER),   # gather, finish: the owners' flow
    "after a completed finish": (_to_finished, lambda rk: None, (NAME, 2)),
    "after a completed score_finish": (_to_scored, None, (NAME, 2)),                            # (nothing to go on with: the blocks are there)
}
ORDER = [
    ("pdl_dist_preprocess_finish", "fresh context"),
    ("pdl_dist_preprocess_finish", "after a plain pdl_preprocess"),
    ("pdl_dist_preprocess_finish", "after ranges said available"),
    ("pdl_dist_preprocess_finish", "after a completed finish"),
    ("pdl_dist_preprocess_ranges", "fresh context"),
    ("pdl_dist_preprocess_ranges", "after a plain pdl_preprocess"),
    ("pdl_dist_preprocess_ranges", "after ranges said available"),                              # a second time: a driver's retry
    ("pdl_dist_preprocess_ranges", "after a completed finish"),
    ("pdl_dist_preprocess_finish_ranges", "fresh context"),
    ("pdl_dist_preprocess_finish_ranges", "after a plain pdl_preprocess"),
    ("pdl_dist_preprocess_finish_ranges", "after begin, without a ranges call"),
    ("pdl_dist_preprocess_finish_ranges", "after ranges said not available"),
    ("pdl_dist_preprocess_finish_ranges", "after a completed finish"),
    ("pdl_dist_genome_owner", "after begin, without a ranges call"),
    ("pdl_dist_score_begin", "after begin, without a ranges call"),
    ("pdl_dist_score_finish", "after a completed finish"),                                      # without a score_begin
    ("pdl_dist_score_finish", "after a completed score_finish"),                                # a second time
]


@pytest.mark.parametrize("entry,state", ORDER, ids=[f"{e[4:]}-{_id(s)}" for e, s in ORDER])
def test_a_call_out_of_order_is_refused_and_the_protocol_goes_on(sets, entry, state):
    from pandelos_amd import _lib
    setup, go_on, (name, world) = STATES[state]
    rk = Ranks(sets, name, world)
    try:
        setup(rk)
        for msg in rk.refused_everywhere(entry, _lib.PDL_ERR_STATE):
            assert _names(msg, entry), (entry, state, msg)
        if go_on is not None:
            sender = go_on(rk)
            assert sender is None or sender == (name == NAME), "the flow the fixture takes"
            rk.score()
        rk.check(f"{entry} {state}")
    finally:
        rk.close()


# ---- b. arguments -------------------------------------------------------------------------------------------------------
# (entry point, the one wrong argument as a function of the Ranks and the rank, the state it is called in, what the message says)
def _own_run_minus_one(rk, r):
    assert rk.runs[r][1] > 0
    return dict(total=rk.runs[r][1] - 1)


ARGUMENTS = {
    "world 0": ("pdl_dist_preprocess_begin", lambda rk, r: dict(world=0, rank=0), "fresh", "rank"),
    "rank == world": ("pdl_dist_preprocess_begin", lambda rk, r: dict(rank=rk.W), "fresh", "rank"),
    "world 65": ("pdl_dist_preprocess_begin", lambda rk, r: dict(world=65), "fresh", "64"),
    "d_residues off 16-byte alignment": ("pdl_dist_preprocess_begin", lambda rk, r: dict(res=rk.t[0].data_ptr() + 8), "fresh", "16-byte"),
    "NULL d_offsets": ("pdl_dist_preprocess_begin", lambda rk, r: dict(off=None), "fresh", "null"),
    "finish: dictionary off 8-byte alignment": ("pdl_dist_preprocess_finish", lambda rk, r: dict(full=rk.full[r].data_ptr() + 4), "gathered", "8-byte"),
    "finish: total_records below the own run": ("pdl_dist_preprocess_finish", _own_run_minus_one, "gathered", "smaller than this rank's run"),
    "ranges: run_records[rank] is not the run's size": ("pdl_dist_preprocess_ranges", lambda rk, r: dict(own_records=int(rk.run_records[r]) + 1), "begun", "run_records"),
    "finish_ranges: dictionary off 8-byte alignment": ("pdl_dist_preprocess_finish_ranges", lambda rk, r: dict(full=rk.full[r].data_ptr() + 4), "exchanged", "8-byte"),
    "finish_ranges: total_records is not the runs' sum": ("pdl_dist_preprocess_finish_ranges", lambda rk, r: dict(total=rk.total + 1), "exchanged", "add up"),
    "finish_ranges: keys off 4-byte alignment": ("pdl_dist_preprocess_finish_ranges", lambda rk, r: dict(keys=rk.tuples[r][0].data_ptr() + 2), "exchanged", "aligned"),
    "finish_ranges: ranges off 8-byte alignment": ("pdl_dist_preprocess_finish_ranges", lambda rk, r: dict(ranges=rk.tuples[r][1].data_ptr() + 4), "exchanged", "aligned"),
    "finish_ranges: NULL counter_sums": ("pdl_dist_preprocess_finish_ranges", lambda rk, r: dict(sums=None), "exchanged", None),     # (refused before the context is looked at: no message)
}


@pytest.mark.parametrize("what", list(ARGUMENTS), ids=[_id(w) for w in ARGUMENTS])
def test_a_bad_argument_is_refused_and_the_build_completes(sets, what):
    from pandelos_amd import _lib
    entry, wrong, state, says = ARGUMENTS[what]
    rk = Ranks(sets)
    try:
        sender = state in ("begun", "exchanged")
        if state != "fresh":
            rk.begin()
        if state == "exchanged":
            assert rk.ranges()
        if state in ("gathered", "exchanged"):
            rk.gather()
        if state == "exchanged":
            rk.exchange_tuples()
        for r in range(rk.W):
            rc, msg = rk.refused(entry, r, **wrong(rk, r))
            print(f"{what} rank {r}: rc={rc} {msg!r}")
            assert rc == _lib.PDL_ERR_ARGUMENT, (what, r, rc, msg)
            assert says is None or says in msg, (what, msg)
        if state == "fresh":
            assert rk.build()
        else:
            assert rk.after_begin(sender) == sender
        rk.score()
        rk.check(what)
    finally:
        rk.close()


# ---- c. what peers send: range tuples -------------------------------------------------------------------------------------
def _i64(v):
    """An unsigned 64-bit pattern as the signed value an int64 tensor takes."""
    return v - (1 << 64) if v >> 63 else v


TUPLES = {
    # what: (the received keys to change -> their new values, or None to change a range instead, bad tuples)
    "gene = N": lambda rk, r, key: ((r << 24) | rk.N, 1),                       # (N is no power of two: no bit above the digits the gene sort covers)
    "gene = 1 << 21 | 5": lambda rk, r, key: ((r << 24) | (1 << 21) | 5, 1),       # below the 22-bit packing limit, far above N
    "owner byte of another rank": lambda rk, r, key: ((key & 0xffffff) | (((r + 1) % rk.W) << 24), 1),
    "three keys with gene = N": lambda rk, r, key: ((r << 24) | rk.N, 3),
}


def _refused_tuples_then_a_fresh_build(rk, r, bad, label):
    from pandelos_amd import _lib
    other = [p for p in range(rk.W) if p != r]
    rk.finish_ranges(only=other)                                      # the peers got well-formed tuples: they finish
    rc, msg = rk.refused("pdl_dist_preprocess_finish_ranges", r)
    print(f"{label}: rc={rc} {msg!r}")
    assert rc == _lib.PDL_ERR_ARGUMENT, (label, rc, msg)
    assert _names(msg, "pdl_dist_preprocess_finish_ranges") and f"{bad} of the {rk.tuples[r][2]} received" in msg, (label, msg)
    assert rk.build(), "a fresh begin on every rank"                  # (the message says so: begin again)
    rk.score()
    rk.check(label)


@pytest.mark.parametrize("what", list(TUPLES), ids=[_id(w) for w in TUPLES])
def test_a_key_no_peer_could_have_sent_is_counted_before_the_sort(sets, what):
    import torch
    assert sets[NAME][2].size & (sets[NAME][2].size - 1), "N must be no power of two for 'gene = N' to stay below the sorted digits"
    rk = Ranks(sets)
    try:
        rk.begin()
        assert rk.ranges()
        rk.gather()
        rk.exchange_tuples()
        r = 1
        keys, _, n_in = rk.tuples[r]
        assert n_in >= 16
        at = n_in // 2
        new, bad = TUPLES[what](rk, r, int(keys[at]) & 0xffffffff)
        for i in range(bad):
            keys[at + 2 * i] = int(new)
        torch.cuda.synchronize()
        _refused_tuples_then_a_fresh_build(rk, r, bad, what)
    finally:
        rk.close()


def test_a_key_for_a_gene_of_another_ranks_genome_is_refused(sets):
    """Below N and with this rank's owner byte, but the gene's genome was dealt to a peer: the range list it would open belongs
    to no row of this rank."""
    import torch
    rk = Ranks(sets)
    try:
        rk.begin()
        assert rk.ranges()
        rk.gather()
        rk.exchange_tuples()
        r = 0
        keys, _, n_in = rk.tuples[r]
        foreign = int(rk.tuples[1][0][0]) & 0xffffff                  # a gene the peer received tuples for: one of ITS genomes'
        assert n_in >= 1 and rk.tuples[1][2] >= 1
        keys[n_in - 1] = (r << 24) | foreign
        torch.cuda.synchronize()
        _refused_tuples_then_a_fresh_build(rk, r, 1, "a gene of a peer's genome")
    finally:
        rk.close()


def test_a_range_that_reaches_past_the_dictionary_is_refused(sets):
    import torch
    rk = Ranks(sets)
    try:
        rk.begin()
        assert rk.ranges()
        rk.gather()
        rk.exchange_tuples()
        r = 1
        _, rngs, n_in = rk.tuples[r]
        v = int(rngs[0]) & ((1 << 64) - 1)
        postings = (v >> 32) & 0x3fffff
        assert postings >= 1
        rngs[0] = _i64((v & ~0xffffffff) | (rk.total - postings + 1))      # first posting: one too far for the postings to fit
        torch.cuda.synchronize()
        _refused_tuples_then_a_fresh_build(rk, r, 1, "a range past the dictionary")
    finally:
        rk.close()


def test_tuples_for_a_rank_that_owns_no_gene_are_refused(sets):
    """Six ranks, five genomes: the last rank owns no genome, nobody files a tuple for it.  Handed one all the same it refuses, as
    a rank without rows refuses cells."""
    import torch
    from pandelos_amd import _lib
    rk = Ranks(sets, NAME, 6)
    try:
        rk.begin()
        assert rk.ranges()
        rk.gather()
        rk.exchange_tuples()
        idle = [r for r in range(rk.W) if rk.tuples[r][2] == 0]
        assert idle == [5], [t[2] for t in rk.tuples]
        r = idle[0]
        donor = rk.tuples[0]
        rk.tuples[r] = (((donor[0][:1] & 0xffffff) | (r << 24)).contiguous(), donor[1][:1].clone(), 1)
        torch.cuda.synchronize()
        rk.finish_ranges(only=range(5))
        rc, msg = rk.refused("pdl_dist_preprocess_finish_ranges", r)
        print(f"rc={rc} {msg!r}")
        assert rc == _lib.PDL_ERR_ARGUMENT and _names(msg, "pdl_dist_preprocess_finish_ranges") and "owns no gene" in msg, (rc, msg)
        assert rk.build()
        rk.score()
        owner = rk.check("tuples for a rank without genes")
        assert r not in set(int(x) for x in owner)
    finally:
        rk.close()


# ---- d. what peers send: cells ----------------------------------------------------------------------------------------------
ROW, COLUMN = 3, 4                                                    # pdl_dist_cell as six 32-bit words: score, perc, tr_perc, row, column, first_group
CELLS = {
    "row = N": lambda rk, r, owner: (ROW, rk.N),
    "column = N": lambda rk, r, owner: (COLUMN, rk.N),
    "column of a genome this rank does not own": lambda rk, r, owner: (COLUMN, int(np.nonzero(owner[rk.gen] != r)[0][0])),
}


@pytest.mark.parametrize("what", list(CELLS), ids=[_id(w) for w in CELLS])
def test_a_cell_no_peer_could_have_sent_is_refused_and_the_pass_repeats(sets, what):
    """One cell of the inbox is changed into one that cannot be; a SECOND, well-formed one gets a score above every real one,
    which the refused call folds into the maxima of its row.  The pass begun again must show neither: the error count does not
    stick, and the maxima are the fixture's."""
    import torch
    from pandelos_amd import _lib
    rk = Ranks(sets)
    try:
        assert rk.build()
        owner = rk.nats[0].dist_genome_owner()
        rk.score_begin()
        rk.exchange_cells()
        r = 1
        inbox, n_in = rk.inboxes[r]
        assert n_in >= 4
        word, value = CELLS[what](rk, r, owner)
        inbox[n_in // 2, word] = value
        inbox[0, 0] = int(np.float32(3.0e9).view(np.int32))
        torch.cuda.synchronize()
        rk.score_finish(only=[0])
        rc, msg = rk.refused("pdl_dist_score_finish", r)
        print(f"{what}: rc={rc} {msg!r}")
        assert rc == _lib.PDL_ERR_ARGUMENT and _names(msg, "pdl_dist_score_finish") and "1 received cells" in msg, (what, rc, msg)
        # the refused pass is over: another finish is a call out of order, with or without a better inbox
        rc, msg = rk.refused("pdl_dist_score_finish", r)
        assert rc == _lib.PDL_ERR_STATE and _names(msg, "pdl_dist_score_finish"), (rc, msg)
        rk.score()                                                    # the same ranks: begin, the right exchange, finish
        rk.check(what)
    finally:
        rk.close()


def test_a_cell_for_a_rank_without_rows_is_refused(sets):
    """Five ranks, two genomes: three ranks own none and have no row to file a cell under."""
    import torch
    from pandelos_amd import _lib
    name, world = NO_ROWS
    rk = Ranks(sets, name, world)
    try:
        rk.build()
        owner = rk.nats[0].dist_genome_owner()
        idle = [r for r in range(world) if r not in set(int(x) for x in owner)]
        assert len(idle) == 3
        r = idle[0]
        rk.score_begin()
        rk.exchange_cells()
        assert rk.inboxes[r][1] == 0
        donor = next(box for box, n in rk.inboxes if n)
        rk.inboxes[r] = (donor[:1].clone(), 1)
        torch.cuda.synchronize()
        rk.score_finish(only=[p for p in range(world) if p != r])
        rc, msg = rk.refused("pdl_dist_score_finish", r)
        print(f"rc={rc} {msg!r}")
        assert rc == _lib.PDL_ERR_ARGUMENT and "without rows" in msg, (rc, msg)
        rk.inboxes[r] = (rk.dummy, 0)                                 # nothing of the rank was touched: its pass still stands, and ends on the right inbox
        rk.score_finish(only=[r])
        rk.check("a cell for a rank without rows")
        rk.score()                                                    # ... and every rank serves the next pass
        rk.check("a cell for a rank without rows, next pass")
    finally:
        rk.close()


# ---- e. what a multi-GPU context refuses besides the incremental entry points ---------------------------------------------------
@pytest.mark.parametrize("entry", ["pdl_score_all", "pdl_set_genome_shard", "pdl_get_dictionary", "pdl_sequence_costs"])
def test_single_gpu_calls_are_refused_by_a_multi_gpu_context(sets, entry):
    from pandelos_amd import _lib
    rk = Ranks(sets)
    try:
        assert rk.build()                                             # (pdl_sequence_costs: refused after the senders' flow, which keeps no per-gene costs)
        rk.refused_everywhere(entry, _lib.PDL_ERR_STATE)
        rk.score()
        if entry != "pdl_score_all":                                  # (on a scored context pdl_score_all has nothing to do and says OK)
            rk.refused_everywhere(entry, _lib.PDL_ERR_STATE)
        rk.check(entry)
    finally:
        rk.close()


# ---- f. re-use ----------------------------------------------------------------------------------------------------------------
def test_the_same_contexts_serve_multi_gpu_and_single_gpu_builds_in_turn(sets):
    rk = Ranks(sets)
    try:
        assert rk.build()
        rk.score()
        rk.check("multi-GPU, senders' flow")
        for n in rk.nats:                                             # a plain build on a context that was a rank: the deal does not carry over
            n.preprocess(rk.k, rk.res, rk.off, rk.gen)
            n.score_all()
        rk.check_single("single-GPU after multi-GPU")
        assert rk.build()
        rk.score()
        rk.check("multi-GPU after single-GPU")
        assert not rk.build(sender=False)                             # the owners' flow straight after the senders'
        rk.score()
        rk.check("owners' flow after senders' flow")
        assert rk.build()                                             # ... and back
        rk.score()
        rk.check("senders' flow after owners' flow")
    finally:
        rk.close()
