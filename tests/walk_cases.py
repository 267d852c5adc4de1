"""Seeded random walks over the C ABI on ONE context (no GPU needed here): the pools of databases, read sets and
parameter sets, the step generators, and a model of what every call must return or refuse after the steps before it.

tests/test_gpu_walk.py drives an Engine through a step list and holds every result to the CPU oracle for the inputs
and parameters in hand at that step; tests/test_walk_cases.py checks, without a device, that the committed walks visit
what they are meant to visit.  `python tests/fuzz_gpu.py walk LO HI` runs further seeds.

A step is a plain tuple, so that a failing walk prints as data:
    ("db", name, "ascii" | "packed")                    ("reads", name, loader)       ("bad_reads",)
    ("index", params)      ("part", 0 | 1)              ("env", variable, value | None)
    ("pass", params, apply_mmtol, "host" | "dev" | "packed" | "compact", times)
    ("replay", apply_mmtol)   ("probes",)   ("gtext",)   ("rtext",)   ("order",)   ("rhits",)   ("text", a, b)
    ("side",)   ("side_text", which, a, b)
A streamed load (loader "stream") is always followed by its pass: the library borrows the host buffer until then.

The model (class Model) is written from include/muscato_hip.h and the two tables of DESIGN.md 19: which generation a
call bumps and what each derived thing needs to be current.  Which index and kernel a pass takes (Model.path) follows
DESIGN.md 4 and 14: context buckets when the run fits them, 120 bases or 200, the two-kernel path otherwise, a
resident window-start index keeping its layout unless MUSC_INDEX names another one.  Two readings of the header that
the model commits to: a musc_maxmatches_apply that "changes nothing" (no block above MaxMatches and apply_mmtol = 0,
or an empty list) leaves the list that of the pass and the order standing; musc_results_text and musc_results_hits
serve an order across a later pass (they need reads, database and texts unchanged), the side stage does not.
"""
from __future__ import annotations

import functools
import random
from typing import Dict, List, Optional, Sequence, Tuple

from oracle import muscato_oracle as orc

import cases
import maxmatches_cases as mc

PART_BASES = 4500  # ("part", 1): two to three partitions on every database of the pool
KNOBS = ("MUSC_INDEX", "MUSC_MATCH", "MUSC_GRAPH", "MUSC_BATCH_READS", "MUSC_CONTEXT")
ENV_VALUES = {"MUSC_INDEX": (None, "classic", "lines"), "MUSC_MATCH": (None, "dma"), "MUSC_GRAPH": (None, "1"),
              "MUSC_BATCH_READS": (None, "64"), "MUSC_CONTEXT": (None, "wide", "narrow")}
LOADERS = ("ascii", "packed", "packed32", "stream", "sort_unique", "fastq")
CLASSES = ("t120", "g", "twide", "tx_reads", "tx_db", "classic", "lines", "rstride", "part")
SIDE = ("nonmatch", "genestats", "readstats")

# refusals, with the library's code (the texts are those tests/test_gpu_ctx_state.py and test_gpu_side.py pin)
E_NO_READS = (4, "no reads loaded")
E_BAD_LOAD = (2, r"read offsets\[0\] must be 0")
E_NOT_PASS_LIST = (2, "resident tuple list is not that of a pass over the reads and the database in hand")
E_NOT_MATCH_LIST = (2, r"resident tuple list is not that of a musc_match\* over the reads and the database in hand")
E_PASS_HAD_MMTOL = (2, "the last pass ran with apply_mmtol = 1")
E_NO_GENE_TEXT = (2, "no gene text")
E_NO_ORDER = (2, "no ordered list")
E_PASS_AFTER = (2, "a pass ran after")
E_NO_READ_TEXT = (2, "no read text")
E_NOT_PREPARED = (2, "nothing prepared")


# ------------------------------------------------------------------------------------------------------- pools

def _distinct(make, n):
    out = set()
    while len(out) < n:
        out.add(make())
    return sorted(out)


@functools.lru_cache(maxsize=None)
def pools():
    """-> (databases, read sets, parameter sets), each a dict by name."""
    rng = random.Random(1906)
    rnd = lambda n: cases.rand_seq(rng, n, b"ACGT")
    motif = rnd(200)
    base = [rnd(300) for _ in range(30)]
    base += [cases.mutate(rng, base[rng.randrange(30)], 0.03, b"ACGT") for _ in range(10)]  # multi-map
    planted = {g: (0, 100, 37, 61)[g] for g in range(4)}  # at the start, flush with the end, in between

    def plant(ts, where):
        ts = list(ts)
        for g, p in where.items():
            if len(ts[g]) >= p + 200:
                ts[g] = ts[g][:p] + motif + ts[g][p + 200:]
        return ts

    plain = plant(base, planted)
    xdb = list(plain)
    for g in (5, 9, 17, 26):  # single X
        t = bytearray(xdb[g])
        for _ in range(1 + g % 3):
            t[rng.randrange(300)] = ord("X")
        xdb[g] = bytes(t)
    t = bytearray(xdb[12])
    t[140:147] = b"X" * 7  # a run
    xdb[12] = bytes(t)
    more = dict(planted)
    more.update({g: rng.randrange(0, 101) for g in range(4, 13)})
    ragged = plant(base, more)
    for g, n in ((13, 0), (14, 3), (15, 9), (16, 11), (20, 47), (21, 101), (22, 230)):  # shorter than a window, and odd
        ragged[g] = ragged[g][:n]
    dbs = {"plain": plain, "xdb": xdb, "ragged": ragged}

    def cut(L, src=None):
        t = plain[rng.randrange(40)] if src is None else src
        p = rng.choice((0, len(t) - L, rng.randrange(len(t) - L + 1)))
        return cases.mutate(rng, t[p:p + L], rng.choice((0, 0.03)), b"ACGT")

    def r100():
        u = rng.random()
        if u < 0.1:
            return rnd(rng.randint(8, 100))
        if u < 0.3:
            return cut(rng.randint(40, 100), src=motif)
        return cut(rng.choice((100, 100, rng.randint(12, 99))))

    def with_x(r, lo, hi, n):
        b = bytearray(r)
        for _ in range(n):
            if hi <= len(b):
                b[rng.randrange(lo, hi)] = ord("X")
        return bytes(b)

    reads = {}
    reads["big"] = _distinct(lambda: cut(100, src=motif) if rng.random() < 0.8 else cut(100), 64 * 6 + 37)
    reads["r100"] = _distinct(r100, 60)
    reads["r100b"] = _distinct(r100, 60)
    reads["r150"] = _distinct(lambda: cut(150), 40)
    reads["r250"] = _distinct(lambda: cut(rng.choice((250, 250, rng.randint(101, 249)))), 30)
    # X outside every window of the pool (they end before base 44), at most three a read
    reads["rx"] = _distinct(lambda: with_x(r100(), 60, 100, rng.randint(0, 3)), 50)
    # X inside a window of every window set
    reads["rxin"] = _distinct(lambda: with_x(with_x(r100(), 0, 40, rng.randint(0, 2)), 60, 100, rng.randint(0, 1)), 50)
    reads["one"] = [plain[35][50:150]]  # (a target no database of the pool cuts short or masks)
    reads["none"] = []
    for name in ("big", "r100", "r100b", "rx", "rxin", "one"):
        assert max(len(r) for r in reads[name]) == 100, name
    assert any(b"X" in r[:44] for r in reads["rxin"]) and not any(b"X" in r[:60] for r in reads["rx"])

    def par(**kw):
        d = dict(Windows=[0, 20], WindowWidth=10, PMatch=0.9, MinDinuc=2, MaxReadLength=300, MaxMatches=1000000, MMTol=1,
                 MatchMode="best")
        d.update(kw)
        return orc.Config(**d)

    params = {"p0": par(), "win5": par(Windows=[5, 20]), "win30": par(Windows=[10, 30]), "ww12": par(WindowWidth=12),
              "pm80": par(PMatch=0.8), "dinuc7": par(MinDinuc=7), "tol3": par(MMTol=3), "first": par(MatchMode="first"),
              "mm20k": par(MaxMatches=20000), "mm6": par(MaxMatches=6), "mm6first": par(MaxMatches=6, MatchMode="first")}
    return dbs, reads, params


def db_of(name):
    return pools()[0][name]


def reads_of(name):
    return pools()[1][name]


def params_of(name):
    return pools()[2][name]


FIXED_LEN = {"big": 100, "r150": 150, "one": 100}  # the sets a streamed load takes: one length, no X
EMPTY = {("none", d) for d in ("plain", "xdb", "ragged")}  # (reads, database) without a tuple by design


def raw_reads(name, salt):
    """The read set as a shuffled multiset with duplicates (what read prep collapses back into it)."""
    reads = reads_of(name)
    raw = list(reads) + list(reads[::3])
    random.Random(salt).shuffle(raw)
    return raw


def fastq_of(name, salt):
    return b"".join(b"@n%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(raw_reads(name, salt)))


def gene_rests(db):
    return [b"g%d\t%d" % (g % 31, len(t)) for g, t in enumerate(db_of(db))]


def read_tails(reads):
    return [b"%d\tr%d" % (1 + i % 3, i) for i in range(len(reads_of(reads)))]


# ------------------------------------------------------------------------------------------------------- oracle

@functools.lru_cache(maxsize=None)
def full_tuples(db, reads, par) -> Tuple[Tuple[int, int, int, int], ...]:
    """Every accepted tuple (no truncation), sorted."""
    return tuple(sorted(orc.match_direct(reads_of(reads), db_of(db), params_of(par), check_overflow=False)))


def pass_tuples(db, reads, par, apply_mmtol):
    full = full_tuples(db, reads, par)
    return tuple(sorted(orc.best_filter(full, params_of(par).MMTol))) if apply_mmtol else full


@functools.lru_cache(maxsize=None)
def replay_model(db, reads, par):
    return mc.model(reads_of(reads), db_of(db), params_of(par))


def replay_tuples(db, reads, par, apply_mmtol):
    union = replay_model(db, reads, par).union
    return tuple(sorted(orc.best_filter(union, params_of(par).MMTol) if apply_mmtol else union))


@functools.lru_cache(maxsize=None)
def hot(db, reads, par):
    return frozenset(cases.hot_probes(reads_of(reads), db_of(db), params_of(par), list(full_tuples(db, reads, par))))


def list_tuples(key):
    """The tuples of a resident list named by the model: ("pass" | "replay", db, reads, params, apply_mmtol)."""
    return (pass_tuples if key[0] == "pass" else replay_tuples)(*key[1:])


@functools.lru_cache(maxsize=None)
def ordered_lines(key, with_tails) -> Tuple[bytes, ...]:
    from test_gpu_results import oracle_text
    _, db, reads = key[:3]
    txt = oracle_text(reads_of(reads), db_of(db), gene_rests(db), list_tuples(key), read_tails(reads) if with_tails else None)
    return tuple(ln + b"\n" for ln in txt.split(b"\n")[:-1])


@functools.lru_cache(maxsize=None)
def side_texts(key) -> Tuple[bytes, bytes, bytes]:
    from test_gpu_side import expected
    _, db, reads = key[:3]
    R = [(r, 1 + i % 3, b"r%d" % i) for i, r in enumerate(reads_of(reads))]
    return tuple(expected(R, db_of(db), gene_rests(db), list_tuples(key)))


def side_records(which, text) -> List[bytes]:
    lines = text.split(b"\n")[:-1]
    per = 4 if which == 0 else 1
    return [b"".join(ln + b"\n" for ln in lines[i:i + per]) for i in range(0, len(lines), per)]


# ------------------------------------------------------------------------------------------------------- the model

def cut_targets(lens: Sequence[int], limit: int) -> List[int]:
    """Partitions of at most `limit` bases, greedily from the front (a longer target is one of its own)."""
    first, g = [0], 0
    while g < len(lens):
        total, g1 = 0, g
        while g1 < len(lens) and total + lens[g1] <= limit:
            total += lens[g1]
            g1 += 1
        g = max(g1, g + 1)
        first.append(g)
    return first


class Model:
    def __init__(self, batch64=False):
        self.db = self.reads = None
        self.streaming = False
        self.gtext = self.rtext = False
        self.list = None      # ("pass" | "replay", db, reads, params, apply_mmtol) while it stands
        self.list_no = 0      # counts the lists made: an order remembers whose it is
        self.order = None     # (list key, with read text, list_no)
        self.side = False
        self.env = {k: None for k in KNOBS}
        self.batch64 = batch64  # MUSC_BATCH_READS as musc_init read it: musc_reload_env does not change it
        self.part = 0
        self.resident = None  # the index in hand: (kind, ww, CL, g0, g1)
        self.nparts = 0

    # -- what a pass runs on
    def path(self, par):
        """{"kind", "nparts", "first", "family", "RW", "XM", "WIDE", "cls"} of a pass with `par` in this state, and the
        index resident after it."""
        P, reads, db = params_of(par), reads_of(self.reads), db_of(self.db)
        lens = [len(t) for t in db]
        first = cut_targets(lens, PART_BASES) if self.part else [0, len(db)]
        if len(first) == 2:
            first = [0, len(db)]
        nparts = len(first) - 1
        max_len = max([len(r) for r in reads], default=0)
        rw = max((((2 * max_len + 31) // 32 + 1 + 3) // 4) * 4, 4)
        db_x = any(b"X" in t for t in db)
        reads_x = any(b"X" in r for r in reads)
        q1min, q1max, ww = min(P.Windows), max(P.Windows), P.WindowWidth
        span = q1max - q1min + max_len
        ctx, wide = self.env["MUSC_INDEX"] is None and len(P.Windows) <= 4, False
        if ctx and (span > 120 or q1max > 120 or self.env["MUSC_CONTEXT"] == "wide"):
            wide = True
            ctx = self.env["MUSC_CONTEXT"] != "narrow" and span <= 200
        if ctx and reads_x:
            listed = 3 if wide else 4
            for r in reads:
                xs = [i for i, b in enumerate(r) if b == ord("X")]
                if db_x:  # every X listed, none inside a window
                    ctx = ctx and len(xs) <= listed and not any(q <= x < q + ww for x in xs for q in P.Windows)
                elif len(xs) > listed:  # more than its word lists: only if that many mismatches rule the read out
                    ctx = ctx and len(xs) > orc.nmiss_allowed(P.PMatch, len(r))
        out = {"nparts": nparts, "first": first, "RW": rw if rw in (4, 8, 12, 16) else 0}
        g0, g1 = first[-2], first[-1]
        if ctx:
            kind = 2 if wide else 1
            xm = 2 if db_x else 1 if reads_x else 0
            dma = self.env["MUSC_MATCH"] == "dma" and len(P.Windows) == 2 and rw == 8 and kind == 1 and not xm
            out.update(kind=kind, family="k_match_g" if dma else "k_match_t", XM=xm, WIDE=int(wide))
            out["cls"] = "g" if dma else "tx_db" if xm == 2 else "tx_reads" if xm == 1 else "twide" if wide else "t120"
            resident = (kind, ww, q1max, g0, g1)
        else:
            kind = 3 if self.env["MUSC_INDEX"] == "lines" else 0
            r = self.resident
            if nparts == 1 and self.env["MUSC_INDEX"] != "lines" and r and r[0] in (0, 3) and r[1:] == (ww, 0, g0, g1):
                kind = r[0]  # a resident window-start index for this width keeps its layout
            lane = kind == 3 and not (db_x or reads_x) and rw in (4, 8, 12, 16)
            out.update(kind=kind, family="k_screen_t" if lane else "k_screen", mask=int(db_x or reads_x))
            out["cls"] = "lines" if kind == 3 else "classic"
            resident = (kind, ww, 0, g0, g1)
        if out["RW"] == 0:
            out["cls"] = "rstride"
        if nparts > 1:
            out["cls"] = "part"
        return out, resident

    def _list_stands(self):
        return self.list is not None

    def _order_current(self):
        return self.order is not None

    def _drop_reads(self):
        self.list = self.order = None
        self.rtext = self.side = False

    # -- one step: what it must return.  {"error": (code, pattern) | None, ...}
    def apply(self, step) -> dict:
        k = step[0]
        exp = {"error": None}
        if k == "db":
            self.db = step[1]
            self.gtext = self.side = False
            self.list = self.order = self.resident = None
        elif k == "reads":
            self._drop_reads()
            self.reads = step[1]
            self.streaming = step[2] == "stream"
        elif k == "bad_reads":
            self._drop_reads()
            self.reads = None
            self.streaming = False
            exp["error"] = E_BAD_LOAD
        elif k == "index":
            if self.reads is not None:
                p, self.resident = self.path(step[1])
                if p["nparts"] > 1:  # the first partition's
                    self.resident = self.resident[:3] + (p["first"][0], p["first"][1])
                self.nparts = p["nparts"]
                exp["first"] = p["first"]
        elif k == "part":
            self.part = step[1]
        elif k == "env":
            self.env[step[1]] = step[2]
        elif k == "pass":
            self.side = False  # (the order keeps serving its text; the side stage does not)
            self.list = None
            self.list_no += 1
            if self.reads is None:
                exp["error"] = E_NO_READS
            else:
                self.streaming = False
                p, self.resident = self.path(step[1])
                self.list = ("pass", self.db, self.reads, step[1], bool(step[2]))
                exp.update(path=p, list=self.list)
        elif k == "replay":
            if self.list is None or self.list[0] != "pass":
                exp["error"] = E_NOT_MATCH_LIST
            elif self.list[4]:
                exp["error"] = E_PASS_HAD_MMTOL
            else:
                _, db, reads, par, _ = self.list
                rep = replay_model(db, reads, par)
                exp["truncated"] = len(rep.truncated)
                if full_tuples(db, reads, par) and (rep.truncated or step[1]):
                    self.list = ("replay", db, reads, par, bool(step[1]))
                    self.list_no += 1
                    self.side = False
                exp["list"] = self.list
        elif k == "probes":
            exp["list"] = self.list if self.list and self.list[0] == "pass" else None
        elif k == "gtext":
            self.gtext, self.order, self.side = True, None, False
        elif k == "rtext":
            if self.reads is None or self.streaming:
                exp["skip"] = True
            else:
                self.rtext, self.order, self.side = True, None, False
        elif k == "order":
            self.order, self.side = None, False
            if not self.gtext:
                exp["error"] = E_NO_GENE_TEXT
            elif self.list is None:
                exp["error"] = E_NOT_PASS_LIST
            else:
                self.order = (self.list, self.rtext, self.list_no)
                exp["lines"] = self.order[:2]
        elif k in ("rhits", "text"):
            if self.order is None:
                exp["error"] = E_NO_ORDER
            else:
                exp["lines"] = self.order[:2]
        elif k == "side":
            self.side = False
            if self.order is None:
                exp["error"] = E_NO_ORDER
            elif self.order[2] != self.list_no:
                exp["error"] = E_PASS_AFTER
            elif not self.rtext:
                exp["error"] = E_NO_READ_TEXT
            else:
                self.side = True
                exp["side"] = self.order[0]
        elif k == "side_text":
            if not (self.side and self.order is not None and self.order[2] == self.list_no):
                exp["error"] = E_NOT_PREPARED
            else:
                exp["side"] = self.order[0]
        else:
            raise ValueError("unknown step %r" % (step,))
        return exp


def expectations(steps, batch64=False):
    m = Model(batch64)
    return [m.apply(s) for s in steps]


# ------------------------------------------------------------------------------------------------------- generators

SEEDS = tuple(range(12))
STEPS = 60


def batch64_of(seed) -> bool:
    """Whether the walk's context is made with MUSC_BATCH_READS=64 (musc_init latches it for the context's lifetime)."""
    return seed % 2 == 1


def param_tour(seed: int) -> List[str]:
    """The parameter sets in an order whose consecutive pairs, over the committed seeds, are every ordered pair: the
    complete digraph on a prime number of sets is the union of the cycles 0, d, 2d, ... for d = 1 .. n - 1, walked one
    after the other from set 0; seed k takes the k-th stretch of n - 1 steps of that circuit."""
    names = sorted(pools()[2])
    n = len(names)
    assert n == 11  # (prime: every d generates the whole cycle)
    circuit = [0]
    for d in range(1, n):
        circuit += [(d * i) % n for i in range(1, n + 1)]
    lo = (seed % n) * (n - 1)
    return [names[i] for i in circuit[lo:lo + n]]


def generate(seed: int, nsteps: int = STEPS) -> List[tuple]:
    """The walk of `seed`: the large read set first, so that every later run finds buffers that held more; then random
    steps, with four blocks placed among them: a knob flipped and put back, a pass after each, the seed's stretch of the parameter tour on standing inputs, the stages
    in an order in which each must succeed and then be refused, and a replay followed by order, text and a pass."""
    rng = random.Random(7919 * seed + 13)
    dbs, readsets, params = (sorted(p) for p in pools())
    small = [r for r in readsets if r != "big"]
    steps = []
    m = Model(batch64_of(seed))

    def emit(*ss):
        for s in ss:
            steps.append(s)
            m.apply(s)

    def some_pass(par=None, apply_mmtol=None, times=None):
        return ("pass", par or rng.choice(params), rng.random() < 0.5 if apply_mmtol is None else apply_mmtol,
                rng.choice(("host", "dev", "packed", "compact")), times or rng.choice((1, 1, 2, 3)))

    def load(reads, loader=None):
        ok = ["ascii", "packed", "fastq"] if reads == "none" else [l for l in LOADERS if l != "stream" or reads in FIXED_LEN]
        emit(("reads", reads, loader if loader in ok else rng.choice(ok)))
        if m.streaming:  # the buffer of a streamed load is borrowed until the pass
            emit(some_pass())

    def tour():
        if m.reads in ("big", "none"):
            load(small[seed % len(small)] if small[seed % len(small)] != "none" else "r100")
        for par in param_tour(seed):
            emit(some_pass(par, times=1))

    def stages():
        load(m.reads)  # (the same reads again: the load forgets their text)
        emit(("rhits",), ("gtext",), some_pass(apply_mmtol=True, times=1), ("order",), ("side",), ("rtext",), ("order",), ("rhits",),
             ("text", rng.randrange(1000), rng.randrange(1, 40)), ("side",))
        for which in range(3):
            emit(("side_text", which, rng.randrange(1000), rng.randrange(1, 40)))
        emit(("replay", False))  # refused: the pass applied MMTol
        emit(some_pass(times=1), ("side",), ("side_text", rng.randrange(3), 0, 5), ("text", rng.randrange(1000), rng.randrange(1, 40)))

    def knob():
        flips = [(k, v) for k in KNOBS for v in ENV_VALUES[k] if v is not None]
        var, value = flips[seed % len(flips)]
        emit(("env", var, value), some_pass(), ("env", var, None), some_pass())

    def replayed():
        emit(("pass", rng.choice(("mm6", "mm6first")), False, rng.choice(("dev", "host")), 1), ("replay", rng.random() < 0.5), ("gtext",),
             ("order",), ("text", rng.randrange(1000), rng.randrange(1, 40)), some_pass())

    emit(("db", dbs[seed % len(dbs)], ("ascii", "packed")[seed // 3 % 2]))
    load("big", LOADERS[seed % len(LOADERS)])
    if steps[-1][0] != "pass":
        emit(some_pass(rng.choice(("p0", "mm20k", "mm6"))))
    blocks = [(rng.randrange(6, 40), f) for f in (tour, stages, replayed, knob)]
    par = "p0"
    while len(steps) < nsteps or blocks:
        due = [b for b in blocks if b[0] <= len(steps)] or (blocks if len(steps) >= nsteps else [])
        if due:
            blocks.remove(due[0])
            if m.reads is None or m.reads == "none":
                load(rng.choice(small[:-1]) if small[-1] == "none" else "r100")
            due[0][1]()
            continue
        u = rng.random()
        if u < 0.06:
            emit(("db", rng.choice(dbs), rng.choice(("ascii", "packed"))))
        elif u < 0.24:
            load(small[(seed + len(steps)) % len(small)] if rng.random() < 0.6 else rng.choice(readsets))
        elif u < 0.28:
            emit(("bad_reads",), some_pass())
            load(rng.choice(small))
        elif u < 0.32:
            emit(("index", rng.choice(params)))
        elif u < 0.38:
            emit(("part", 0 if m.part else 1))
        elif u < 0.52:
            on = [k for k in KNOBS if m.env[k] is not None]
            if on and rng.random() < 0.5:  # every walk comes back to the default path
                emit(("env", rng.choice(on), None))
            else:
                var = rng.choice(KNOBS)
                emit(("env", var, rng.choice([v for v in ENV_VALUES[var] if v != m.env[var]])))
        elif u < 0.72:
            for _ in range(rng.choice((1, 2))):
                par = rng.choice(params)
                emit(some_pass(par))
        elif u < 0.77:
            emit(("pass", rng.choice(("mm6", "mm20k", par)), False, rng.choice(("dev", "host")), 1), ("replay", rng.random() < 0.5))
        elif u < 0.80:
            emit(("replay", rng.random() < 0.5))
        elif u < 0.83:
            emit(("probes",))
        elif u < 0.86:
            emit(("gtext",))
        elif u < 0.89:
            emit(("rtext",))
        elif u < 0.92:
            emit(("order",))
        elif u < 0.94:
            emit(("rhits",))
        elif u < 0.96:
            emit(("text", rng.randrange(1000), rng.randrange(1, 40)))
        elif u < 0.98:
            emit(("side",))
        else:
            emit(("side_text", rng.randrange(3), rng.randrange(1000), rng.randrange(1, 40)))
    return steps


def replay(seed: int, upto: Optional[int] = None) -> List[tuple]:
    """The first `upto` steps of the walk of `seed` (a debugging session feeds them to test_gpu_walk.run_walk)."""
    steps = directed() if seed == "directed" else generate(seed)
    return steps if upto is None else steps[:upto]


# the state that puts a pass on each path class: (database, reads, MUSC_INDEX, MUSC_MATCH, partitioned)
CLASS_STATE = {"t120": ("plain", "r100", None, None, 0), "g": ("plain", "r100", None, "dma", 0),
               "twide": ("plain", "r150", None, None, 0), "tx_reads": ("plain", "rx", None, None, 0),
               "tx_db": ("xdb", "r100", None, None, 0), "classic": ("plain", "r100", "classic", None, 0),
               "lines": ("plain", "r100", "lines", None, 0), "rstride": ("plain", "r250", None, None, 0),
               "part": ("plain", "r100", None, None, 1)}


def directed() -> List[tuple]:
    """One sequence that holds every ordered pair of path classes back to back: a pass on A, the steps that force the
    change, a pass on B."""
    m, steps = Model(), []

    def emit(s):
        steps.append(s)
        m.apply(s)

    def goto(cls):
        db, reads, index, match, part = CLASS_STATE[cls]
        if m.db != db:
            emit(("db", db, "ascii"))
        if m.reads != reads:
            emit(("reads", reads, "ascii"))
        for var, v in (("MUSC_INDEX", index), ("MUSC_MATCH", match)):
            if m.env[var] != v:
                emit(("env", var, v))
        if m.part != part:
            emit(("part", part))
        if m.path("p0")[0]["cls"] != cls:  # a resident line index would keep its layout: a load forgets it
            emit(("db", db, "ascii"))
        assert m.path("p0")[0]["cls"] == cls, (cls, m.path("p0"))

    n = 0
    for a in CLASSES:
        for b in CLASSES:
            goto(a)
            emit(("pass", "p0", n % 2 == 0, "host", 1))
            goto(b)
            emit(("pass", "p0", n % 3 == 0, "host", 1))
            n += 1
    return steps


def pass_classes(steps, batch64=False) -> List[Optional[str]]:
    """Per step: the path class of a pass that runs, else None."""
    return [e["path"]["cls"] if "path" in e else None for e in expectations(steps, batch64)]
