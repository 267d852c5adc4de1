"""Inputs of the long-read tests (tests/test_gpu_long_reads.py), in plain Python: reads of up to 65 535 bases on the
two-kernel path -- k_screen<0, ..> (Rec<0>), the runtime-stride branch of confirm_pair in k_confirm<0, ..>, the budget
table beyond its LDS copy -- and what follows a match whose nmiss has three and four digits.

A case is a seeded database, a sorted list of distinct reads, a configuration, and `roles`: which read plays which
part, so that the coverage conditions (tests/test_long_read_cases.py, no GPU) can be asserted from the ORACLE's tuples.
Beyond a few hundred bases oracle/muscato_oracle.py and oracle/literal.cpp are the only pin; the same CPU test holds
them to each other on every case.

The database, in this order: T0 (LMAX + 300 random bases), T0' (T0 with every 97th base changed: a long read has two
placements with different nmiss), 500 random bases, an empty target, and LAST, 180 bases -- the database ends where
the short reads sit.  Long reads are T0[100 : 100 + n] with a chosen number of mismatches, laid from the last base
backwards (the last record word), two of them in record words 64 and 65 (the first words a 1 000-base stride does not
have), the rest spread over the read, none inside a window.

X variants.  "reads": the long reads hold X at base 1 024 (the first base of record word 64), on either side of the
word boundary at 2 048 and at their last base.  "db": T0 holds X under the read at 1 024, 2 048 and the last base of
the longest read, and the reads hold X at 2 048 as well (X == X matches).  The base that faces an X is A on the other
side -- code 0, what an X is stored as -- so that only the mask plane tells them apart."""
import functools
import random

import numpy as np

import loader_cases as lc

WW = 15
T0_AT = 100                       # a long read of n bases is T0[T0_AT : T0_AT + n]
T0_EXTRA = 300
PHASES = (0, 1, 15, 16, 17)       # lengths LMAX - d: every way the last base word and the word count can fall
SPLIT_LENS = (255, 256, 257)      # the kernels keep the budgets of lengths < 256 (CONF_NM) in LDS
WORD64, WORD65 = 1030, 1045       # a base of record word 64 and one of word 65
X_READ_PLACES = (1024, 2047, 2048)
X_DB_PLACES = (1024, 2048)        # and the last base of the longest read
X_BOTH = 2048
MMTOL = 3

# name -> (LMAX, windows, PMatch, MinDinuc, X variant)
SPECS = {
    "L1000": (1000, (0, 20), 0.9, 0, ""),      # stride 64 words: the last that fits 64 words of slack
    "L1009": (1009, (0, 20), 0.97, 0, ""),     # stride 68: the first that does not
    "L4099": (4099, (0, 20), 0.9, 0, ""),      # stride 260
    "L4099-w1": (4099, (0,), 0.9, 0, ""),
    "L4099-w3": (4099, (0, 20, 40), 0.9, 2, ""),
    "L4099-far": (4099, (0, 4000), 0.9, 2, ""),
    "L4099-xr": (4099, (0, 20), 0.9, 0, "reads"),
    "L4099-xt": (4099, (0, 20), 0.9, 0, "db"),
    "L65535": (65535, (0, 20), 0.9, 0, ""),    # stride 4 100: the limit
    "L65535-xr": (65535, (0, 20), 0.9, 0, "reads"),
    "L65535-xt": (65535, (0, 20), 0.9, 0, "db"),
    "L65535-far": (65535, (0, 65500), 0.9, 0, ""),
}
NAMES = tuple(SPECS)
LMAXES = (1000, 1009, 4099, 65535)


def budget(pmatch, n):
    """A read's mismatch budget as the reference computes it: IEEE double, truncated."""
    return int((1 - pmatch) * float(n))


def step_up(pmatch, lo):
    """The smallest length >= lo whose budget is one more than that of the length before it."""
    n = lo
    while budget(pmatch, n) == budget(pmatch, n - 1):
        n += 1
    return n


def step_down(pmatch, hi):
    """The largest such length <= hi."""
    n = hi
    while budget(pmatch, n) == budget(pmatch, n - 1):
        n -= 1
    return n


def _other(base, salt):
    return lc.ACGT[(lc.ACGT.index(base) + 1 + salt % 3) % 4]


class Case:
    def __init__(self, name):
        self.name = name
        self.lmax, self.windows, self.pmatch, self.min_dinuc, self.x = SPECS[name]
        self.ww = WW
        self.budget = budget(self.pmatch, self.lmax)
        self._build()

    def ocfg(self, **kw):
        from oracle import muscato_oracle as orc
        d = dict(Windows=list(self.windows), WindowWidth=self.ww, PMatch=self.pmatch, MinDinuc=self.min_dinuc,
                 MaxReadLength=self.lmax, MaxMatches=1000000, MMTol=MMTOL)
        d.update(kw)
        return orc.Config(**d)

    # ---- construction
    def _build(self):
        lmax, x = self.lmax, self.x
        rng = random.Random(7 * lmax + 1)  # (the variants of one LMAX share their bases)
        n0 = lmax + T0_EXTRA
        t0 = bytearray(lc.rand_bases(rng, n0))
        self.phase_lens = [lmax - d for d in PHASES]
        for p in X_READ_PLACES + tuple(n - 1 for n in self.phase_lens):
            if p < lmax:
                t0[T0_AT + p] = ord("A")
        self.t0 = t0 = bytes(t0)
        t0p = bytearray(t0)
        for i in range(96, n0, 97):
            t0p[i] = _other(t0[i], i)
        mid, last = lc.rand_bases(rng, 500), lc.rand_bases(rng, 180)
        t0_db = bytearray(t0)
        if x == "db":
            for p in X_DB_PLACES + (lmax - 1,):
                t0_db[T0_AT + p] = ord("X")
        self.t0_db = bytes(t0_db)
        self.targets = [self.t0_db, bytes(t0p), mid, b"", last]
        self.total_bases = sum(len(t) for t in self.targets)
        self.inwin = set()
        for q in self.windows:
            self.inwin.update(range(q, q + self.ww))

        roles = {}
        B = self.budget
        roles["long_0"] = self.cut(lmax, None)
        for tag, m in (("bm1", B - 1), ("b", B), ("bp1", B + 1)):
            roles["long_" + tag] = self.cut(lmax, m)
        w0 = bytearray(roles["long_0"])
        w0[5] = _other(w0[5], 5)  # inside window 0 only: a later window alone finds the read
        roles["long_w0"] = bytes(w0)
        for n in self.phase_lens[1:]:
            roles["ph%d_b" % n] = self.cut(n, budget(self.pmatch, n))
            roles["ph%d_bp1" % n] = self.cut(n, budget(self.pmatch, n) + 1)
        self.step_lens = sorted({step_up(self.pmatch, 258), step_down(self.pmatch, lmax)})
        for n in self.step_lens:
            roles["step%d_b" % n] = self.cut(n, budget(self.pmatch, n))
            roles["step%d_bp1" % n] = self.cut(n, budget(self.pmatch, n) + 1)
        self.ten = 0
        if self.pmatch == 0.9:
            self.ten = lmax // 10 * 10
            roles["ten_acc"] = self.cut(self.ten, self.ten // 10 - 1)
            roles["ten_rej"] = self.cut(self.ten, self.ten // 10)
        for n in SPLIT_LENS:
            roles["split%d_b" % n] = self.cut(n, budget(self.pmatch, n), start=300)
            roles["split%d_bp1" % n] = self.cut(n, budget(self.pmatch, n) + 1, start=300)
        # short reads where the database ends, where T0 ends, across target boundaries, and at position 0
        for n in (40, 57, 120):
            roles["flush_last_%d" % n] = last[180 - n:]
        for n in (40, 57):  # one base further: the base behind the database's last is the zeroed slack, an A
            roles["over_last_%d" % n] = last[180 - n + 1:] + b"A"
        for n in (40, 200):
            roles["flush_t0_%d" % n] = t0[n0 - n:]
        roles["straddle_t0"] = t0[n0 - 39:] + bytes(t0p[:1])  # contiguous in the database, not inside one target
        roles["straddle_mid"] = mid[-20:] + last[:20]
        for n in (85, 86, 120):  # 100 - q2 = 85: the longest read window 0 places at position 0
            roles["pos0_%d" % n] = t0[:n]
        for n in (85, 86):
            r = bytearray(t0[:n])
            r[25] = _other(r[25], 25)  # inside the window at 20: window 0 (or one from 26 on) has to find the read
            roles["pos0_%d_w0" % n] = bytes(r)
        self.reads = sorted(set(roles.values()))
        index = {r: i for i, r in enumerate(self.reads)}
        self.roles = {k: index[v] for k, v in roles.items()}

    def cut(self, n, m, start=T0_AT):
        """T0[start : start + n] with the variant's X and exactly m mismatches against the database there (m None: only
        those the X bring)."""
        r = bytearray(self.t0[start:start + n])
        fixed = set(self.inwin)
        if start == T0_AT and n > 2048:
            if self.x == "reads":
                for p in X_READ_PLACES + ((n - 1,) if n in self.phase_lens else ()):
                    r[p] = ord("X")
                    fixed.add(p)
            elif self.x == "db":
                r[X_BOTH] = ord("X")
                fixed.add(X_BOTH)
        tgt = self.t0_db[start:start + n]
        have = [i for i in range(n) if r[i] != tgt[i]]
        if m is None:
            return bytes(r)
        assert len(have) <= m, (self.name, n, m, have)
        fixed.update(have)
        fixed.update(i for i in range(n) if tgt[i] == ord("X"))
        need = m - len(have)
        picks = [p for p in (n - 1, WORD64, WORD65) if p < n and p not in fixed][:need]
        cands = [p for p in range(n - 1, -1, -1) if p not in fixed and p not in picks]
        k = need - len(picks)
        picks += [cands[i * len(cands) // k] for i in range(k)]
        assert len(set(picks)) == need
        for p in picks:
            r[p] = _other(r[p], p)
        return bytes(r)

    # ---- what the tests ask
    def rests(self):
        return lc.target_rests(self.targets)

    def read_of(self, role):
        return self.reads[self.roles[role]]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def oracle_hits(name):
    """Every accepted tuple of the case by oracle/literal.cpp: sorted uint32 [n, 4], made once, not to be changed."""
    from oracle import literal
    c = case(name)
    rbuf, roff = literal.concat(c.reads)
    gbuf, goff = literal.concat(c.targets)
    hits, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(c.ocfg(), bloom_size=4_000_000, num_hash=20))
    hits = np.array(sorted(map(tuple, hits.tolist())), dtype=np.uint32).reshape(-1, 4)
    hits.setflags(write=False)
    return hits


def best_hits(name, mmtol):
    """The per-read best + MMTol selection of oracle_hits: sorted uint32 [n, 4]."""
    from oracle import muscato_oracle as orc
    keep = orc.best_filter(map(tuple, oracle_hits(name).tolist()), mmtol)
    return np.array(sorted(keep), dtype=np.uint32).reshape(-1, 4)
