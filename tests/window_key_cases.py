"""Inputs of the window-key tests (tests/test_gpu_window_keys.py), in plain Python: WindowWidth 16 to 4096, where the
window key is no longer one word of a direct table -- a hashed table folded 64 bits at a time (bucket_of / rec_bucket),
the general MinDinuc gate in 32-base chunks that overlap by one base (rec_count_dinuc), and an exact window comparison
whose masks span several words (k_match_t, k_match_g, confirm_pair).

A case is a seeded database, a sorted list of distinct reads, a configuration and `roles`: which read plays which part,
so that tests/test_window_key_cases.py (no GPU) can assert from the ORACLE's tuples that the case still holds what it
exists for.  The three key classes: 16 (one word, always hashed: 2 * 16 > 30 bits), 17-32 (one 64-bit chunk), 33 and
more (several chunks; the gate's chunk seams are at bases 31, 62, 93 ...).

The parts of a case.

  random   families of a target and three copies at 2 % substitutions, a few low-complexity targets (a unit of 1-3
           bases repeated, 3 % point changes); reads at full length and ragged -- exactly max(Windows) + ww bases and one
           less: the last window just valid and just invalid -- at position 0, flush with the target end and in
           between, with 0-3 % substitutions.
  eq       (two windows) for each window k and every base p of it a read that copies a placement of the target EQ
           exactly but for one substitution at base p of window k.  The other window reports the tuple, once, unless
           it covers that base too (the windows of the 100-base geometries overlap from width 18 on): then no window of
           the read equals the target and the oracle has no tuple for it.  A window mask that misses base p loses the
           tuple, reports one that does not exist, or miscounts n_accepted.
  dinuc    for each window k and every p a target window that is poly-A with a single C at base p (window 0; the
           later windows take G/T, C/A, T/G: with one pair of letters window 0's key would sit in window 1's targets
           as well), between random flanks, and a read that copies it: 3 distinct pairs when p is interior, 2 at
           either end, MinDinuc 3.  The read ends two bases behind window k (MaxReadLength allowing), and every
           other window it is long enough for carries one substitution outside window k: window k alone can report
           the tuple, so the gate's verdict IS the tuple.  A pair dropped or counted twice at a chunk seam flips it
           at p = 31, 32, 62, 63.
  X        "xr": an X-free database; reads with up to three X outside every window, and reads with one X inside a
           window (barred on the fused path).  "xd": a database with X at 0.3 %; reads keep the target's X outside
           the run's windows -- also those the read is too short for: the host's check does not look at lengths --
           three at most (k_match_t<.., XM = 2>).  "xw": the same database; reads keep the target's X inside their
           windows as well -- the two-kernel path with the mask plane, where X == X matches -- and, from width 33
           on, three planted windows per window start with an X in one chunk of the gate and none in another (its
           merge loop): two pass MinDinuc only if the pairs of both kinds of chunk are counted, one fails it.

Widths above 128 (the case at the limit, 4096) take the sweeps at the bases places() names, and their family copies
differ from the original in its first 40 bases only (at 2 % no copy would share a 4 096-base window).

Reference limits every case respects (asserted in the CPU test): oracle/literal.cpp returns no error; a window at 0
keeps ww <= 50 (the reference panics when 100 - ww < ww there); MaxReadLength >= max(Windows) + ww."""
import functools
import random

import numpy as np

X = ord("X")
ACGT = b"ACGT"
MIN_DINUC = 3
MMTOL = 1
SMALL_MM = 2     # a family is a target and three copies: an exact read's block accepts up to four pairs
EQ_AT = 7        # where the eq reads sit in the target EQ
SEAMS = (31, 32, 62, 63)
PAIRS = (b"AC", b"GT", b"CA", b"TG")  # window k's dinuc windows are poly-PAIRS[k][0] with a single PAIRS[k][1]


def places(ww):
    """The bases of a window the sweeps visit: all of them up to 128, beyond that both ends, the gate's first seams,
    the first 64-bit chunk's end, the middle and the last chunk's first base (each dinuc place costs a target
    segment of the window's length)."""
    if ww <= 128:
        return list(range(ww))
    want = {0, 1, 31, 32, 62, 63, 64, ww // 2 - 1, ww // 2, ww - 33, ww - 1}
    return sorted(p for p in want if 0 <= p < ww)


# name -> (WindowWidth, Windows, MaxReadLength, PMatch, X variant)
SPECS = {}
for _ww in (16, 17, 31, 32, 33, 48, 63, 64):          # 120-base context buckets: 17 + 100 bases of context, records of 8 words
    SPECS["n%d" % _ww] = (_ww, (3, 20), 100, 0.93, "")
for _x in ("xr", "xd", "xw"):
    for _ww in (16, 32, 33, 64):
        SPECS["n%d-%s" % (_ww, _x)] = (_ww, (3, 20), 100, 0.93, _x)
for _ww, _wins in ((16, (1, 22)), (32, (1, 22)), (33, (1, 22)), (64, (1, 22)), (96, (1, 22)), (97, (1, 40)), (128, (1, 22))):
    SPECS["w%d" % _ww] = (_ww, _wins, 150, 0.93, "")   # wide buckets: up to 200 bases of context, records of 12 words
for _ww in (16, 32, 65):                               # three windows (k_confirm's w2 = false), 198 bases of context
    SPECS["w%d-3" % _ww] = (_ww, (2, 30, 50), 150, 0.93, "")
SPECS["w33-4"] = (33, (0, 10, 30, 50), 150, 0.93, "")  # four windows, one at 0
SPECS["w33-xr"] = (33, (1, 22), 150, 0.93, "xr")
SPECS["w64-xd"] = (64, (1, 22), 150, 0.93, "xd")
for _ww, _wins, _L in ((16, (1, 200), 250), (32, (1, 200), 250), (33, (1, 200), 250), (64, (1, 150), 250), (97, (1, 300), 450),
                       (128, (1, 130), 260)):
    SPECS["r%d" % _ww] = (_ww, _wins, _L, 0.95, "")    # the runtime stride: one window far into the read
SPECS["r64-3"] = (64, (1, 70, 150), 250, 0.95, "")
SPECS["r33-xw"] = (33, (1, 200), 250, 0.95, "xw")
SPECS["k4096"] = (4096, (1, 60), 4200, 0.98, "")       # the limit of check_params
NAMES = tuple(SPECS)


def rand_seq(rng, n, alphabet=ACGT):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet=ACGT):
    """Point changes at `rate`; an X of s stays."""
    b = bytearray(s)
    for i in range(len(b)):
        if b[i] != X and rng.random() < rate:
            b[i] = rng.choice(alphabet)
    return bytes(b)


def other(base, salt=0):
    return ACGT[(ACGT.index(base) + 1 + salt % 3) % 4] if base in ACGT else ACGT[salt % 4]


def low_complexity(rng, n):
    unit = rand_seq(rng, rng.choice([1, 2, 3]))
    return mutate(rng, (unit * (n // len(unit) + 1))[:n], 0.03)


class Case:
    def __init__(self, name, spec=None, seed=None, sweeps=True):
        """A named case of SPECS at its pinned seed -- or any (WindowWidth, Windows, MaxReadLength, PMatch, X variant)
        at any seed; sweeps = False: the random part alone."""
        self.name = name
        self.ww, self.windows, self.lmax, self.pmatch, self.x = SPECS[name] if spec is None else spec
        self.windows = tuple(self.windows)
        self.seed = SEEDS.get(name, 0) if seed is None else seed
        self.sweeps = sweeps
        self._build()

    def ocfg(self, **kw):
        from oracle import muscato_oracle as orc
        d = dict(Windows=list(self.windows), WindowWidth=self.ww, PMatch=self.pmatch, MinDinuc=MIN_DINUC,
                 MaxReadLength=self.lmax, MaxMatches=1000000, MMTol=MMTOL)
        d.update(kw)
        return orc.Config(**d)

    # ---- construction
    def in_window(self, i, length, skip=None):
        """Whether base i lies in a window (other than `skip`) that a read of `length` bases is long enough for."""
        return any(q <= i < q + self.ww for k, q in enumerate(self.windows) if k != skip and q + self.ww <= length)

    def _build(self):
        ww, wins, L = self.ww, self.windows, self.lmax
        rng = random.Random(1000 * ww + 10 * len(wins) + L + 7919 * self.seed + sum(map(ord, self.x)))
        last = max(wins) + ww
        assert last <= L and (min(wins) > 0 or ww <= 50)
        big = ww > 128
        nfam, nlow, nrand = (1, 1, 60) if big else (5, 3, 200) if L > 150 else (12, 8, 300)
        fam = []
        for _ in range(nfam):
            base = rand_seq(rng, rng.randint(L + 50, L + 300) if big else rng.randint(L, 3 * L))
            fam.append(base)
            if big:  # (2 % would leave no copy with a window in common: these differ in their first 40 bases only)
                for n in (1, 3, 4):
                    t = bytearray(base)
                    for i in rng.sample(range(40), n):
                        t[i] = other(t[i], i)
                    fam.append(bytes(t))
            else:
                fam.extend(mutate(rng, base, 0.02) for _ in range(3))
        fam.extend(low_complexity(rng, rng.randint(L, 2 * L)) for _ in range(nlow))
        if self.x in ("xd", "xw"):
            fam = [mutate(rng, t, 0.003, b"X") for t in fam]
        self.n_random_targets = len(fam)
        targets = list(fam)
        reads, roles = set(), {}

        def random_read():
            t = rng.choice(fam)
            n = rng.choice([L, L, rng.randint(last - 1, L), last, last - 1, rng.randint(max(1, ww - 2), L), min(wins) + ww - 1])
            if len(t) < n:
                return None
            p = rng.choice([0, len(t) - n, rng.randint(0, len(t) - n)])
            r = bytearray(mutate(rng, t[p:p + n], rng.choice([0, 0.01, 0.03])))
            xs = [i for i in range(n) if r[i] == X]
            if xs:  # a database with X: keep up to three of the target's (xd: outside the windows only), or none
                keep = []
                if rng.random() < 0.6:
                    keep = [i for i in xs if self.x == "xw" or not self.in_window(i, L)][:3]  # (xd: outside every window, whatever the read's length)
                for i in xs:
                    if i not in keep:
                        r[i] = rng.choice(ACGT)
            if self.x == "xr":
                u = rng.random()
                out = [i for i in range(n) if not self.in_window(i, n)]
                if u < 0.3 and out:
                    for i in rng.sample(out, min(len(out), rng.randint(1, 3))):
                        r[i] = X
                elif u < 0.45 and n >= min(wins) + ww:
                    q = rng.choice([q for q in wins if q + ww <= n])
                    r[q + rng.randrange(ww)] = X
            return bytes(r)

        while len(reads) < nrand:
            r = random_read()
            if r is not None:
                reads.add(r)

        def spoil_others(r, k):
            """One substitution in every window other than k the read is long enough for, outside window k."""
            n, qk, subs = len(r), wins[k], 0
            for j, q in enumerate(wins):
                if j == k or q + ww > n:
                    continue
                free = [i for i in range(q, q + ww) if not qk <= i < qk + ww and r[i] != X]
                assert free, (self.name, k, j)
                i = free[len(free) // 2]
                r[i] = other(r[i], i)
                subs += 1
            return subs

        def planted(tag, k, window):
            """A target segment whose window k is `window`, and the read that copies it (dinuc in the docstring)."""
            n = min(wins[k] + ww + 2, L)
            body = bytearray(rand_seq(rng, n))
            body[wins[k]:wins[k] + ww] = window
            for i in (wins[k] - 1, wins[k] + ww):  # the flanks do not continue the window
                if 0 <= i < n and body[i] in PAIRS[k]:
                    body[i] = PAIRS[k ^ 1][0]
            r = bytearray(body)
            before = bytes(r)
            spoil_others(r, k)
            nsub = sum(1 for a, b in zip(before, r) if a != b)
            return bytes(body), (tag, bytes(r), nsub)

        # ---- eq
        self.eq_gene = None
        if len(wins) == 2 and self.sweeps:
            eq = rand_seq(rng, L + 40)
            self.eq_gene = len(targets)
            targets.append(eq)
            src = eq[EQ_AT:EQ_AT + L]
            for k, q in enumerate(wins):
                for p in places(ww):
                    r = bytearray(src)
                    r[q + p] = other(r[q + p], k)  # (where the windows overlap, the two reads of one base differ)
                    roles[("eq", k, p)] = bytes(r)
        # ---- dinuc, and the planted X windows
        self.planted = {}  # role -> (gene, pos, nmiss, passes the gate)
        plant = []
        if self.sweeps:
            for k in range(len(wins)):
                for p in places(ww):
                    w = bytearray(PAIRS[k][:1] * ww)
                    w[p] = PAIRS[k][1]
                    plant.append((("dinuc", k, p), k, bytes(w), 0 < p < ww - 1))
        if self.sweeps and self.x == "xw" and ww > 32:
            for k in range(len(wins)):
                a, b = PAIRS[k]
                w = bytearray(bytes([a]) * ww)
                w[0], w[ww - 1] = X, b    # chunk 0: XA AA; the last chunk: AC -- 3 pairs, 2 with the X chunk alone
                plant.append((("xchunk", k, 0), k, bytes(w), True))
                w = bytearray(bytes([a]) * ww)
                w[ww - 1] = X                     # the last chunk: AX; the others: AA -- 2 pairs
                plant.append((("xchunk", k, 1), k, bytes(w), False))
                w = bytearray(bytes([a]) * ww)
                w[3], w[ww - 1] = b, X    # chunk 0: AA AC CA; the last chunk: AX -- 4 pairs, 1 with the X chunk alone
                plant.append((("xchunk", k, 2), k, bytes(w), True))
        for k in range(len(wins)):
            segs, pos = [], 0
            gene = len(targets)
            for role, kk, w, ok in plant:
                if kk != k:
                    continue
                gap = rand_seq(rng, 5, b"GT")
                seg, (_, r, nsub) = planted(role, k, w)
                segs.append(gap + seg)
                self.planted[role] = (gene, pos + len(gap), nsub, ok)
                roles[role] = r
                pos += len(gap) + len(seg)
            if segs:
                targets.append(b"".join(segs))
        nrole = len(set(roles.values()))
        assert nrole == len(roles), (self.name, "two roles share a read")
        reads.update(roles.values())
        while len(reads) % 64 != 37:  # a ragged last wave-tile
            r = random_read()
            if r is not None:
                reads.add(r)
        self.targets = targets
        self.reads = sorted(reads)
        index = {r: i for i, r in enumerate(self.reads)}
        self.roles = {k: index[v] for k, v in roles.items()}
        self.total_bases = sum(map(len, targets))

    def read_of(self, role):
        return self.reads[self.roles[role]]


# the seeds for which the oracle meets the coverage conditions of tests/test_window_key_cases.py (0 unless named)
SEEDS = {"n64-xd": 2}  # (only 19 of its reads' 100 bases lie outside the windows: few reads keep an X)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def literal_hits(c, **kw):
    """Every accepted tuple of a case by oracle/literal.cpp (which raises on any error code): sorted uint32 [n, 4]."""
    from oracle import literal
    rbuf, roff = literal.concat(c.reads)
    gbuf, goff = literal.concat(c.targets)
    hits, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(c.ocfg(**kw), bloom_size=4_000_000, num_hash=20))
    return np.array(sorted(map(tuple, hits.tolist())), dtype=np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def oracle_hits(name):
    """literal_hits of the named case, made once, not to be changed."""
    hits = literal_hits(case(name))
    hits.setflags(write=False)
    return hits


def best_hits(name, mmtol):
    """The per-read best + MMTol selection of oracle_hits: sorted uint32 [n, 4]."""
    from oracle import muscato_oracle as orc
    keep = orc.best_filter(map(tuple, oracle_hits(name).tolist()), mmtol)
    return np.array(sorted(keep), dtype=np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def hot(name):
    """(read, window) of the probes whose block accepts more than SMALL_MM pairs (cases.hot_probes)."""
    from cases import hot_probes
    c = case(name)
    return frozenset(hot_probes(c.reads, c.targets, c.ocfg(MaxMatches=SMALL_MM), oracle_hits(name)))


@functools.lru_cache(maxsize=None)
def block_counts(name):
    """-> (probes, counts): the (read, window) pairs that probe, and per window key -> accepted pairs of its block,
    counted as cases.hot_probes counts them (oracle.match_direct's rule)."""
    from oracle import muscato_oracle as orc
    c = case(name)
    cfg, ww = c.ocfg(), c.ww
    valid = [[orc.window_valid(r, k, cfg) for k in range(len(c.windows))] for r in c.reads]
    counts = [{} for _ in c.windows]
    for ri, g, p, _ in oracle_hits(name).tolist():
        r, t = c.reads[ri], c.targets[g]
        for k, q in enumerate(c.windows):
            jx, key = p + q, r[q:q + ww]
            if valid[ri][k] and t[jx:jx + ww] == key and not (jx == 0 and len(r) > min(100 - (q + ww), len(t))):
                counts[k][key] = counts[k].get(key, 0) + 1
    probes = [(ri, k) for ri in range(len(c.reads)) for k in range(len(c.windows)) if valid[ri][k]]
    return probes, counts


def _mix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & (1 << 64) - 1
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & (1 << 64) - 1
    return x ^ x >> 33


def hashed_bucket(key, bits):
    """The bucket of an X-free window key in a hashed table of 2^bits buckets, as bucket_of / rec_bucket
    (kernels_common.hpp, kernels_screen.hpp) fold it: 2 bits per base (A0 C1 G2 T3), first base lowest, 64 bits at a
    time through mix64 with the chunk's (empty) mask word."""
    v = sum(ACGT.index(b) << 2 * i for i, b in enumerate(key))
    h = 0
    for c in range(0, 2 * len(key), 64):
        chunk = v >> c & (1 << 64) - 1
        h = _mix64(h ^ chunk ^ _mix64(0x9E3779B97F4A7C15 * (c + 1) & (1 << 64) - 1))
    return h >> (64 - bits)


def bucket_hot(name, bits):
    """The probes overflow_probes() has to name on a hashed table of 2^bits buckets, where the block counters are
    keyed by (window, bucket): those whose bucket's keys accept more than SMALL_MM pairs TOGETHER."""
    c = case(name)
    probes, counts = block_counts(name)
    total = {}
    for k, d in enumerate(counts):
        for key, n in d.items():
            b = (k, hashed_bucket(key, bits))
            total[b] = total.get(b, 0) + n
    return {(ri, k) for ri, k in probes if total.get((k, hashed_bucket(c.reads[ri][c.windows[k]:c.windows[k] + c.ww], bits)), 0) > SMALL_MM}


def random_case(ww, wins, L, pmatch, x, seed):
    """The random part alone, for further seeds (tests/fuzz_gpu.py windowkeys)."""
    return Case("fuzz-%d-%d" % (ww, seed), spec=(ww, wins, L, pmatch, x), seed=seed, sweeps=False)
