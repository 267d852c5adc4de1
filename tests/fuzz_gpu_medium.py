"""Medium-scale fuzz of the GPU path against the literal C++ oracle (not collected by pytest):
`python tests/fuzz_gpu_medium.py LO HI` draws one random configuration per seed -- 1-5 windows,
WindowWidth 6-20 (direct and hashed index), PMatch 0.9-1, MinDinuc 0-6, MMTol 0-3, X rate 0 / 0.1 % /
1 %, read length 40-200 (180 and 200: records of 16 words; half of the runs of 150 bases and more keep their windows
within 200 bases of context, so that they stay on the fused path), MaxMatches 25 / 20 000 / 10^6 -- over a few thousand reads and a few hundred targets, and compares all
accepted tuples (the oracle without truncation), the best+MMTol selection and the MaxMatches verdict (every probe of
an overflowing oracle block named by overflow_probes(); a verdict without one is counted apart), and tallies
Engine.last_instance() per run: the totals line lists the kernel instances that ran and those with no run
(profiles/r06_fuzz_instance_totals.txt).  Round 1: seeds 0..85000, no mismatch (28 min on
one MI355X); round 2 (both index kinds, as each configuration selects): seeds 0..56000 with k_match,
0..80000 with k_match_d where a configuration has at most two windows, and 0..20000 with
MUSC_FUZZ_READS_X=1 (X in the reads only): no mismatch; round 3 (k_match_t, wide and line buckets): seeds
0..22000 and 0..9000 with MUSC_FUZZ_READS_X=1, no mismatch, all four index kinds used; round 4: profiles/r04_fuzz_totals.txt (k_match_t with the
eight-lanes-per-line fetch, and k_match_g with MUSC_MATCH=dma).

MUSC_FUZZ_SPEC=1 draws only the geometry of the specialised fused kernels (SpecGeom<1>: WindowWidth 15, Windows 0,20,
MinDinuc 5) on a direct table (MUSC_DEBUG_CTX_DIRECT=1, set here), with ragged reads of at most 100 bases and random
PMatch, MMTol, MatchMode and MaxMatches; a database serves a block of SPEC_BLOCK seeds (each one a 2^30-bucket table
build).  Every tuple is compared with the untruncated oracle, n_overflow_blocks with the oracle's block counts, and
a configuration that does not run variant 3 (5 with MUSC_MATCH=dma) counts as bad.  Totals: profiles/r05_fuzz_spec_totals.txt."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from oracle import literal
from oracle import muscato_oracle as orc
from muscato_amd import Config, Engine, sorted_hits
from muscato_amd.api import instance_name, instances
from cases import hot_probes


# MUSC_FUZZ_READS_X=1: X in the reads only (an X-free database: with at most two windows and reads
# of at most 112 bases those runs take k_match_d's RX path whenever every read's X fit its xpos word)
READS_X_ONLY = bool(os.environ.get("MUSC_FUZZ_READS_X"))
# MUSC_FUZZ_DB_X=1: X in the database only, single bases and runs (N stretches), the reads sampled over
# them get random bases there -- those runs stay on context buckets (k_match_t<.., XM = 2>: flagged
# entries compared through the mask plane); =2: the reads keep the target's X where it falls outside
# their windows (at most three per read), so read X meets target X
DB_X = int(os.environ.get("MUSC_FUZZ_DB_X", "0"))
KINDS = {0: 0, 1: 0, 2: 0, 3: 0}
# MUSC_FUZZ_SPEC=1: the specialised kernels' geometry only (see the docstring)
SPEC = bool(os.environ.get("MUSC_FUZZ_SPEC"))
SPEC_BLOCK = 100
# MUSC_FUZZ_SECONDS=S: stop after the seed that ends past S seconds (the totals line names the seeds that ran)
SECONDS = float(os.environ.get("MUSC_FUZZ_SECONDS", "0"))
BLOCKS = {"overflow": 0, "extra verdict": 0}  # configurations with an overflowing block / a verdict without one
INSTANCES = {}  # runs per kernel instance (Engine.last_instance(): a two-kernel pass counts for its screen and its confirm instance)


def case(seed):
    rng = np.random.default_rng(seed)
    L = int(rng.choice([40, 60, 100, 120, 150, 180, 200]))
    ww = int(rng.integers(6, 21))
    nwin = int(rng.integers(1, 6))
    wins = sorted(int(x) for x in rng.choice(np.arange(0, max(1, L - ww - 5)), size=nwin, replace=False))
    if rng.random() < 0.5:
        wins[0] = 0
    if L >= 150 and rng.random() < 0.5:  # windows within 200 - L bases of each other: wide context buckets hold such a run
        nwin = min(nwin, 201 - L)
        w0 = int(rng.integers(0, L - ww - (200 - L)))
        wins = sorted(int(x) for x in w0 + rng.choice(np.arange(0, 201 - L), size=nwin, replace=False))
    cfg = orc.Config(Windows=wins, WindowWidth=ww, PMatch=float(rng.choice([1.0, 0.97, 0.95, 0.92, 0.9])),
                     MinDinuc=int(rng.integers(0, 7)), MaxReadLength=L, MaxMatches=int(rng.choice([25, 20000, 1000000])),
                     MMTol=int(rng.integers(0, 4)), MatchMode=str(rng.choice(["best", "first"])))
    nt, tlen, nr = int(rng.integers(50, 400)), int(rng.integers(L + 5, 800)), int(rng.integers(500, 6000))
    xrate = float(rng.choice([0.0, 0.001, 0.01]))
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    T = bases[rng.integers(0, 4, size=(nt, tlen))]
    ncopy = nt // 4
    T[nt - ncopy:] = T[rng.integers(0, nt - ncopy, size=ncopy)]
    sub = rng.random((ncopy, tlen)) < 0.03
    T[nt - ncopy:][sub] = bases[rng.integers(0, 4, size=int(sub.sum()))]
    if DB_X:
        xrate = float(rng.choice([0.001, 0.004, 0.015]))
        run = int(rng.choice([1, 1, 4, 40]))
        starts = rng.random(T.shape) < xrate / run
        for d in range(run):
            T[:, d:][starts[:, :tlen - d]] = ord("X")
    elif xrate and not READS_X_ONLY:
        T[rng.random(T.shape) < xrate] = ord("X")
    g = rng.integers(0, nt, size=nr)
    p = rng.integers(0, tlen - L + 1, size=nr)
    p[rng.random(nr) < 0.05] = 0
    p[rng.random(nr) < 0.05] = tlen - L
    R = T[g[:, None], p[:, None] + np.arange(L)[None, :]].copy()
    sub = rng.random(R.shape) < float(rng.choice([0.0, 0.01, 0.03]))
    R[sub] = bases[rng.integers(0, 4, size=int(sub.sum()))]
    if DB_X:
        isx = R == ord("X")
        keep = np.zeros_like(isx)
        if DB_X == 2:  # a read keeps the target's X outside its windows, three at most
            inwin = np.zeros(L, dtype=bool)
            for q in wins:
                inwin[q:q + ww] = True
            keep = isx & ~inwin[None, :]
            keep &= np.cumsum(keep, axis=1) <= 3
        fill = isx & ~keep
        R[fill] = bases[rng.integers(0, 4, size=int(fill.sum()))]
        xrate = 0.0
    if READS_X_ONLY:  # X (N in the FASTQ) in the reads alone, at rates where most reads keep a few of them
        xrate = float(rng.choice([0.002, 0.005, 0.02]))
    if xrate:
        R[rng.random(R.shape) < xrate] = ord("X")
    lens = rng.integers(max(ww, L // 2), L + 1, size=nr)
    reads = sorted({bytes(r[:n]) for r, n in zip(R, lens)})
    return cfg, reads, [bytes(t) for t in T]


def spec_targets(block):
    """The database of a block of SPEC_BLOCK seeds: random targets, a quarter of them mutated copies, a motif in up to
    sixty of them (heavy blocks), and some shorter than 100 bases."""
    rng = np.random.default_rng(1_000_003 + block)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    nt, tlen = int(rng.integers(100, 800)), int(rng.integers(120, 1000))
    T = bases[rng.integers(0, 4, size=(nt, tlen))]
    ncopy = nt // 4
    T[nt - ncopy:] = T[rng.integers(0, nt - ncopy, size=ncopy)]
    sub = rng.random((ncopy, tlen)) < 0.03
    T[nt - ncopy:][sub] = bases[rng.integers(0, 4, size=int(sub.sum()))]
    motif = bases[rng.integers(0, 4, size=110)]
    for i in rng.choice(nt - ncopy, size=int(rng.integers(0, 61)), replace=False):
        p = int(rng.integers(0, tlen - 110 + 1))
        T[i, p:p + 110] = motif
    short = [bytes(bases[rng.integers(0, 4, size=int(rng.integers(15, 100)))]) for _ in range(int(rng.integers(0, 40)))]
    return [bytes(t) for t in T] + short


def spec_case(seed, targets):
    rng = np.random.default_rng(seed)
    cfg = orc.Config(Windows=[0, 20], WindowWidth=15, PMatch=float(rng.choice([1.0, 0.97, 0.95, 0.92, 0.9, 0.8])), MinDinuc=5,
                     MaxReadLength=100, MaxMatches=int(rng.choice([3, 10, 50, 1000, 20000, 1000000])),
                     MMTol=int(rng.integers(0, 4)), MatchMode=str(rng.choice(["best", "first"])))
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    nr = int(rng.integers(1, 6000))
    shape = int(rng.integers(0, 3))  # every read 100 bases | one length 49-100 | ragged 5-100
    L1 = int(rng.integers(49, 101))
    lens = np.full(nr, 100) if shape == 0 else np.full(nr, L1) if shape == 1 else rng.integers(5, 101, size=nr)
    lens[0] = max(49, int(lens[0]))  # (8-word records: the specialised instances' layout)
    rate = float(rng.choice([0.0, 0.01, 0.03]))
    reads = set()
    for L in lens:
        L = int(L)
        fit = [t for t in targets if len(t) >= L]
        if rng.random() < 0.1 or not fit:
            reads.add(bytes(bases[rng.integers(0, 4, size=L)]))
            continue
        t = fit[int(rng.integers(0, len(fit)))]
        u = rng.random()
        p = 0 if u < 0.05 else len(t) - L if u < 0.1 else int(rng.integers(0, len(t) - L + 1))
        r = np.frombuffer(t[p:p + L], dtype=np.uint8).copy()
        sub = rng.random(L) < rate
        r[sub] = bases[rng.integers(0, 4, size=int(sub.sum()))]
        reads.add(bytes(r))
    cfg.MaxReadLength = max(len(r) for r in reads)
    return cfg, sorted(reads)


def main():
    lo, hi = int(sys.argv[1]), int(sys.argv[2])
    if SPEC:
        os.environ["MUSC_DEBUG_CTX_DIRECT"] = "1"
        os.environ.pop("MUSC_NO_SPEC", None)
    e = Engine(0)
    bad, t0 = 0, time.time()
    block, targets, loaded = None, None, None
    for seed in range(lo, hi):
        if SECONDS and time.time() - t0 > SECONDS:
            hi = seed
            break
        if SPEC:
            if seed // SPEC_BLOCK != block:
                block = seed // SPEC_BLOCK
                targets = spec_targets(block)
            c, reads = spec_case(seed, targets)
        else:
            c, reads, targets = case(seed)
        rbuf, roff = literal.concat(reads)
        gbuf, goff = literal.concat(targets)
        oc = orc.Config(**dict(c.__dict__, MaxMatches=2 ** 31 - 1))  # (every tuple, no truncation)
        exp, _, _ = literal.match_arrays(rbuf, roff, gbuf, goff, literal.make_params(oc, bloom_size=16_000_000, num_hash=6, nthreads=8))
        if targets is not loaded:  # (SPEC: one database, one table build, per block of seeds)
            e.load_targets(targets)
            loaded = targets
        e.load_reads(reads)
        k = Config(Windows=list(c.Windows), WindowWidth=c.WindowWidth, PMatch=c.PMatch, MinDinuc=c.MinDinuc,
                   MaxReadLength=c.MaxReadLength, MaxMatches=c.MaxMatches, MMTol=c.MMTol, MatchMode=c.MatchMode)
        got = sorted_hits(e.match(k, apply_mmtol=False))
        ok = got.shape == exp.shape and bool((got == exp).all())
        st = e.stats()
        # n_overflow_blocks is an upper bound (hashed block counters): every probe of an overflowing block must be
        # named; a verdict without an oracle overflow is counted apart
        hot = hot_probes(reads, targets, c, exp)
        probes = set(map(tuple, e.overflow_probes().tolist())) if st["n_overflow_blocks"] else set()
        ok = ok and hot <= probes and (st["n_overflow_blocks"] >= 1 or not hot)
        if SPEC:
            ok = ok and st["match_variant"] == (5 if os.environ.get("MUSC_MATCH") == "dma" else 3)
        BLOCKS["overflow"] += bool(hot)
        BLOCKS["extra verdict"] += bool(probes) and not hot
        best = sorted_hits(e.match(k, apply_mmtol=True))
        eb = np.array(sorted(orc.best_filter([tuple(int(x) for x in r) for r in exp], c.MMTol)), dtype=np.uint32).reshape(-1, 4)
        ok = ok and best.shape == eb.shape and bool((best == eb).all())
        KINDS[e.stats()["index_kind"]] += 1
        li = e.last_instance()
        for d in (li["match"], li["screen"], li["confirm"]):
            if d is not None:
                INSTANCES[instance_name(d)] = INSTANCES.get(instance_name(d), 0) + 1
        if not ok:
            bad += 1
            print("MISMATCH seed", seed, c, len(reads), len(targets), len(got), len(exp), flush=True)
        if seed % 50 == 0:
            print("seed", seed, "hits", len(exp), "elapsed %.0fs" % (time.time() - t0), flush=True)
    print("fuzz_medium", lo, hi, "bad", bad, "in %.0fs" % (time.time() - t0), "index kinds used", KINDS, "MaxMatches", BLOCKS,
          "(reads-only X)" if READS_X_ONLY else "(database X, mode %d)" % DB_X if DB_X else
          "(SpecGeom<1> on a direct table%s)" % (", MUSC_MATCH=dma" if os.environ.get("MUSC_MATCH") == "dma" else "")
          if SPEC else "")
    print("instances run:", ", ".join("%s x %d" % kv for kv in sorted(INSTANCES.items())))
    print("instances with no run:", ", ".join(sorted(set(map(instance_name, instances())) - set(INSTANCES))) or "none")


if __name__ == "__main__":
    main()
