"""Long-running fuzz of the GPU path (not collected by pytest): `python tests/fuzz_gpu.py LO HI`
runs make_case(seed) for seed in [LO, HI) through one Engine -- all accepted tuples, best+MMTol
three times (the later passes are sync-free; with MUSC_GRAPH=1 the last is a graph replay), and the same reads through the GPU read prep -- against
the Python oracle.  Round 1: seeds 0..100000 with the final kernels, no mismatch (270 s on one MI355X); round 2 (context
buckets wherever a case fits them): seeds 0..90000 with k_match and again with k_match_d (up to two
windows; k_match otherwise), no mismatch (308 s each); 30000 of them with MUSC_GRAPH=1; round 3 (k_match_t): seeds 0..60000, no mismatch (153 s).
`python tests/fuzz_gpu.py walk LO HI [STEPS]` runs the random walks of tests/walk_cases.py instead (one context per seed).
`python tests/fuzz_gpu.py windowkeys LO HI` runs further seeds of the random part of tests/window_key_cases.py (WindowWidth 16
to 128)."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cases import make_case
from oracle import muscato_oracle as orc
from muscato_amd import Engine, Config, sorted_hits
if sys.argv[1] == "walk":
    # `python tests/fuzz_gpu.py walk LO HI [STEPS]`: the walks of tests/walk_cases.py for seeds [LO, HI) on one context each,
    # every step held to the oracle (tests/test_gpu_walk.py runs the committed seeds); ends at the first walk that fails
    import walk_cases as wc
    from test_gpu_walk import run_walk
    lo, hi = int(sys.argv[2]), int(sys.argv[3])
    nsteps = int(sys.argv[4]) if len(sys.argv) > 4 else wc.STEPS
    tally, t0 = {}, time.time()
    for seed in range(lo, hi):
        run_walk(wc.generate(seed, nsteps), "seed %d" % seed, wc.batch64_of(seed), tally)
        if seed % 20 == 0: print("seed", seed, "elapsed %.0fs" % (time.time() - t0), flush=True)
    print("fuzz walk", lo, hi, "no mismatch in %.0fs" % (time.time() - t0))
    print("passes per path class:", ", ".join("%s x %d" % (c, tally.get(c, 0)) for c in wc.CLASSES))
    print("passes that repeated exact:", tally.get("exact rerun", 0), "-- with several batches:", tally.get("batches > 1", 0))
    sys.exit(0)
if sys.argv[1] == "windowkeys":
    # `python tests/fuzz_gpu.py windowkeys LO HI`: further seeds of the random part of tests/window_key_cases.py (window
    # keys of 16 to 128 bases, every X variant) on the index the library picks and under MUSC_INDEX=classic and =lines,
    # against oracle/literal.cpp (tests/test_gpu_window_keys.py runs the committed cases)
    import window_key_cases as wk
    from test_gpu_window_keys import to_cfg
    geoms = sorted({(s[0], s[1], s[2], s[3]) for s in wk.SPECS.values() if s[0] <= 128})
    lo, hi = int(sys.argv[2]), int(sys.argv[3])
    e, bad, t0 = Engine(0), 0, time.time()
    for seed in range(lo, hi):
        ww, wins, L, pm = geoms[seed % len(geoms)]
        c = wk.random_case(ww, wins, L, pm, ("", "xr", "xd", "xw")[seed // len(geoms) % 4], seed)
        full = wk.literal_hits(c)
        best = np.array(sorted(orc.best_filter(map(tuple, full.tolist()), wk.MMTOL)), dtype=np.uint32).reshape(-1, 4)
        for index in (None, "classic", "lines"):
            os.environ.pop("MUSC_INDEX", None)
            if index: os.environ["MUSC_INDEX"] = index
            e.reload_env(); e.load_targets(c.targets); e.load_reads(c.reads)
            for mode, exp in ((False, full), (True, best), (True, best)):
                got = sorted_hits(e.match(to_cfg(c), apply_mmtol=mode))
                if got.shape != exp.shape or (got != exp).any():
                    bad += 1
                    print("MISMATCH seed", seed, c.ww, c.windows, c.lmax, repr(c.x), "index", index, "apply_mmtol", mode, len(got), len(exp), flush=True)
        if seed % 50 == 0: print("seed", seed, "elapsed %.0fs" % (time.time() - t0), flush=True)
    os.environ.pop("MUSC_INDEX", None)
    print("fuzz windowkeys", lo, hi, "bad", bad, "in %.0fs" % (time.time() - t0))
    sys.exit(1 if bad else 0)
lo, hi = int(sys.argv[1]), int(sys.argv[2])
e = Engine(0)
bad = 0
t0 = time.time()
for seed in range(lo, hi):
    ocfg, reads, targets = make_case(seed)
    full = sorted(orc.match_direct(reads, targets, ocfg))
    best = sorted(orc.best_filter(full, ocfg.MMTol))
    e.load_targets(targets); e.load_reads(reads)
    cfg = Config(Windows=list(ocfg.Windows), WindowWidth=ocfg.WindowWidth, PMatch=ocfg.PMatch, MinDinuc=ocfg.MinDinuc, MaxReadLength=ocfg.MaxReadLength, MaxMatches=ocfg.MaxMatches, MMTol=ocfg.MMTol, MatchMode=ocfg.MatchMode)
    for mode, exp in ((False, full), (True, best), (True, best), (True, best)):  # sizing, sized, (MUSC_GRAPH=1: captured, replayed)
        got = [tuple(int(x) for x in r) for r in sorted_hits(e.match(cfg, apply_mmtol=mode))]
        if got != exp:
            bad += 1
            print("MISMATCH seed", seed, "apply_mmtol", mode, len(got), len(exp), flush=True)
    # the same reads through the GPU prep, shuffled with duplicates
    raw = list(reads) + list(reads[::3])
    rng = np.random.default_rng(seed); rng.shuffle(raw)
    order, ustart = e.sort_unique_reads(raw)
    if [raw[i] for i in order[ustart[:-1]]] != list(reads):
        bad += 1; print("PREP MISMATCH seed", seed, flush=True)
    got = [tuple(int(x) for x in r) for r in sorted_hits(e.match(cfg, apply_mmtol=False))]
    if got != full:
        bad += 1; print("MISMATCH after prep, seed", seed, flush=True)
    if seed % 200 == 0: print("seed", seed, "elapsed %.0fs" % (time.time() - t0), flush=True)
print("fuzz", lo, hi, "bad", bad, "in %.0fs" % (time.time() - t0))
