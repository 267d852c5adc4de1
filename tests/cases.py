"""Seeded random test cases shared by the oracle cross-check and the GPU parity tests."""
import random

from oracle import muscato_oracle as orc


def rand_seq(rng, n, alphabet):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet):
    b = bytearray(s)
    for i in range(len(b)):
        if rng.random() < rate:
            b[i] = rng.choice(alphabet)
    return bytes(b)


def make_case(seed):
    """Small randomized (cfg, unique sorted reads, targets).

    Alphabet with X for every third seed; 1-3 windows (often starting at 0);
    ragged read lengths incl. reads shorter than a window; reads sampled from
    targets at position 0, at the target end and in between, with 0-8 %
    substitutions; 30 % of targets are mutated copies of earlier ones
    (multi-map).  Every window is guaranteed at least one long-enough read (the
    reference exits otherwise, cmd/muscato_window_reads/main.go:143-151).
    """
    rng = random.Random(seed)
    alphabet = b"ACGT" if seed % 3 else b"ACGTX"
    ww = rng.choice([4, 5, 8, 12, 15])
    nwin = rng.choice([1, 2, 3])
    windows = sorted(rng.sample(range(0, 40), nwin))
    if rng.random() < 0.6:
        windows[0] = 0
    maxlen = rng.choice([60, 100, 120])
    cfg = orc.Config(Windows=windows, WindowWidth=ww,
                     PMatch=rng.choice([1.0, 0.97, 0.93, 0.9, 0.8, 0.7]),
                     MinDinuc=rng.choice([0, 1, 3, 5]), MaxReadLength=maxlen,
                     MaxMatches=1000000, MMTol=rng.choice([0, 1, 3]),
                     MatchMode=rng.choice(["best", "first"]))
    ngene = rng.randint(3, 25)
    targets = []
    for g in range(ngene):
        if targets and rng.random() < 0.3:
            targets.append(mutate(rng, rng.choice(targets), 0.03, alphabet))
        else:
            targets.append(rand_seq(rng, rng.randint(10, 260), alphabet))
    reads = set()
    for _ in range(rng.randint(5, 80)):
        t = rng.choice(targets)
        L = rng.randint(max(1, ww - 2), maxlen)
        u = rng.random()
        if u < 0.15 or len(t) < L:
            r = rand_seq(rng, L, alphabet)
        else:
            p = 0 if u < 0.35 else rng.randint(0, len(t) - L)
            if u > 0.9:
                p = len(t) - L  # flush with the target end
            r = mutate(rng, t[p:p + L], rng.choice([0, 0.01, 0.03, 0.08]), alphabet)
        reads.add(r)
    reads.add(rand_seq(rng, maxlen, alphabet))  # every window has a valid read
    return cfg, sorted(reads), targets


def hot_probes(reads, targets, cfg, full):
    """(read, window) of the probes whose (window, key) block accepts more than cfg.MaxMatches pairs, counted as
    orc.match_direct counts them, from `full`, every accepted (read, gene, pos, nmiss) tuple without truncation: a
    tuple counts in window k's block when the read's window k passes its gate, equals the target's bases at
    jx = pos + q1 and that window's fit rule holds (at jx = 0 the literal 100)."""
    ww = cfg.WindowWidth
    counts = [{} for _ in cfg.Windows]
    valid = [[orc.window_valid(r, k, cfg) for k in range(len(cfg.Windows))] for r in reads]
    for ri, g, p, _ in (full.tolist() if hasattr(full, "tolist") else full):
        r, t = reads[ri], targets[g]
        for k, q1 in enumerate(cfg.Windows):
            jx = p + q1
            key = r[q1:q1 + ww]
            if not valid[ri][k] or t[jx:jx + ww] != key:
                continue
            if jx == 0 and len(r) > min(100 - (q1 + ww), len(t)):
                continue
            counts[k][key] = counts[k].get(key, 0) + 1
    hot = [{key for key, n in d.items() if n > cfg.MaxMatches} for d in counts]
    return {(ri, k) for ri, r in enumerate(reads) for k, q1 in enumerate(cfg.Windows) if valid[ri][k] and r[q1:q1 + ww] in hot[k]}


def check_groups(reads, order, ustart):
    """order/ustart describe exactly sorted(set(reads)) with stable groups."""
    uniq = sorted(set(reads))
    assert len(ustart) == len(uniq) + 1 and ustart[0] == 0 and ustart[-1] == len(reads)
    assert sorted(order.tolist()) == list(range(len(reads)))
    for g, u in enumerate(uniq):
        grp = order[ustart[g]:ustart[g + 1]].tolist()
        assert grp, "empty group"
        assert all(reads[i] == u for i in grp)
        assert grp == sorted(grp), "ties must keep input order"
    return uniq
