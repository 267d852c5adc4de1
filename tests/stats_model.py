"""A CPU model of musc_stats (include/muscato_hip.h): what the counters and the algorithmic bytes of a pass must be,
computed from the oracle's own pieces (orc.window_valid, orc._kmer_index, orc.nmiss_allowed and the fit rule of
orc.match_direct) and never from the library.  A plain helper module: tests/test_stats_model.py checks it without a
GPU, tests/test_gpu_stats.py and tests/test_gpu_spec.py hold the kernels' tallies and the host's sums to it.

The model is exact where the table is direct (bucket = key) and reads and targets hold only ACGT, with the one
exception of n_descriptors on 64-byte buckets, which it brackets (which entries of a bucket arrive inline, and so
which placements found through two adjacent windows share a descriptor, depends on the order the index build's atomics
ran in).  On a hashed table the candidates -- and on the fused paths the pairs -- are lower bounds: colliding keys are
walked and compared too."""
from collections import Counter

import numpy as np

from oracle import muscato_oracle as orc

KINDS = ("ctx", "ctx_wide", "classic64", "lines")
INDEX_KIND = {"ctx": 1, "ctx_wide": 2, "classic64": 0, "lines": 3}  # musc_stats.index_kind
INLINE = {"ctx": 3, "ctx_wide": 2, "classic64": 3, "lines": 7}      # entries that arrive with the bucket
ENTRY_BYTES = {"ctx": 40, "ctx_wide": 60}                           # an overflow entry of a context bucket
XPOS_MAX = {"ctx": 4, "ctx_wide": 3}                                # X of a read its xpos word lists
BUCKET_BYTES = 128                                                  # a context bucket is one cache line
FLANK = 8                                                           # bases either side of the window the screen compares
X = ord("X")


def fits(q1, ww, rlen, tlen, jx):
    """The fit rule of orc.match_direct for a candidate at target offset jx of a read window at q1: the placement
    starts inside the target, and ends inside it -- at jx == 0 by the rule with the literal 100."""
    p = jx - q1
    if p < 0:
        return False
    if jx == 0:
        return rlen <= min(100 - (q1 + ww), tlen)
    return p + rlen <= tlen


def flank_mismatches(read, q1, ww, target, jx):
    """Mismatches among the min(q1, 8) read bases left of the window and the min(len - q2, 8) right of it against
    the target (the flank filter of the two-kernel path; the placement fits, so every base compared exists)."""
    q2 = q1 + ww
    nl = min(q1, FLANK)
    nr = min(max(len(read) - q2, 0), FLANK)
    return (sum(1 for i in range(1, nl + 1) if read[q1 - i] != target[jx - i]) +
            sum(1 for i in range(nr) if read[q2 + i] != target[jx + ww + i]))


def ctx_entries_bytes(n, wide):
    """Bytes of the overflow array of a context table for n entries: three 40-byte entries (wide: two of 60 bytes)
    per 128-byte line."""
    return ((n + 1) // 2 if wide else (n + 2) // 3) * 128


def _index(targets, ww, kind, first, last, wanted):
    """key -> [(gene, jx)] over targets [first, last) with global target numbers, for the keys in `wanted` (the read
    windows that probe): orc._kmer_index target by target (a window that crosses a target end is never indexed),
    less -- in context buckets -- the windows that hold an X."""
    out = {}
    for g in range(first, last):
        for key, ent in orc._kmer_index(targets[g:g + 1], ww).items():
            if key not in wanted or (kind in ("ctx", "ctx_wide") and X in key):
                continue
            out.setdefault(key, []).extend((g, jx) for _, jx in ent)
    return out


def expected(reads, targets, cfg, kind, accepted, parts=None, apply_mmtol=False):
    """The counters of one pass over `reads` (as loaded: sorted, unique) and `targets` with the oracle Config `cfg` on
    index `kind` ("ctx": narrow context buckets, "ctx_wide", "classic64", "lines"); `accepted` = every accepted
    (read, gene, pos, nmiss) tuple, from oracle.literal without truncation; parts = the partition plan as target
    numbers (Engine.partitions(): n + 1 boundaries), None = one partition.

    -> dict of the musc_stats fields the model knows (exact on a direct table with ACGT only), with
    n_descriptors_lo / n_descriptors_hi instead of n_descriptors on 64-byte buckets, plus the quantities the fixture
    checks read: see the keys set at the end."""
    assert kind in KINDS
    fused = kind in ("ctx", "ctx_wide")
    ww, W = cfg.WindowWidth, len(cfg.Windows)
    nin = INLINE[kind]
    parts = [0, len(targets)] if parts is None else list(parts)
    npart = len(parts) - 1
    acc = [tuple(int(v) for v in h) for h in (accepted.tolist() if hasattr(accepted, "tolist") else accepted)]
    m = Counter()
    # ---- the probes: (read, window) pairs that pass the length and MinDinuc gates
    probes = []
    for ri, r in enumerate(reads):
        nx = r.count(b"X")
        for k, q1 in enumerate(cfg.Windows):
            if len(r) < q1 + ww:
                m["len_rejected"] += 1
                continue
            if not orc.window_valid(r, k, cfg):
                m["dinuc_rejected"] += 1
                continue
            if fused and (X in r[q1:q1 + ww] or nx > XPOS_MAX[kind]):
                m["x_windows"] += 1  # a read window that holds an X takes no part on the fused paths
                continue
            probes.append((ri, k, q1))
    m["n_read_windows"] = len(probes) * npart
    wanted = {reads[ri][q1:q1 + ww] for ri, _, q1 in probes}
    survivors = []  # two-kernel path: (read, window, gene, pos) that fit and pass the flank filter
    for pi in range(npart):
        idx = _index(targets, ww, kind, parts[pi], parts[pi + 1], wanted)
        for ri, k, q1 in probes:
            r = reads[ri]
            ent = idx.get(r[q1:q1 + ww], ())
            m["n_candidates"] += len(ent)
            m["n_overflow_entries"] += max(0, len(ent) - nin)
            m["empty_probes"] += not ent
            budget = orc.nmiss_allowed(cfg.PMatch, len(r))
            for g, jx in ent:
                t = targets[g]
                if not fits(q1, ww, len(r), len(t), jx):
                    m["unfit_before_start" if jx < q1 else "unfit_at_jx0" if jx == 0 else "unfit_past_end"] += 1
                    continue
                m["fitting"] += 1
                if fused:
                    continue
                if flank_mismatches(r, q1, ww, t, jx) > budget:
                    m["flank_rejected"] += 1
                    continue
                survivors.append((ri, k, g, jx - q1))
    out = {"n_reads": len(reads), "n_read_windows": m["n_read_windows"], "n_candidates": m["n_candidates"],
           "index_kind": INDEX_KIND[kind], "n_accepted": len(set(acc)),
           "n_hits": len(orc.best_filter(acc, cfg.MMTol)) if apply_mmtol else len(set(acc))}
    L = max(map(len, reads)) if reads else 0
    rec_b = (2 * L + 7) // 8
    # the tuples the passes write: every partition's pass selects (apply_mmtol) among its own targets' tuples
    staged = 0
    for pi in range(npart):
        mine = {h for h in acc if parts[pi] <= h[1] < parts[pi + 1]}
        staged += len(orc.best_filter(mine, cfg.MMTol)) if apply_mmtol else len(mine)
    out["staged_tuples"] = staged
    out["record_bytes"] = rec_b  # ceil(2L/8), L = the longest loaded read
    if fused:
        ent_b = out["entry_bytes"] = ENTRY_BYTES[kind]
        out["n_pairs"] = m["fitting"]
        out["n_descriptors"] = 0
        out["n_overflow_entries"] = m["n_overflow_entries"]
        out["confirm_bytes"] = 0
        out["confirm_launches"] = 0
        # per partition: every read's record + a bucket line per probe + the overflow entries walked + the tuples staged
        out["match_bytes"] = (npart * len(reads) * rec_b + BUCKET_BYTES * out["n_read_windows"] +
                              ent_b * out["n_overflow_entries"] + 16 * staged)
        out["match_bytes_strict"] = (npart * len(reads) * rec_b + 8 * out["n_read_windows"] + ent_b * out["n_candidates"] +
                                     16 * staged)
    else:
        out["n_pairs"] = len(survivors)
        out["n_overflow_entries"] = 0
        out["match_bytes"] = out["match_bytes_strict"] = 0
        out["match_launches"] = 0
        out["descriptor_bytes"] = 12 + 2 * rec_b + 1  # confirm_bytes = this per descriptor + 16 per tuple staged
        if kind == "lines":
            out["n_descriptors"] = len(survivors)
        else:
            # one descriptor may stand for windows 2j and 2j + 1 of a read that found the same placement
            out["n_descriptors_lo"] = len({(ri, k // 2, g, p) for ri, k, g, p in survivors})
            out["n_descriptors_hi"] = len(survivors)
    # ---- what the fixture checks read
    per_read = Counter(h[0] for h in set(acc))
    out["model"] = {
        "len_rejected": m["len_rejected"], "dinuc_rejected": m["dinuc_rejected"], "x_windows": m["x_windows"],
        "empty_probes": m["empty_probes"], "fitting": m["fitting"], "unfit_before_start": m["unfit_before_start"],
        "unfit_at_jx0": m["unfit_at_jx0"], "unfit_past_end": m["unfit_past_end"], "flank_rejected": m["flank_rejected"],
        "multi_tuple_reads": sum(1 for v in per_read.values() if v > 1),
        "max_tuples_per_read": max(per_read.values()) if per_read else 0,
        "both_windows": len(survivors) - len({(ri, g, p) for ri, k, g, p in survivors}),
        "accepted_triples": len({(ri, g, p) for ri, g, p, _ in acc}),
        # (two-kernel path) accepted placements the flank filter would have dropped: it never drops one
        "accepted_not_surviving": 0 if fused else len({(ri, g, p) for ri, g, p, _ in acc} - {(ri, g, p) for ri, _, g, p in survivors}),
    }
    return out


def index_bytes(targets, cfg, kind, first=0, last=None):
    """musc_stats.index_bytes of a DIRECT context table over targets [first, last): the table's 4^ww buckets and its
    end sentinel, and the lines of the overflow array, which is allocated for the overflow entries + 16.  The build's
    temporaries are released when the build ends and are not counted."""
    assert kind in ("ctx", "ctx_wide")
    last = len(targets) if last is None else last
    per_key = Counter()
    for key, ent in orc._kmer_index(targets[first:last], cfg.WindowWidth).items():
        if X not in key:
            per_key[key] = len(ent)
    novf = sum(max(0, n - INLINE[kind]) for n in per_key.values())
    return (4 ** cfg.WindowWidth + 1) * BUCKET_BYTES + ctx_entries_bytes(novf + 16, kind == "ctx_wide")


def uniform_batches(nreads, batch):
    return (nreads + batch - 1) // batch


def as_hits(hits):
    """A set of oracle tuples as the sorted uint32 [n, 4] array the GPU tests compare with."""
    return np.array(sorted(hits), dtype=np.uint32).reshape(-1, 4)
