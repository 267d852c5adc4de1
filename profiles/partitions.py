"""Cost of a partitioned pass, one JSON record per line on stdout.

  python profiles/partitions.py cfg3        cfg3 (bench.py's synthetic 1 M x 1 kbp targets, 44.8 M unique reads) forced
                                            into 1, 2 and 4 partitions: index build (device ms, wall s), pass ms, and an
                                            order-free digest of the tuples, which must not depend on the partition count
  python profiles/partitions.py big [GBP]   a random database of GBP Gbp (default 20) with 10-kbp targets: first the
                                            unpartitioned path (one partition forced) must fail to build its index, then
                                            the automatic plan runs; the tuples of a seeded sample of planted reads are
                                            checked base by base against the packed database on the host (every tuple's
                                            nmiss recounted, every planted placement within budget found)
"""
import json
import math
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/profiles/", 1)[0])

from muscato_amd import Config, Engine, MuscatoError  # noqa: E402


def digest(h):
    """bench.py --dump-outputs' order-free digest: tuple count, per-field sums and a per-tuple hash sum, mod 2^48"""
    a = h.astype(np.uint64)
    m48 = np.uint64((1 << 48) - 1)
    with np.errstate(over="ignore"):
        x = (a[:, 0] * np.uint64(0x9E3779B97F4A7C15) ^ a[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F)
             ^ a[:, 2] * np.uint64(0x165667B19E3779F9) ^ a[:, 3] * np.uint64(0x27D4EB2F165667C5))
        sums = [int(a[:, i].sum(dtype=np.uint64) & m48) for i in range(4)] + [int((x >> np.uint64(16)).sum(dtype=np.uint64) & m48)]
    return [len(h)] + sums


def timed_match(eng, cfg):
    t0 = time.time()
    n = eng.match_device(cfg, apply_mmtol=True)
    wall = time.time() - t0
    return n, wall, eng.stats()


def cfg3():
    import torch
    from muscato_amd import synth
    device = torch.device("cuda", 0)
    wl = synth.workload_for("cfg3", 1)
    seed = synth.SEED_BASE + sum(ord(c) for c in wl.seed_key)
    targets = synth.gen_targets(wl, device, seed)
    toff = synth.offsets_for(wl.n_targets, wl.target_len, device)
    reads = synth.sort_reads(synth.gen_unique_reads(wl, targets, device, seed + 7919))
    roff = synth.offsets_for(reads.shape[0], wl.read_len, device)
    torch.cuda.synchronize()
    cfg = Config(Windows=list(wl.windows), WindowWidth=wl.window_width, PMatch=wl.pmatch, MinDinuc=wl.min_dinuc,
                 MaxReadLength=wl.read_len, MaxMatches=wl.max_matches, MMTol=wl.mmtol, MatchMode=wl.match_mode)
    nbases = wl.n_targets * wl.target_len
    with Engine(0) as eng:
        eng.load_targets_device(targets.data_ptr(), toff.data_ptr(), wl.n_targets)
        eng.load_reads_device(reads.data_ptr(), roff.data_ptr(), reads.shape[0])
        for parts in (1, 2, 4):
            eng.set_partition_bases(0 if parts == 1 else math.ceil(nbases / parts))
            n, wall_first, st1 = timed_match(eng, cfg)  # builds every partition's index
            n2, wall_second, st2 = timed_match(eng, cfg)
            h = np.zeros((n2, 4), dtype=np.uint32)
            eng.hits_to(h.ctypes.data, n2, False)
            print(json.dumps({"workload": "cfg3", "partitions": len(eng.partitions()) - 1, "tuples": n2,
                              "index_kind": st2["index_kind"], "match_variant": st2["match_variant"],
                              "first_call_wall_s": round(wall_first, 3), "first_call_index_build_ms": st1["ms_index_build"],
                              "first_call_ms_total": st1["ms_total"], "second_call_wall_s": round(wall_second, 3),
                              "second_call_index_build_ms": st2["ms_index_build"], "second_call_ms_total": st2["ms_total"],
                              "ms_select": st2["ms_select"], "digest": digest(h), "same_first": n == n2}), flush=True)


def big(gbp):
    rng = np.random.default_rng(20261016)
    tlen = 10_000
    nseq = int(gbp * 1e9) // tlen
    nbases = nseq * tlen
    t0 = time.time()
    packed = rng.integers(0, 256, size=nbases // 4 + 8, dtype=np.uint8)  # iid random bases, 2 bits each
    off = np.arange(nseq + 1, dtype=np.uint64) * np.uint64(tlen)

    def bases(start, n):
        j = np.arange(start, start + n, dtype=np.int64)
        return (packed[j >> 2] >> ((j & 3) * 2).astype(np.uint8)) & 3

    # planted reads: 100 bp from random places with 0-3 substitutions, plus random ones
    nr = 20_000
    planted = []
    reads = set()
    for i in range(nr):
        if i % 5 == 4:
            reads.add(bytes(b"ACGT"[k] for k in rng.integers(0, 4, 100)))
            continue
        g, p = int(rng.integers(0, nseq)), int(rng.integers(0, tlen - 100 + 1))
        r = bases(g * tlen + p, 100).copy()
        for q in rng.choice(np.arange(40, 100), size=int(rng.integers(0, 4)), replace=False):
            r[q] = (r[q] + 1) & 3
        s = bytes(b"ACGT"[k] for k in r)
        reads.add(s)
        planted.append((s, g, p))
    reads = sorted(reads)
    ridx = {s: i for i, s in enumerate(reads)}
    print(json.dumps({"workload": "big", "gbp": gbp, "targets": nseq, "reads": len(reads),
                      "host_gen_s": round(time.time() - t0, 1)}), flush=True)
    cfg = Config(Windows=[0, 20], WindowWidth=15, PMatch=0.97, MinDinuc=5, MaxReadLength=100, MaxMatches=1000000)
    with Engine(0) as eng:
        t0 = time.time()
        eng._check(eng._lib.musc_db_load_packed(eng._h, packed.ctypes.data, None, off.ctypes.data, nseq), "musc_db_load_packed")
        load_s = time.time() - t0
        eng.load_reads(reads)
        # the unpartitioned path: one partition forced
        eng.set_partition_bases(nbases)
        t0 = time.time()
        try:
            eng.build_index_for(cfg, 100)
            unpart = "built"
        except MuscatoError as e:
            unpart = "failed: %s" % e
        print(json.dumps({"workload": "big", "db_load_s": round(load_s, 2), "unpartitioned_index": unpart,
                          "unpartitioned_wall_s": round(time.time() - t0, 2)}), flush=True)
        if unpart == "built":
            return 2  # not above the ceiling: run a larger database
        eng.set_partition_bases(0)
        n, wall_first, st1 = timed_match(eng, cfg)
        plan = eng.partitions()
        n2, wall_second, st2 = timed_match(eng, cfg)
        h = np.zeros((n2, 4), dtype=np.uint32)
        eng.hits_to(h.ctypes.data, n2, False)
    # the sample: every tuple of the planted reads recounted on the host, every planted placement within budget found
    sample = {ridx[s]: (g, p) for s, g, p in planted[:2000]}
    sel = np.isin(h[:, 0], np.fromiter(sample, dtype=np.uint32))
    bad = found = want = 0
    for r, g, p, nm in h[sel].tolist():
        rb = np.frombuffer(reads[r], dtype=np.uint8)
        code = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), rb)
        bad += int((bases(g * tlen + p, len(rb)) != code).sum() != nm)
    have = {tuple(t) for t in h[sel][:, :3].tolist()}
    from oracle import muscato_oracle as orc
    for r, (g, p) in sample.items():
        rb = np.frombuffer(reads[r], dtype=np.uint8)
        code = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), rb)
        nmiss = int((bases(g * tlen + p, 100) != code).sum())
        # budget int((1 - PMatch) * 100) as the library evaluates it (3 here); a window must pass MinDinuc (position 0
        # has the literal-100 rule: skipped)
        if nmiss <= int((1.0 - cfg.PMatch) * 100) and p > 0 and max(orc.count_dinuc(reads[r][0:15]), orc.count_dinuc(reads[r][20:35])) >= 5:
            want += 1
            found += (r, g, p) in have
    print(json.dumps({"workload": "big", "partitions": len(plan) - 1, "plan_first_targets": plan[:8],
                      "index_kind": st2["index_kind"], "tuples": n2, "same_first": n == n2,
                      "first_call_wall_s": round(wall_first, 2), "index_build_ms": st1["ms_index_build"],
                      "first_call_ms_total": st1["ms_total"], "second_call_wall_s": round(wall_second, 2),
                      "second_call_ms_total": st2["ms_total"], "sample_tuples": int(sel.sum()),
                      "sample_tuples_with_wrong_nmiss": bad, "planted_within_budget": want, "planted_found": found}),
          flush=True)
    return 0 if bad == 0 and found == want else 1


if __name__ == "__main__":
    if sys.argv[1] == "cfg3":
        cfg3()
    else:
        sys.exit(big(float(sys.argv[2]) if len(sys.argv) > 2 else 20.0))
