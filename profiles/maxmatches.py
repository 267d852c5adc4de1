#!/usr/bin/env python3
"""The MaxMatches replay on the host against the replay on the device.

Workload: profiles/e2e.py's shape (2 M reads x 100 k targets of 1 000 bases, 100-base reads sampled from
the targets with 1 % substitutions, 20 % random, 10 % duplicates) with a repeat family planted so that (window, key)
blocks overflow at the configured MaxMatches: one 160-base motif copied into FAMILY_GENES genes at random places, and
FAMILY_READS reads sampled from the motif.  A read of the family is accepted in every gene of the family, so the block
of its window holds (reads with that key) x FAMILY_GENES pairs.

The CLI runs RUNS times with MUSC_MAXMATCHES=host and RUNS times with =device, interleaved.  Per run, from muscato.log:
the replay lap (`MaxMatches replay on the ...`), the `results.txt` lap and the `nonmatch + stats files` lap -- what the
choice moves: after a host replay the selection exists on the host only -- their sum, the counts of the replay (suspect
probes, truncated blocks, and on the device the pairs those blocks held), musc_maxmatches_last_ms and k_mm_replay's own
time, and the sha1 of the four output files.  The summary applies DESIGN.md 15's rule to the sums: the device wins when
the difference of the medians exceeds three times the larger spread.  One JSON object per line goes to
profiles/maxmatches.jsonl; the last line is the summary.
usage: maxmatches.py <workdir> [n_reads] [n_targets] [runs] [max_matches]"""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "maxmatches.jsonl")
OUTPUTS = ("results.txt", "results.nonmatch.txt.fastq", "results_genestats.txt", "results_readstats.txt")
FAMILY_GENES, FAMILY_READS, MOTIF = 2000, 400, 160


def generate(wd, n_reads, n_targets, max_matches):
    L, TL = 100, 1000
    os.makedirs(wd, exist_ok=True)
    rng = np.random.default_rng(1)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    T = lut[rng.integers(0, 4, size=(n_targets, TL), dtype=np.uint8)]
    fam = min(FAMILY_GENES, n_targets)
    motif = lut[rng.integers(0, 4, size=MOTIF, dtype=np.uint8)]
    for g in rng.choice(n_targets, size=fam, replace=False):
        p = int(rng.integers(0, TL - MOTIF + 1))
        T[g, p:p + MOTIF] = motif
    with open(os.path.join(wd, "genes.txt"), "wb") as f:
        for i in range(n_targets):
            f.write(b"gene%d\t" % i + T[i].tobytes() + b"\n")
    g = rng.integers(0, n_targets, size=n_reads)
    p = rng.integers(0, TL - L + 1, size=n_reads)
    R = T[g[:, None], p[:, None] + np.arange(L)[None, :]].copy()
    sub = rng.random(R.shape) < 0.01
    R[sub] = lut[rng.integers(0, 4, size=int(sub.sum()))]
    rnd = rng.random(n_reads) < 0.2
    R[rnd] = lut[rng.integers(0, 4, size=(int(rnd.sum()), L))]
    dup = rng.random(n_reads) < 0.1
    R[dup] = R[rng.integers(0, n_reads, size=int(dup.sum()))]
    nfam = min(FAMILY_READS, n_reads)
    for i in rng.choice(n_reads, size=nfam, replace=False):  # the family's reads: windows at a few offsets of the motif
        o = int(rng.integers(0, 8)) * 8
        R[i] = motif[o:o + L]
        s = rng.random(L) < 0.01
        s[:35] = False  # both windows stay exact
        R[i, s] = lut[rng.integers(0, 4, size=int(s.sum()))]
    qual = b"F" * L
    with open(os.path.join(wd, "reads.fastq"), "wb") as f:
        for i in range(n_reads):
            f.write(b"@read%d\n" % i + R[i].tobytes() + b"\n+\n" + qual + b"\n")
    subprocess.check_call([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], cwd=wd)
    cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
           "ResultsFileName": "results.txt", "Windows": [0, 20], "WindowWidth": 15, "PMatch": 0.97, "MinDinuc": 5,
           "MaxReadLength": 100, "MaxMatches": max_matches, "MMTol": 0, "MatchMode": "best"}
    with open(os.path.join(wd, "config.json"), "w") as f:
        json.dump(cfg, f)
    os.makedirs(os.path.join(wd, "muscato_logs"), exist_ok=True)
    return {"reads": n_reads, "targets": n_targets, "family_genes": fam, "family_reads": nfam, "motif_bases": MOTIF,
            "max_matches": max_matches}


def cli_run(wd, where):
    env = {k: v for k, v in os.environ.items() if k not in ("MUSC_RESULTS", "MUSC_SIDE")}
    env["MUSC_MAXMATCHES"] = where
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], cwd=wd, env=env, stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    lap = lambda name: float(re.search(r"stage " + name + r"\s+([0-9.]+) s", log).group(1))
    m = re.search(r"MaxMatches replay on the (\w+): ([0-9.]+) s", log)
    if not m or m.group(1) != where:
        raise SystemExit("the replay did not run on the %s:\n%s" % (where, log))
    c = re.search(r"MaxMatches: (\d+) suspect probes, (\d+) blocks truncated", log)
    rec = {"where": where, "replay_s": float(m.group(2)), "results_s": lap(r"results\.txt"), "side_s": lap(r"nonmatch \+ stats files"),
           "hot_path_s": lap("hot path[^0-9]*?"), "suspect_probes": int(c.group(1)), "truncated_blocks": int(c.group(2)),
           "results_from": "device" if "results on the device" in log else "host",
           "side_from": "device" if "side outputs on the device" in log else "host"}
    rec["sum_s"] = round(rec["replay_s"] + rec["results_s"] + rec["side_s"], 3)
    d = re.search(r"\(device ([0-9.]+) ms, k_mm_replay ([0-9.]+) ms, (\d+) pairs", log)
    if d:
        rec.update(maxmatches_ms=float(d.group(1)), k_mm_replay_ms=float(d.group(2)), pairs_in_truncated_blocks=int(d.group(3)),
                   k_mm_replay_share=round(float(d.group(2)) / max(float(d.group(1)), 1e-9), 4))
    h = hashlib.sha1()
    for o in OUTPUTS:
        with open(os.path.join(wd, o), "rb") as f:
            h.update(f.read())
    rec["sha1_outputs"] = h.hexdigest()
    rec["results_bytes"] = os.path.getsize(os.path.join(wd, "results.txt"))
    return rec


def main():
    wd = sys.argv[1]
    n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
    n_targets = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    max_matches = int(sys.argv[5]) if len(sys.argv) > 5 else 1000
    recs = []
    with open(OUT, "w") as out:
        def emit(rec):
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec), flush=True)
        emit(dict(generate(wd, n_reads, n_targets, max_matches), workload=True))
        for i in range(runs):
            for where in ("host", "device"):
                rec = dict(cli_run(wd, where), run=i)
                recs.append(rec)
                emit(rec)
        sums = {w: [r["sum_s"] for r in recs if r["where"] == w] for w in ("host", "device")}
        spread = max(max(v) - min(v) for v in sums.values())
        diff = statistics.median(sums["host"]) - statistics.median(sums["device"])
        dev = [r for r in recs if r["where"] == "device"]
        emit({"summary": True, "runs": runs, "identical_outputs": len({r["sha1_outputs"] for r in recs}) == 1,
              "host_sum_s": sums["host"], "device_sum_s": sums["device"],
              "host_sum_median_s": statistics.median(sums["host"]), "device_sum_median_s": statistics.median(sums["device"]),
              "larger_spread_s": round(spread, 3), "median_difference_s": round(diff, 3), "device_wins": diff > 3 * spread,
              "truncated_blocks": dev[0]["truncated_blocks"], "pairs_in_truncated_blocks": dev[0].get("pairs_in_truncated_blocks"),
              "maxmatches_ms_median": statistics.median(r["maxmatches_ms"] for r in dev),
              "k_mm_replay_ms_median": statistics.median(r["k_mm_replay_ms"] for r in dev)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
