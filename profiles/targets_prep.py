#!/usr/bin/env python3
"""muscato_prep_targets through the host chain against the same through musc_targets_prep / musc_sz_frame.

A FASTA file of about <mbytes> MB is generated once (records of 500 to 5 000 bases in 60-base lines, one base in 200
an N).  Then the tool runs RUNS times with MUSC_PREP_TARGETS=host and RUNS times with =device, interleaved, each with
-rev: wall time per run, the device path's own log line, and one sha1 over both output files.  After that the library
alone: Engine.prep_targets on the same bytes (the info struct's HIP-event time), prepared_text downloads, Engine.sz_frame.
One JSON object per line goes to profiles/targets_prep.jsonl; the last line is the summary with the decision rule of
DESIGN.md 15 -- the device would become the default when the difference of the medians exceeds three times the larger
spread (max - min) of the two sides.  MUSC_PREP_TARGETS_DEFAULT_DEVICE stays 0 whatever this says.
usage: targets_prep.py <workdir> [mbytes] [runs]"""
import hashlib
import json
import os
import random
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "targets_prep.jsonl")


def make_fasta(path, mbytes):
    rng = random.Random(22)
    unit = bytes(rng.choice(b"ACGT") for _ in range(1 << 16))
    with open(path, "wb") as f:
        size, g = 0, 0
        while size < mbytes << 20:
            n = rng.randint(500, 5000)
            p = rng.randrange(len(unit) - n)
            seq = bytearray(unit[p:p + n])
            for _ in range(n // 200):
                seq[rng.randrange(n)] = ord("N")
            rec = b">gene%d some description\n" % g + b"".join(bytes(seq[i:i + 60]) + b"\n" for i in range(0, n, 60))
            f.write(rec)
            size += len(rec)
            g += 1


def tool_run(wd, where):
    env = dict(os.environ, MUSC_PREP_TARGETS=where)
    t0 = time.perf_counter()
    r = subprocess.run([os.path.join(BIN, "muscato_prep_targets"), "-rev", "genes.fasta"], cwd=wd, env=env, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    err = r.stderr.decode()
    if r.returncode:
        raise SystemExit(err)
    m = re.search(r"targets prep on the device: .* ([0-9.]+) ms", err)
    if (m is not None) != (where == "device"):
        raise SystemExit("MUSC_PREP_TARGETS=%s, but stderr says otherwise:\n%s" % (where, err))
    h = hashlib.sha1()
    for f in ("musc_genes.fasta.sz", "musc_ids_genes.fasta.sz"):
        with open(os.path.join(wd, f), "rb") as fh:
            h.update(fh.read())
    rec = {"where": where, "wall_s": round(wall, 3), "sha1": h.hexdigest()}
    if m:
        rec["ms_prep"] = float(m.group(1))
    return rec


def main(argv):
    wd = argv[0]
    mbytes = int(argv[1]) if len(argv) > 1 else 100
    runs = int(argv[2]) if len(argv) > 2 else 5
    os.makedirs(wd, exist_ok=True)
    fasta = os.path.join(wd, "genes.fasta")
    make_fasta(fasta, mbytes)
    recs = []
    with open(OUT, "w") as out:
        def emit(rec):
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec), flush=True)
        for i in range(runs):
            for where in ("host", "device"):
                recs.append(dict(tool_run(wd, where), run=i))
                emit(recs[-1])
        from muscato_amd import Engine
        with open(fasta, "rb") as f:
            raw = f.read()
        with Engine(0) as e:
            for i in range(runs):
                t0 = time.perf_counter()
                info = e.prep_targets(raw, True, True)
                t1 = time.perf_counter()
                seqs = e.prepared_text(0)
                t2 = time.perf_counter()
                framed = e.sz_frame(seqs)
                t3 = time.perf_counter()
                emit({"library": True, "run": i, "ms_prep_events": round(info.ms, 3), "prep_call_s": round(t1 - t0, 4),
                      "download_s": round(t2 - t1, 4), "sz_frame_call_s": round(t3 - t2, 4), "n_targets": info.n_targets,
                      "n_seq_bytes": info.n_seq_bytes, "n_id_bytes": info.n_id_bytes, "framed_bytes": len(framed)})
        wall = {w: [r["wall_s"] for r in recs if r["where"] == w] for w in ("host", "device")}
        spread = max(max(v) - min(v) for v in wall.values())
        diff = statistics.median(wall["host"]) - statistics.median(wall["device"])
        emit({"summary": True, "runs": runs, "input_bytes": len(raw), "identical_bytes": len({r["sha1"] for r in recs}) == 1,
              "host_wall_s": wall["host"], "device_wall_s": wall["device"], "host_median_s": statistics.median(wall["host"]),
              "device_median_s": statistics.median(wall["device"]), "spread_s": round(spread, 3), "median_difference_s": round(diff, 3),
              "device_would_become_default": diff > 3 * spread})


if __name__ == "__main__":
    main(sys.argv[1:])
