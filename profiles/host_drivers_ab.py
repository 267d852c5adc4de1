#!/usr/bin/env python3
"""The stage times the library reports and bench.py's value, parent build against this build.

`--parent PATH` names the parent commit's libmuscato_hip.so (MUSC_LIB_PATH); the tree's own library is `this`.  Each
measurement runs in a process of its own, RUNS times per build, interleaved (parent, this, parent, ...) so that drift
of the machine hits both alike:
  stages  on profiles/e2e.py's workload (2 M reads x 100 k targets, the input of profiles/read_names.py), generated once:
          musc_reads_prep_fastq_names (ms_read_prep, names.ms_names), a pass, musc_maxmatches_apply (maxmatches_ms),
          musc_results_order (results_ms) and musc_side_prepare (side_ms), with a hash of what they returned
  bench   bench.py --gpus 1 on its default workload (value, reads/s)
One JSON object per run goes to --out; the last line is the summary: per metric the median and the spread (max - min)
of both builds, and whether this build's median lies within the parent's spread of the parent's median.
usage: host_drivers_ab.py --parent PATH [--runs N] [--out FILE] [--bench-args "..."]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("ms_read_prep", "ms_names", "maxmatches_ms", "results_ms", "side_ms")


def make_workload(wd, n_reads=2_000_000, n_targets=100_000, L=100, TL=1000):
    """profiles/e2e.py's reads and targets (same generator, same seed), as arrays and one FASTQ text."""
    rng = np.random.default_rng(1)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    T = lut[rng.integers(0, 4, size=(n_targets, TL), dtype=np.uint8)]
    g = rng.integers(0, n_targets, size=n_reads)
    p = rng.integers(0, TL - L + 1, size=n_reads)
    R = T[g[:, None], p[:, None] + np.arange(L)[None, :]].copy()
    sub = rng.random(R.shape) < 0.01
    R[sub] = lut[rng.integers(0, 4, size=int(sub.sum()))]
    rnd = rng.random(n_reads) < 0.2
    R[rnd] = lut[rng.integers(0, 4, size=(int(rnd.sum()), L))]
    dup = rng.random(n_reads) < 0.1
    R[dup] = R[rng.integers(0, n_reads, size=int(dup.sum()))]
    qual = b"\n+\n" + b"F" * L + b"\n"
    with open(os.path.join(wd, "reads.fastq"), "wb") as f:
        f.write(b"".join(b"@read%d\n" % i + R[i].tobytes() + qual for i in range(n_reads)))
    np.save(os.path.join(wd, "targets.npy"), T)


def stages_child(wd):
    sys.path.insert(0, ROOT)
    from muscato_amd import Config, Engine
    T = np.load(os.path.join(wd, "targets.npy"))
    raw = open(os.path.join(wd, "reads.fastq"), "rb").read()
    cfg = Config(Windows=[0, 20], WindowWidth=15, PMatch=0.97, MinDinuc=5, MaxReadLength=100, MaxMatches=1000000, MMTol=0,
                 MatchMode="best").with_defaults()
    h = hashlib.sha1()
    with Engine(0) as e:
        e.load_targets_arrays(np.ascontiguousarray(T.reshape(-1)), np.arange(T.shape[0] + 1, dtype=np.uint64) * T.shape[1])
        e.set_gene_text([b"gene%d\t%d" % (i, T.shape[1]) for i in range(T.shape[0])])
        fp = e.prep_fastq_names(raw, cfg.MinReadLength, cfg.MaxReadLength)
        rec = {"ms_read_prep": e.stats()["ms_read_prep"], "ms_names": float(fp["names"]["ms_names"]), "n_unique": fp["n_unique"]}
        for k in ("order", "ustart", "ranked"):
            h.update(fp[k].tobytes())
        rec["nhits"] = e.match_device(cfg, apply_mmtol=False)
        rec["kept"] = e.apply_maxmatches()["nhits"]
        rec["maxmatches_ms"] = e.maxmatches_ms()
        rec["lines"], rec["bytes"] = e.results_order(None)
        rec["results_ms"] = e.results_ms()[0]
        h.update(e.results_hits().tobytes())
        side = e.side_prepare()
        rec["side_ms"] = e.side_ms()[0]
        h.update(json.dumps(side, sort_keys=True).encode())
        h.update(e.genestats_text())
    rec["sha1"] = h.hexdigest()
    print(json.dumps(rec), flush=True)


def run_child(argv, lib):
    env = dict(os.environ)
    env.pop("MUSC_LIB_PATH", None)
    if lib:
        env["MUSC_LIB_PATH"] = os.path.abspath(lib)
    r = subprocess.run(argv, env=env, cwd=ROOT, stdout=subprocess.PIPE, timeout=900)
    if r.returncode:
        raise SystemExit("%s failed (%d)" % (" ".join(argv), r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_drivers_ab.jsonl"))
    ap.add_argument("--bench-args", default="--steps 20 --warmup 5")
    ap.add_argument("--stages-child", default=None)
    a = ap.parse_args()
    if a.stages_child:
        return stages_child(a.stages_child)
    if not a.parent or not os.path.exists(a.parent):
        raise SystemExit("--parent: the parent commit's libmuscato_hip.so")
    builds = (("parent", a.parent), ("this", None))
    recs = []
    with open(a.out, "w") as out, tempfile.TemporaryDirectory() as wd:
        def note(rec):
            recs.append(rec)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec), flush=True)
        make_workload(wd)
        for i in range(a.runs):
            for label, lib in builds:
                note(dict(run_child([sys.executable, os.path.abspath(__file__), "--stages-child", wd], lib), build=label, run=i, what="stages"))
        for i in range(a.runs):
            for label, lib in builds:
                b = run_child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + a.bench_args.split(), lib)
                note({"build": label, "run": i, "what": "bench", "value": b["value"], "ms_per_step": b["ms_per_step"]})
        summary = {"summary": True, "runs": a.runs, "identical_outputs": len({r["sha1"] for r in recs if r["what"] == "stages"}) == 1}
        for what, metrics, higher in (("stages", STAGES, False), ("bench", ("value",), True)):
            for m in metrics:
                v = {label: [r[m] for r in recs if r["what"] == what and r["build"] == label] for label, _ in builds}
                med = {k: statistics.median(x) for k, x in v.items()}
                spread = {k: max(x) - min(x) for k, x in v.items()}
                loss = (med["parent"] - med["this"]) if higher else (med["this"] - med["parent"])
                summary[m] = {"parent_median": med["parent"], "this_median": med["this"], "parent_spread": spread["parent"],
                              "this_spread": spread["this"], "within_parent_spread": abs(med["this"] - med["parent"]) <= spread["parent"], "loss": loss}
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
