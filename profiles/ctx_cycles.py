#!/usr/bin/env python3
"""Free device memory over create .. destroy cycles of a context (every buffer goes with its owner).

Twenty cycles in one process of: musc_init, load targets and reads, set both texts, a pass, musc_results_order of its
list, musc_side_prepare and the three side texts, musc_maxmatches_apply, musc_destroy.  After each cycle the free
device memory (hipMemGetInfo of the runtime the library links) is written down, together with a checksum of what the
cycle returned.  The loop runs once per library, each in a process of its own: `--lib label=path` names another build
of libmuscato_hip.so (MUSC_LIB_PATH: the parent commit's, say), and the tree's own library always runs last as `this`.
One JSON object per cycle goes to profiles/ctx_cycles.jsonl (or --out); the last line per library is its summary:
the free bytes after the first and after the last cycle, and their difference -- a context that leaks a block per
cycle shows as a series that falls, step by step.  Device-wide free memory also moves with whatever else runs on the
GPU, which is why this is a script and not a test.
usage: ctx_cycles.py [--lib label=path]... [--cycles N] [--out file]"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ctx_cycles.jsonl")


def make_case():
    rng = random.Random(19)
    targets = [bytes(rng.choice(b"ACGT") for _ in range(300)) for _ in range(2000)]
    reads = set()
    for t in targets:
        for p in (0, 57, 240):
            r = bytearray(t[p:p + 60])
            if rng.random() < 0.5:
                q = rng.randrange(60)
                r[q] = rng.choice(bytes(set(b"ACGT") - {r[q]}))
            reads.add(bytes(r))
    return sorted(reads), targets


def free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    rc = hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    if rc != 0:
        raise RuntimeError("hipMemGetInfo failed (%d)" % rc)
    return int(free.value)


def child(label, cycles, out):
    sys.path.insert(0, ROOT)
    from muscato_amd import Config, Engine, sorted_hits
    reads, targets = make_case()
    cfg = Config(Windows=[0, 10], WindowWidth=12, PMatch=0.95, MinDinuc=2, MaxReadLength=60, MMTol=1)
    rests = [b"g%d\t%d" % (g, len(t)) for g, t in enumerate(targets)]
    tails = [b"%d\tr%d" % (1 + i % 3, i) for i in range(len(reads))]
    series, sums = [], set()
    with open(out, "a") as f:
        for cycle in range(cycles):
            h = hashlib.sha1()
            with Engine(0) as e:
                e.load_targets(targets)
                e.load_reads(reads)
                e.set_gene_text(rests)
                e.set_read_text(tails)
                n = e.match_device(cfg, apply_mmtol=False)
                e.results_order(None)
                h.update(e.results_text())
                e.side_prepare()
                for text in (e.nonmatch_text, e.genestats_text, e.readstats_text):
                    h.update(text())
                kept = e.apply_maxmatches()["nhits"]
                h.update(sorted_hits(e.hits()).tobytes())
            series.append(free_bytes())
            sums.add(h.hexdigest())
            f.write(json.dumps({"lib": label, "cycle": cycle, "free_bytes": series[-1], "nhits": n, "kept": kept,
                                "sha1": h.hexdigest()}) + "\n")
        f.write(json.dumps({"lib": label, "summary": True, "cycles": cycles, "free_after_first": series[0],
                            "free_after_last": series[-1], "drift_bytes": series[-1] - series[0],
                            "min_free": min(series), "max_free": max(series), "distinct_outputs": len(sums)}) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="label=path of another libmuscato_hip.so")
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.cycles, a.out)
    open(a.out, "w").close()
    for spec in a.lib + ["this="]:
        label, path = spec.split("=", 1)
        env = dict(os.environ)
        env.pop("MUSC_LIB_PATH", None)
        if path:
            env["MUSC_LIB_PATH"] = os.path.abspath(path)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", label, "--cycles", str(a.cycles), "--out", a.out],
                       env=env, check=True, timeout=600)
    with open(a.out) as f:
        for line in f:
            if '"summary"' in line:
                print(line.strip())


if __name__ == "__main__":
    main()
