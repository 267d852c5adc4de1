#!/usr/bin/env python3
"""The nonmatch FASTQ and the two stats files on the host against the same on the device, on
profiles/e2e.py's workload.

The workload is generated once (e2e.py: 2 M reads x 100 k targets unless sizes are given); then the CLI runs RUNS times
with MUSC_SIDE=host and RUNS times with MUSC_SIDE=device, interleaved (host, device, host, ...) so that drift of the
machine hits both alike.  Per run: the `nonmatch + stats files` lap of muscato.log (the stage this work moves), for the
device runs the HIP-event times of musc_side_prepare and of the musc_side_text calls (the log's `side outputs on the
device` line), the bytes of the three files and one sha1 over them.  The host side is the parent's code unchanged in the
same build: the comparison is never against an earlier figure of the device path.  One JSON object per line goes to
profiles/side_outputs.jsonl; the last line is the summary with the decision rule of DESIGN.md 15: the device becomes
the default when the difference of the medians exceeds three times the larger spread (max - min) of the two sides.
usage: side_outputs.py <workdir> [n_reads] [n_targets] [runs]"""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "side_outputs.jsonl")
FILES = ("results.nonmatch.txt.fastq", "results_genestats.txt", "results_readstats.txt")


def cli_run(wd, where):
    env = dict(os.environ, MUSC_SIDE=where)
    env.pop("MUSC_RESULTS", None)  # (results.txt from the device, the default with one GPU: the device side needs it)
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], cwd=wd, env=env, stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    rec = {"where": where, "lap_s": float(re.search(r"stage nonmatch \+ stats files\s+([0-9.]+) s", log).group(1)),
           "results_lap_s": float(re.search(r"stage results\.txt\s+([0-9.]+) s", log).group(1))}
    m = re.search(r"side outputs on the device: prepare ([0-9.]+) ms, text ([0-9.]+) ms", log)
    if (m is not None) != (where == "device"):
        raise SystemExit("MUSC_SIDE=%s, but the log says otherwise:\n%s" % (where, log))
    if m:
        rec.update(ms_prepare=float(m.group(1)), ms_text=float(m.group(2)))
    h = hashlib.sha1()
    sizes = []
    for f in FILES:
        with open(os.path.join(wd, f), "rb") as fh:
            data = fh.read()
        h.update(data)
        sizes.append(len(data))
    rec.update(bytes=sizes, sha1=h.hexdigest())
    return rec


def main():
    wd = sys.argv[1]
    sizes = sys.argv[2:4]
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    subprocess.check_call([sys.executable, os.path.join(ROOT, "profiles", "e2e.py"), wd] + sizes, stderr=subprocess.DEVNULL)
    recs = []
    with open(OUT, "w") as out:
        for i in range(runs):
            for where in ("host", "device"):
                rec = dict(cli_run(wd, where), run=i)
                recs.append(rec)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
        laps = {w: [r["lap_s"] for r in recs if r["where"] == w] for w in ("host", "device")}
        spread = max(max(v) - min(v) for v in laps.values())
        diff = statistics.median(laps["host"]) - statistics.median(laps["device"])
        dev = [r for r in recs if r["where"] == "device"]
        summary = {"summary": True, "runs": runs, "identical_bytes": len({r["sha1"] for r in recs}) == 1,
                   "host_lap_s": laps["host"], "device_lap_s": laps["device"],
                   "host_lap_median_s": statistics.median(laps["host"]), "device_lap_median_s": statistics.median(laps["device"]),
                   "spread_s": spread, "median_difference_s": diff, "device_becomes_default": diff > 3 * spread,
                   "ms_prepare_median": statistics.median(r["ms_prepare"] for r in dev),
                   "ms_text_median": statistics.median(r["ms_text"] for r in dev)}
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
