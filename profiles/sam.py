#!/usr/bin/env python3
"""The SAM file written by the host against the same written by the device, on profiles/e2e.py's workload.

The workload is generated once (e2e.py: 2 M reads x 100 k targets unless sizes are given); then the CLI runs RUNS times
with MUSC_SAM=host and RUNS times with MUSC_SAM=device, interleaved (host, device, host, ...) so that drift of the
machine hits both alike.  Per run: the `sam file on the host|device` lap of muscato.log, the bytes and the sha1 of the SAM
file, and for the device runs the HIP-event times of musc_sam_prepare and of the musc_sam_text calls beside those of
musc_results_text on the same list (the log's `sam on the device` and `results on the device` lines): bytes per second of
k_sam_render next to k_results_render's, the parent's kernel in the same run.  One JSON object per line goes to
profiles/sam.jsonl; the last line is the summary with the decision rule of DESIGN.md 15: the device becomes the default
(MUSC_SAM_DEFAULT_DEVICE) when the difference of the medians exceeds three times the larger spread (max - min) of the two
sides.
usage: sam.py <workdir> [n_reads] [n_targets] [runs]"""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "sam.jsonl")
SAM = "results.sam"


def cli_run(wd, where):
    env = dict(os.environ, MUSC_SAM=where)
    env.pop("MUSC_RESULTS", None)  # (results.txt from the device, the default with one GPU: the device side needs its list)
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json", "-SamFileName=" + SAM], cwd=wd, env=env,
                       stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    lap = re.search(r"sam file on the (host|device): ([0-9.]+) s", log)
    if lap is None or lap.group(1) != where:
        raise SystemExit("MUSC_SAM=%s, but the log says otherwise:\n%s" % (where, log))
    rec = {"where": where, "lap_s": float(lap.group(2))}
    res = re.search(r"results on the device: (\d+) bytes, order ([0-9.]+) ms, text ([0-9.]+) ms", log)
    if res:
        rec.update(results_bytes=int(res.group(1)), results_ms_text=float(res.group(3)),
                   results_render_bytes_per_s=int(res.group(1)) / (float(res.group(3)) * 1e-3))
    m = re.search(r"sam on the device: (\d+) bytes, prepare ([0-9.]+) ms, text ([0-9.]+) ms", log)
    if m:
        rec.update(ms_prepare=float(m.group(2)), ms_text=float(m.group(3)), sam_render_bytes_per_s=int(m.group(1)) / (float(m.group(3)) * 1e-3))
    h = hashlib.sha1()
    with open(os.path.join(wd, SAM), "rb") as fh:
        data = fh.read()
    h.update(data)
    rec.update(bytes=len(data), sha1=h.hexdigest())
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
                   "ms_text_median": statistics.median(r["ms_text"] for r in dev),
                   "sam_render_bytes_per_s_median": statistics.median(r["sam_render_bytes_per_s"] for r in dev),
                   "results_render_bytes_per_s_median": statistics.median(r["results_render_bytes_per_s"] for r in dev)}
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
