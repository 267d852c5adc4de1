#!/usr/bin/env python3
"""The coverage files made by the host against the same made by the device, on profiles/e2e.py's workload.

The workload is generated once (e2e.py: 2 M reads x 100 k targets unless sizes are given); then the CLI runs RUNS times
with MUSC_COVERAGE=host and RUNS times with MUSC_COVERAGE=device, interleaved (host, device, host, ...) so that drift of
the machine hits both alike.  Per run: the `coverage files on the host|device` lap of muscato.log, the bytes and the sha1
of both files, and for the device runs the HIP-event times of musc_cov_prepare (events, the KeyPasses sort, the scans and
compactions: the sort's rate is stated as events per second of the whole prepare, its upper bound in time) and of the
musc_cov_text calls (bytes per second of k_cov_render and k_cov_sum_render together) beside k_results_render's on the
same list.  One JSON object per line goes to profiles/coverage.jsonl; the last line is the summary with the decision
rule of DESIGN.md 15: the device becomes the default (MUSC_COVERAGE_DEFAULT_DEVICE) when the difference of the medians
exceeds three times the larger spread (max - min) of the two sides.
usage: coverage.py <workdir> [n_reads] [n_targets] [runs]"""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "coverage.jsonl")
COV = "results.bedgraph"


def sha1(path):
    with open(path, "rb") as fh:
        data = fh.read()
    return len(data), hashlib.sha1(data).hexdigest()


def cli_run(wd, where):
    env = dict(os.environ, MUSC_COVERAGE=where)
    env.pop("MUSC_RESULTS", None)  # (results.txt from the device, the default with one GPU: the device side needs its list)
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json", "-CoverageFileName=" + COV, "-CoverageWeighted"],
                       cwd=wd, env=env, stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    lap = re.search(r"coverage files on the (host|device): ([0-9.]+) s", log)
    if lap is None or lap.group(1) != where:
        raise SystemExit("MUSC_COVERAGE=%s, but the log says otherwise:\n%s" % (where, log))
    rec = {"where": where, "lap_s": float(lap.group(2))}
    res = re.search(r"results on the device: (\d+) bytes, order ([0-9.]+) ms, text ([0-9.]+) ms", log)
    if res:
        rec.update(results_bytes=int(res.group(1)), results_ms_text=float(res.group(3)),
                   results_render_bytes_per_s=int(res.group(1)) / (float(res.group(3)) * 1e-3))
    m = re.search(r"coverage on the device: (\d+) \+ (\d+) bytes, (\d+) events, prepare ([0-9.]+) ms, text ([0-9.]+) ms", log)
    if m:
        nbytes, events, ms_prepare, ms_text = int(m.group(1)) + int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5))
        rec.update(events=events, ms_prepare=ms_prepare, ms_text=ms_text, sort_events_per_s=events / (ms_prepare * 1e-3),
                   cov_render_bytes_per_s=nbytes / (ms_text * 1e-3))
    (rec["bytes"], rec["sha1"]), (rec["targets_bytes"], rec["targets_sha1"]) = sha1(os.path.join(wd, COV)), sha1(os.path.join(wd, COV + "_targets"))
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
        summary = {"summary": True, "runs": runs, "identical_bytes": len({(r["sha1"], r["targets_sha1"]) for r in recs}) == 1,
                   "host_lap_s": laps["host"], "device_lap_s": laps["device"],
                   "host_lap_median_s": statistics.median(laps["host"]), "device_lap_median_s": statistics.median(laps["device"]),
                   "spread_s": spread, "median_difference_s": diff, "device_becomes_default": diff > 3 * spread,
                   "ms_prepare_median": statistics.median(r["ms_prepare"] for r in dev),
                   "ms_text_median": statistics.median(r["ms_text"] for r in dev),
                   "sort_events_per_s_median": statistics.median(r["sort_events_per_s"] for r in dev),
                   "cov_render_bytes_per_s_median": statistics.median(r["cov_render_bytes_per_s"] for r in dev),
                   "results_render_bytes_per_s_median": statistics.median(r["results_render_bytes_per_s"] for r in dev)}
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
