#!/usr/bin/env python3
"""Read prep with the names of the reads made on the host against the names made on the device, the FASTQ
parse on the device either way, on profiles/e2e.py's workload (2 M reads x 100 k targets unless sizes are
given).

The workload is generated once; then the CLI runs RUNS times with MUSC_PREP=device MUSC_PREP_NAMES=host and RUNS times
with MUSC_PREP_NAMES=device, interleaved (host, device, host, ...) so that drift of the machine hits both alike.  Per
run: the `read prep` lap of muscato.log (the stage this work moves), the device times from the log's `read prep on the
device` and `read names on the device` lines (ms_names), and a hash of results.txt.  The summary has the median and the
spread (max - min) of both laps and whether the difference of the medians exceeds three times the larger spread
(DESIGN.md 15's criterion).  One JSON object per line goes to profiles/read_names.jsonl; the last line is the summary.
usage: read_names.py <workdir> [n_reads] [n_targets] [runs]"""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "read_names.jsonl")


def cli_run(wd, names):
    env = dict(os.environ, MUSC_PREP="device", MUSC_PREP_NAMES=names)
    os.makedirs(os.path.join(wd, "muscato_logs"), exist_ok=True)
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], cwd=wd, env=env, stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    rec = {"names": names, "lap_s": float(re.search(r"stage read prep\s+([0-9.]+) s", log).group(1)),
           "total_s": float(re.findall(r"\(total ([0-9.]+) s\)", log)[-1])}
    m = re.search(r"read prep on the device: (\d+) records, (\d+) kept, (\d+) distinct, ([0-9.]+) ms", log)
    rec.update(records=int(m.group(1)), kept=int(m.group(2)), distinct=int(m.group(3)), device_ms=float(m.group(4)))
    m = re.search(r"read names on the device: (\d+) groups of one, (\d+) counted, (\d+) sorted \((\d+) pairs, (\d+) key passes\), "
                  r"(\d+) bytes of lines, ([0-9.]+) ms", log)
    assert bool(m) == (names == "device"), log
    if m:
        rec.update(n_single=int(m.group(1)), n_counted=int(m.group(2)), n_sorted=int(m.group(3)), n_pairs=int(m.group(4)),
                   key_passes=int(m.group(5)), line_bytes=int(m.group(6)), ms_names=float(m.group(7)))
    h = hashlib.sha1()
    with open(os.path.join(wd, "results.txt"), "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    rec["sha1"] = h.hexdigest()
    return rec


def main():
    wd = sys.argv[1]
    sizes = sys.argv[2:4]
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    subprocess.check_call([sys.executable, os.path.join(ROOT, "profiles", "e2e.py"), wd] + sizes, stderr=subprocess.DEVNULL)
    recs = []
    with open(OUT, "w") as out:
        for i in range(runs):
            for names in ("host", "device"):
                rec = dict(cli_run(wd, names), run=i)
                recs.append(rec)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
        laps = {w: [r["lap_s"] for r in recs if r["names"] == w] for w in ("host", "device")}
        spread = {w: max(v) - min(v) for w, v in laps.items()}
        med = {w: statistics.median(v) for w, v in laps.items()}
        ms_names = [r["ms_names"] for r in recs if r["names"] == "device"]
        summary = {"summary": True, "runs": runs, "fastq_bytes": os.path.getsize(os.path.join(wd, "reads.fastq")),
                   "identical_bytes": len({r["sha1"] for r in recs}) == 1,
                   "host_lap_s": laps["host"], "device_lap_s": laps["device"],
                   "host_lap_median_s": med["host"], "device_lap_median_s": med["device"],
                   "host_spread_s": spread["host"], "device_spread_s": spread["device"],
                   "ms_names": ms_names, "ms_names_median": statistics.median(ms_names),
                   "difference_s": med["host"] - med["device"],
                   "exceeds_three_spreads": abs(med["host"] - med["device"]) > 3 * max(spread.values())}
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
