#!/usr/bin/env python3
"""Read prep with the FASTQ parse on the host against the parse on the device, on profiles/e2e.py's
workload (2 M reads x 100 k targets unless sizes are given).

The workload is generated once; then the CLI runs RUNS times with MUSC_PREP=host and RUNS times with MUSC_PREP=device,
interleaved (host, device, host, ...) so that drift of the machine hits both alike.  Per run: the `read prep` lap of
muscato.log (the stage this work moves), the device stage's HIP-event time from the log's `read prep on the device`
line, and a hash of results.txt.  The summary has the median and the spread (max - min) of both laps and whether the
difference of the medians exceeds three times the larger spread (DESIGN.md 15's criterion).  One JSON object per line
goes to profiles/fastq_prep.jsonl; the last line is the summary.
The newline pass alone, from a kernel trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/fastq_prep.py --kernel-only FASTQ
(k_fq_count / k_fq_lines in DIR/*/*kernel_stats.csv; `--rate CSV BYTES` turns their average times into input bytes per
second, to be read next to the 6.29 TB/s copy ceiling of DESIGN.md 5).
usage: fastq_prep.py <workdir> [n_reads] [n_targets] [runs]  |  --kernel-only <fastq> [reps]  |  --rate <csv> <bytes>"""
import csv
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "fastq_prep.jsonl")
COPY_CEILING_TBPS = 6.29
sys.path.insert(0, ROOT)


def cli_run(wd, where):
    env = dict(os.environ, MUSC_PREP=where)
    os.makedirs(os.path.join(wd, "muscato_logs"), exist_ok=True)
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], cwd=wd, env=env, stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    rec = {"where": where, "lap_s": float(re.search(r"stage read prep\s+([0-9.]+) s", log).group(1)),
           "total_s": float(re.findall(r"\(total ([0-9.]+) s\)", log)[-1])}
    m = re.search(r"read prep on the device: (\d+) records, (\d+) kept, (\d+) distinct, ([0-9.]+) ms", log)
    assert bool(m) == (where == "device"), log
    if m:
        rec.update(records=int(m.group(1)), kept=int(m.group(2)), distinct=int(m.group(3)), device_ms=float(m.group(4)))
    h = hashlib.sha1()
    with open(os.path.join(wd, "results.txt"), "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    rec["sha1"] = h.hexdigest()
    return rec


def kernel_only(path, reps):
    """The device stage on a text that is already in device memory, reps times (the first call warms up)."""
    import torch
    import numpy as np
    from muscato_amd import Engine
    raw = np.fromfile(path, dtype=np.uint8)
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    ms = []
    with Engine(0) as eng:
        for _ in range(reps + 1):
            out = eng.prep_fastq_device(d.data_ptr(), len(raw), 0, 100)
            ms.append(eng.stats()["ms_read_prep"])
    return {"kernel_only": True, "fastq_bytes": int(len(raw)), "records": out["n_records"], "distinct": out["n_unique"],
            "device_stage_ms": ms[1:], "device_stage_ms_median": statistics.median(ms[1:])}


def rate(csv_path, nbytes):
    out = {"newline_pass": True, "fastq_bytes": nbytes, "copy_ceiling_TBps": COPY_CEILING_TBPS}
    with open(csv_path) as f:
        for row in csv.DictReader(f):
            for k in ("k_fq_count", "k_fq_lines", "k_fq_records", "k_fq_gather"):
                if k in row["Name"]:
                    avg_ns = float(row["AverageNs"])
                    out[k] = {"calls": int(row["Calls"]), "avg_us": avg_ns / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                              "input_TBps": nbytes / avg_ns / 1e3}
    return out


def main():
    if sys.argv[1] == "--kernel-only":
        print(json.dumps(kernel_only(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)))
        return 0
    if sys.argv[1] == "--rate":
        rec = rate(sys.argv[2], int(sys.argv[3]))
        with open(OUT, "a") as out:
            out.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))
        return 0
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
        spread = {w: max(v) - min(v) for w, v in laps.items()}
        med = {w: statistics.median(v) for w, v in laps.items()}
        dev_ms = [r["device_ms"] for r in recs if r["where"] == "device"]
        summary = {"summary": True, "runs": runs, "fastq_bytes": os.path.getsize(os.path.join(wd, "reads.fastq")),
                   "identical_bytes": len({r["sha1"] for r in recs}) == 1,
                   "host_lap_s": laps["host"], "device_lap_s": laps["device"],
                   "host_lap_median_s": med["host"], "device_lap_median_s": med["device"],
                   "host_spread_s": spread["host"], "device_spread_s": spread["device"],
                   "device_stage_ms": dev_ms, "device_stage_ms_median": statistics.median(dev_ms),
                   "difference_s": med["host"] - med["device"],
                   "exceeds_three_spreads": abs(med["host"] - med["device"]) > 3 * max(spread.values())}
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
