#!/usr/bin/env python3
"""results.txt on the host against results.txt on the device, on profiles/e2e.py's workload.

The workload is generated once (e2e.py: 2 M reads x 100 k targets unless sizes are given); then the CLI runs RUNS times
with MUSC_RESULTS=host and RUNS times with MUSC_RESULTS=device, interleaved (host, device, host, ...) so that drift
of the machine hits both alike.  Per run: the `results.txt` lap of muscato.log (the stage this work moves), the HIP-event
times of the order and of the text calls, the output bytes, and whether the bytes equal the first run's.  Last, one
musc_results_text call that renders every line of a resident synthetic list into a device buffer (no copy to the
host): the HIP-event time of the CALL (`text_call_ms`: two 8-byte copies to the host and a stream synchronisation come
before the launch, so it is an upper bound of the kernel's time and `text_call_out_GBps` a lower bound of its rate).
One JSON object per line goes to profiles/results_render.jsonl; the last line is the summary.
The kernel's own time comes from a kernel trace of that last part alone:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/results_render.py --kernel-only
(k_results_render in DIR/*/*kernel_stats.csv, kept as profiles/results_render_kernel_stats.csv), to be read next to
the 4.7 TB/s of the k_compact_w copy.
usage: results_render.py <workdir> [n_reads] [n_targets] [runs]  |  results_render.py --kernel-only"""
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
OUT = os.path.join(ROOT, "profiles", "results_render.jsonl")
sys.path.insert(0, ROOT)


def cli_run(wd, where):
    env = dict(os.environ, MUSC_RESULTS=where)
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], cwd=wd, env=env, stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    rec = {"where": where, "lap_s": float(re.search(r"stage results\.txt\s+([0-9.]+) s", log).group(1)),
           "hot_path_s": float(re.search(r"stage hot path[^0-9]+([0-9.]+) s", log).group(1))}
    m = re.search(r"results on the device: (\d+) bytes, order ([0-9.]+) ms, text ([0-9.]+) ms", log)
    if m:
        rec.update(ms_order=float(m.group(2)), ms_text=float(m.group(3)))
    with open(os.path.join(wd, "results.txt"), "rb") as f:
        data = f.read()
    rec.update(bytes=len(data), lines=data.count(b"\n"), sha1=hashlib.sha1(data).hexdigest())
    return rec


def kernel_rate(n_reads=400_000, n_targets=20_000, reps=5):
    """Text calls that render into a device buffer: one line per read, 100-base reads on 1 000-base targets."""
    import torch
    from muscato_amd import Engine
    rng = np.random.default_rng(3)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    T = lut[rng.integers(0, 4, size=(n_targets, 1000), dtype=np.uint8)]
    g = rng.integers(0, n_targets, size=n_reads)
    p = rng.integers(0, 901, size=n_reads)
    R = T[g[:, None], p[:, None] + np.arange(100)[None, :]]
    R, first = np.unique(R, axis=0, return_index=True)  # distinct, in bytewise order
    hits = np.stack([np.arange(len(R)), g[first], p[first], np.zeros(len(R), dtype=np.int64)], axis=1).astype(np.uint32)
    with Engine(0) as eng:
        eng.load_targets_arrays(np.concatenate([T.reshape(-1), np.zeros(8, np.uint8)]), np.arange(n_targets + 1, dtype=np.uint64) * 1000)
        eng.load_reads_arrays(np.concatenate([R.reshape(-1), np.zeros(8, np.uint8)]), np.arange(len(R) + 1, dtype=np.uint64) * 100)
        eng.set_gene_text([b"gene%d\t1000" % i for i in range(n_targets)])
        eng.set_read_text([b"1\tread%d" % i for i in range(len(R))])
        nl, nb = eng.results_order(hits)
        buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
        import ctypes
        ms = []
        for _ in range(reps + 1):  # the first one warms up
            before = eng.results_ms()[1]
            got = ctypes.c_uint64()
            eng._check(eng._lib.musc_results_text(eng._h, 0, nl, buf.data_ptr(), nb, 1, ctypes.byref(got)), "musc_results_text")
            ms.append(eng.results_ms()[1] - before)
        assert bytes(buf[:200].cpu().numpy()) == eng.results_text(0, 1)[:200]
        order_ms = eng.results_ms()[0]
    ms = ms[1:]
    return {"text_call_lines": nl, "text_call_bytes": nb, "text_call_ms": ms, "text_call_ms_median": statistics.median(ms),
            "text_call_out_GBps": nb / 1e6 / statistics.median(ms), "order_ms": order_ms}


def main():
    if sys.argv[1] == "--kernel-only":
        print(json.dumps(kernel_rate()))
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
        spread = max(max(v) - min(v) for v in laps.values())
        summary = {"summary": True, "runs": runs, "identical_bytes": len({r["sha1"] for r in recs}) == 1,
                   "host_lap_s": laps["host"], "device_lap_s": laps["device"],
                   "host_lap_median_s": statistics.median(laps["host"]), "device_lap_median_s": statistics.median(laps["device"]),
                   "spread_s": spread,
                   "device_wins": statistics.median(laps["host"]) - statistics.median(laps["device"]) > spread}
        summary.update(kernel_rate())
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
