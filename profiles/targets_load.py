#!/usr/bin/env python3
"""The gene file through the host chain against the same through musc_db_load_text, on profiles/e2e.py's
workload: the gene file is the one muscato_prep_targets writes (uncompressed chunks of 65 536 bytes).

laps:   the workload is generated once; then the CLI runs RUNS times with MUSC_TARGETS=host and RUNS times with
        MUSC_TARGETS=device, interleaved.  Per run: the laps `windows check, target files` and `hot path (init, load,
        match)` of muscato.log and their sum -- the device path makes GPU 0's context in the first lap where the host
        path makes it in the second, so only the sum compares like with like -- the stage's own log line, and one sha1
        over the four outputs.  One JSON object per line goes to profiles/targets_load.jsonl; the last line is the
        summary with the decision rule of DESIGN.md 15: the device becomes the default when the difference of the
        medians exceeds three times the larger spread (max - min) of the two sides.
rates:  Engine.load_db_text on the workload's gene text, as uncompressed chunks and as a compressed stream tiled from
        N_DISTINCT distinct chunks made by the compressor of tests/sz_cases.py (a load needs no sensible index; the
        chunks are cached in <workdir>/comp_chunks.bin, or read from the file given).  Prints the HIP-event times of
        the info struct; run it under `rocprofv3 --kernel-trace --stats` for the kernel times.
usage: targets_load.py laps <workdir> [n_reads] [n_targets] [runs]
       targets_load.py rates <workdir> [chunk cache file]"""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "targets_load.jsonl")
FILES = ("results.txt", "results.nonmatch.txt.fastq", "results_genestats.txt", "results_readstats.txt")
N_DISTINCT = 200


def cli_run(wd, where):
    env = dict(os.environ, MUSC_TARGETS=where)
    before = set(os.listdir(os.path.join(wd, "muscato_logs")))
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], cwd=wd, env=env, stderr=subprocess.PIPE)
    if r.returncode:
        raise SystemExit(r.stderr.decode())
    new = sorted(set(os.listdir(os.path.join(wd, "muscato_logs"))) - before)
    log = open(os.path.join(wd, "muscato_logs", new[-1], "muscato.log")).read()
    lap = {k: float(re.search(r"stage %s\s+([0-9.]+) s" % re.escape(k), log).group(1))
           for k in ("windows check, target files", "hot path (init, load, match)")}
    rec = {"where": where, "targets_lap_s": lap["windows check, target files"], "hot_lap_s": lap["hot path (init, load, match)"],
           "sum_s": round(sum(lap.values()), 3)}
    m = re.search(r"targets on the device: .* decode ([0-9.]+) ms, parse ([0-9.]+) ms", log)
    if (m is not None) != (where == "device"):
        raise SystemExit("MUSC_TARGETS=%s, but the log says otherwise:\n%s" % (where, log))
    if m:
        rec.update(ms_decode=float(m.group(1)), ms_parse=float(m.group(2)))
    h = hashlib.sha1()
    for f in FILES:
        with open(os.path.join(wd, f), "rb") as fh:
            h.update(fh.read())
    rec["sha1"] = h.hexdigest()
    return rec


def laps(argv):
    wd = argv[0]
    sizes = argv[1:3]
    runs = int(argv[3]) if len(argv) > 3 else 5
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
        sums = {w: [r["sum_s"] for r in recs if r["where"] == w] for w in ("host", "device")}
        spread = max(max(v) - min(v) for v in sums.values())
        diff = statistics.median(sums["host"]) - statistics.median(sums["device"])
        dev = [r for r in recs if r["where"] == "device"]
        summary = {"summary": True, "runs": runs, "identical_bytes": len({r["sha1"] for r in recs}) == 1,
                   "gene_file_bytes": os.path.getsize(os.path.join(wd, "musc_genes.txt.sz")),
                   "host_sum_s": sums["host"], "device_sum_s": sums["device"],
                   "host_sum_median_s": statistics.median(sums["host"]), "device_sum_median_s": statistics.median(sums["device"]),
                   "spread_s": round(spread, 3), "median_difference_s": round(diff, 3), "device_becomes_default": diff > 3 * spread,
                   "ms_decode_median": statistics.median(r["ms_decode"] for r in dev),
                   "ms_parse_median": statistics.median(r["ms_parse"] for r in dev)}
        out.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)
    return 0


def compressed_chunks(text, cache):
    """N_DISTINCT chunks of the text through the test's compressor, as chunk bytes (header, CRC, block)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sz_cases as sc
    if os.path.exists(cache):
        blob = open(cache, "rb").read()
    else:
        blob = b"".join(sc.comp_chunk(sc.compress(text[k * 65536:(k + 1) * 65536]), plain=text[k * 65536:(k + 1) * 65536])
                        for k in range(N_DISTINCT))
        with open(cache, "wb") as f:
            f.write(blob)
    chunks, pos = [], 0
    while pos < len(blob):
        n = 4 + int.from_bytes(blob[pos + 1:pos + 4], "little")
        chunks.append(blob[pos:pos + n])
        pos += n
    return sc.STREAM_ID, chunks


def rates(argv):
    wd = argv[0]
    sys.path.insert(0, ROOT)
    from muscato_amd import Engine
    from oracle import muscato_oracle as orc
    plain_stream = open(os.path.join(wd, "musc_genes.txt.sz"), "rb").read()
    text = orc.snappy_framed_decode(plain_stream[:10 + N_DISTINCT * (65536 + 8)])
    ident, chunks = compressed_chunks(text, argv[1] if len(argv) > 1 else os.path.join(wd, "comp_chunks.bin"))
    n_chunks = (len(plain_stream) - 10) // (65536 + 8)
    comp_stream = ident + b"".join(chunks[k % len(chunks)] for k in range(n_chunks))
    with Engine(0) as e:
        for name, stream in (("uncompressed", plain_stream), ("compressed", comp_stream)):
            for rep in range(3):
                info = e.load_db_text(stream, framed=1)
                print(json.dumps({"stream": name, "rep": rep, "stream_bytes": len(stream), "text_bytes": info.n_text_bytes,
                                  "chunks": info.n_chunks, "targets": info.n_targets, "bases": info.n_bases,
                                  "ms_decode": round(info.ms_decode, 3), "ms_parse": round(info.ms_parse, 3),
                                  "decode_GBps_out": round(info.n_text_bytes / 1e6 / info.ms_decode, 2),
                                  "parse_GBps_text": round(info.n_text_bytes / 1e6 / info.ms_parse, 2)}), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] not in ("laps", "rates"):
        sys.exit(__doc__)
    sys.exit(laps(sys.argv[2:]) if sys.argv[1] == "laps" else rates(sys.argv[2:]))
