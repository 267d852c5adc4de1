#!/usr/bin/env python3
"""The compressing writer of framed snappy streams measured.  One JSON object per line is appended to
profiles/sz_compress.jsonl.

  sizes                  no GPU.  Per text corpus of tests/sz_compress_cases.py (one chunk each): the stored stream, the
                         compressed one, and the bytes of the elements beside those of the sequential model
                         (tests/sz_cases.py: compress).  Fixtures 06 and 07 of tests/golden/prep_targets hold real
                         Go-snappy streams: Go's stream length beside ours for the same plain text (informative: tiny).
  synth                  the gene text of `synth` cfg2 (100 000 targets of 1 000 bases, a line each), made and compressed
                         on the device: stored and compressed stream sizes, the sequential model on sampled chunks.
  kernels [mbytes]       runs `workload` under rocprofv3 --kernel-trace --stats in a run of its own (no counters): the
                         GB/s of input of k_sz_compress, k_sz_gather and k_sz_frame over a resident DNA text.
  workload [mbytes]      what `kernels` traces: a resident text of seeded DNA lines framed and compressed device to
                         device, three times each.
  tool <workdir> [mbytes] [runs]
                         muscato_prep_targets -rev in four configurations -- stored and compressed, on the host and on
                         the device -- `runs` times each, interleaved; wall time per run, the sizes of the files, the
                         bytes that cross PCIe on the device path (with musc_targets_prep_sz, and what the same run
                         moved when the texts came down and went up again), the criterion of DESIGN.md 15 (a difference
                         counts above three times the larger spread) and the host writer's single-thread rate from the
                         difference of the two host medians.  Both defaults stay 0 whatever this says."""
import csv
import glob
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
BIN = os.path.join(ROOT, "muscato_amd", "bin")
OUT = os.path.join(ROOT, "profiles", "sz_compress.jsonl")
CHUNK = 65536


def emit(rec):
    with open(OUT, "a") as out:
        out.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def sizes():
    import sz_cases as sc
    import sz_compress_cases as zc
    for name, _ in zc.CORPORA:
        data = zc.corpus(name)
        p = zc.parses(data)[0]
        emit({"mode": "sizes", "corpus": name, "plain_bytes": len(data), "stored_stream": len(sc.frame(data, False)),
              "compressed_stream": len(zc.model(data)), "element_bytes": p.element_bytes,
              "sequential_model_element_bytes": sum(len(e[1]) for e in sc.compress(data)), "copies": len(p.copies),
              "near_copies": sum(1 for q, _, _ in p.copies if q in p.near)})
    for case in ("06", "07"):
        d = os.path.join(ROOT, "tests", "golden", "prep_targets", case)
        go = open(os.path.join(d, "genes.txt.sz"), "rb").read()
        plain = sc.ref_decode(go)
        emit({"mode": "sizes", "fixture": case, "plain_bytes": len(plain), "go_snappy_stream": len(go), "our_compressed_stream": len(zc.model(plain)),
              "stored_stream": len(sc.frame(plain, False))})


def dna_text(torch, mbytes, width=1000):
    g = torch.Generator(device="cuda")
    g.manual_seed(27)
    n = (mbytes << 20) // (width + 1)
    t = torch.randint(0, 4, (n, width + 1), dtype=torch.uint8, device="cuda", generator=g)
    t = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[t.long()]
    t[:, width] = 10
    return t.reshape(-1).contiguous()


def raw_call(e, fn, text, out):
    import ctypes
    nout = ctypes.c_uint64()
    rc = fn(e._h, text.data_ptr(), text.numel(), 1, out.data_ptr(), out.numel(), 1, ctypes.byref(nout))
    if rc:
        raise SystemExit(e._lib.musc_last_error(e._h).decode())
    return int(nout.value)


def workload(mbytes):
    import torch
    from muscato_amd import Engine
    text = dna_text(torch, mbytes)
    out = torch.empty(text.numel() + 8 * (text.numel() // CHUNK + 1) + 64, dtype=torch.uint8, device="cuda")
    with Engine(0) as e:
        for _ in range(3):
            n_stored = raw_call(e, e._lib.musc_sz_frame, text, out)
            n_comp = raw_call(e, e._lib.musc_sz_compress, text, out)
    print(json.dumps({"plain_bytes": text.numel(), "stored_stream": n_stored, "compressed_stream": n_comp}), flush=True)


def kernels(mbytes):
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "workload", str(mbytes)], stdout=subprocess.PIPE)
        if r.returncode:
            raise SystemExit("the traced run ended with %d" % r.returncode)
        info = json.loads(r.stdout.decode().strip().splitlines()[-1])
        (path,) = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        rows = {row["Name"].split("(")[0]: row for row in csv.DictReader(open(path))}
    rec = dict(info, mode="kernels")
    for k in ("k_sz_compress", "k_sz_gather", "k_sz_frame"):
        row = next(v for n, v in rows.items() if n.startswith(k))
        calls, total_ns = int(row["Calls"]), int(row["TotalDurationNs"])
        rec[k] = {"calls": calls, "mean_ms": round(total_ns / calls / 1e6, 3), "input_GB_per_s": round(info["plain_bytes"] * calls / total_ns, 2)}
    emit(rec)


def synth():
    import torch
    import sz_cases as sc
    from muscato_amd import Engine, synth as sy
    wl = sy.workload_for("cfg2")
    t = sy.gen_targets(wl, "cuda", sy.SEED_BASE)
    text = torch.cat([t, torch.full((t.shape[0], 1), 10, dtype=torch.uint8, device="cuda")], 1).reshape(-1).contiguous()
    out = torch.empty(text.numel() + 8 * (text.numel() // CHUNK + 1) + 64, dtype=torch.uint8, device="cuda")
    with Engine(0) as e:
        n_stored = raw_call(e, e._lib.musc_sz_frame, text, out)
        n_comp = raw_call(e, e._lib.musc_sz_compress, text, out)
        rng = random.Random(2)
        nch = text.numel() // CHUNK
        ours = seq = 0
        for k in sorted(rng.sample(range(nch), 24)):  # the sequential model is Python: two dozen chunks of the 1 500
            piece = bytes(text[k * CHUNK:(k + 1) * CHUNK].cpu().numpy())
            ours += len(e.sz_compress(piece)) - 10 - 8 - 3
            seq += sum(len(el[1]) for el in sc.compress(piece))
    emit({"mode": "synth", "workload": wl.name, "plain_bytes": text.numel(), "stored_stream": n_stored, "compressed_stream": n_comp,
          "ratio": round(text.numel() / n_comp, 3), "sampled_chunks": 24, "element_bytes_sampled": ours, "sequential_model_element_bytes_sampled": seq})


def tool(wd, mbytes, runs):
    from targets_prep import make_fasta
    os.makedirs(wd, exist_ok=True)
    make_fasta(os.path.join(wd, "genes.fasta"), mbytes)
    configs = [(where, write) for write in ("stored", "compressed") for where in ("host", "device")]
    wall = {c: [] for c in configs}
    size = {}
    for i in range(runs):
        for where, write in configs:
            env = dict(os.environ, MUSC_PREP_TARGETS=where, MUSC_SZ_WRITE=write)
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(BIN, "muscato_prep_targets"), "-rev", "genes.fasta"], cwd=wd, env=env, stderr=subprocess.PIPE)
            dt = time.perf_counter() - t0
            if r.returncode or (b"targets prep on the device" in r.stderr) != (where == "device"):
                raise SystemExit(r.stderr.decode())
            wall[(where, write)].append(round(dt, 3))
            size[(where, write)] = [os.path.getsize(os.path.join(wd, f)) for f in ("musc_genes.fasta.sz", "musc_ids_genes.fasta.sz")]
            emit({"mode": "tool", "run": i, "where": where, "write": write, "wall_s": round(dt, 3), "file_bytes": size[(where, write)]})
    assert size[("host", "stored")] == size[("device", "stored")] and size[("host", "compressed")] == size[("device", "compressed")]
    raw = os.path.getsize(os.path.join(wd, "genes.fasta"))
    framed, comp = sum(size[("host", "stored")]), sum(size[("host", "compressed")])
    text = sum(s - 10 - 8 * ((s - 10 + CHUNK + 7) // (CHUNK + 8)) for s in size[("host", "stored")])  # (a stored stream: 10 + 8 a chunk + the text)
    med = {c: statistics.median(v) for c, v in wall.items()}
    spread = {c: round(max(v) - min(v), 3) for c, v in wall.items()}

    def verdict(a, b):
        diff = med[a] - med[b]
        return {"median_difference_s": round(diff, 3), "three_spreads_s": round(3 * max(spread[a], spread[b]), 3), "counts": abs(diff) > 3 * max(spread[a], spread[b])}

    emit({"mode": "tool", "summary": True, "runs": runs, "input_bytes": raw, "text_bytes": text, "stored_bytes": framed, "compressed_bytes": comp,
          "median_s": {"%s/%s" % c: m for c, m in med.items()}, "spread_s": {"%s/%s" % c: s for c, s in spread.items()},
          "device_compressed_vs_stored": verdict(("device", "compressed"), ("device", "stored")),
          "host_compressed_vs_stored": verdict(("host", "compressed"), ("host", "stored")),
          "host_writer_MB_per_s": round(text / 1e6 / max(med[("host", "compressed")] - med[("host", "stored")], 1e-9), 1),
          # the device path: the input up; then, before musc_targets_prep_sz, both texts down, up again and the stream down
          "pcie_bytes_before": {"stored": raw + text + text + framed, "compressed": None},
          "pcie_bytes_now": {"stored": raw + framed, "compressed": raw + comp}})


def main(argv):
    mode = argv[0] if argv else "sizes"
    if mode == "sizes":
        sizes()
    elif mode == "synth":
        synth()
    elif mode == "workload":
        workload(int(argv[1]) if len(argv) > 1 else 256)
    elif mode == "kernels":
        kernels(int(argv[1]) if len(argv) > 1 else 256)
    elif mode == "tool":
        tool(argv[1], int(argv[2]) if len(argv) > 2 else 100, int(argv[3]) if len(argv) > 3 else 5)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
