#!/usr/bin/env python3
"""The grids two stages really launch with MUSC_DEBUG_STAGE_GRID=3 and with the knob unset.

`prep_fastq` over the 3 300-record text of tests/test_gpu_stage_grid.py and `sz_decode` over its gene file of eleven
chunks run in a child process under `rocprofv3 --kernel-trace`, once per knob value, each a run of its own.  The table
(--out, default profiles/stage_grid_trace.txt) lists every kernel in launch order with its blocks under the knob and
without it; the runtime's own fill and copy kernels are left out and rocPRIM's are named by their configuration.
usage: stage_grid_trace.py [--out FILE]"""
import argparse
import collections
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "MUSC_DEBUG_STAGE_GRID"


def probe(knob):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    os.environ.pop(KNOB, None)
    if knob:
        os.environ[KNOB] = str(knob)
    import sz_cases as sc
    import test_gpu_stage_grid as T
    from muscato_amd import Engine
    c = T.fastq_case()
    text = T.gene_file()[0]
    with Engine(0) as e:
        T.probe_db(e)
        assert e.prep_fastq(c.raw, c.min_len, c.max_len)["n_records"] == 3300
        assert e.sz_decode(sc.frame(text, True)) == text


def launches(knob):
    """[((kernel, blocks, workgroup size), launches)] of one traced child, in the order of the first launch."""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                        "--probe", str(knob)], check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        (path,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    out = collections.OrderedDict()
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if name.startswith("__amd_rocclr"):
            continue
        m = re.search(r"wrapped_(\w+)_config", name)
        if name.startswith("rocprim::") and m:
            name = "rocprim " + m.group(1)
        key = (name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_X"]))
        out[key] = out.get(key, 0) + 1
    return list(out.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage_grid_trace.txt"))
    ap.add_argument("--probe", type=int, default=None)
    a = ap.parse_args()
    if a.probe is not None:
        return probe(a.probe)
    with_knob, without = launches(3), launches(0)
    if [(k[0], k[2], n) for k, n in with_knob] != [(k[0], k[2], n) for k, n in without]:
        raise SystemExit("the two runs launched different kernels")
    lines = ["# profiles/stage_grid_trace.py: rocprofv3 --kernel-trace of prep_fastq over the 3 300-record text of",
             "# tests/test_gpu_stage_grid.py and of sz_decode over its gene file of eleven chunks, once with MUSC_DEBUG_STAGE_GRID=3",
             "# and once with the knob unset (a run of its own each, MI355X).",
             "# per kernel in launch order: blocks with the knob at 3 | blocks with the knob unset | workgroup size | launches"]
    for ((name, b3, wg), n), ((_, b0, _), _) in zip(with_knob, without):
        lines.append("%-30s %5d | %5d | %4d | x%d" % (name, b3, b0, wg, n))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
