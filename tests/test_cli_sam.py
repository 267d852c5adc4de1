"""The CLI's SAM file (-SamFileName, -SamRev, MUSC_SAM): the same bytes whether the host function or the
device writes it, both the model's (tests/sam_cases.py); the other four outputs, the log and the saved configuration of
a run without the flag untouched; the reference's `-rev` fixture back through the inverse to result_e.txt."""
import json
import os
import re

import pytest

from muscato_amd import build as mbuild

import sam_cases as sc
from test_cli import BIN, MUSCATO_CASES, _check_outputs, _stage_case, run
from test_cli_results import OUTPUTS, _workload
from test_sam_cases import fixture_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _run(cwd, args, where, ok=True):
    env = {k: v for k, v in os.environ.items() if k not in ("MUSC_SAM", "MUSC_SIDE", "MUSC_RESULTS")}
    if where:
        env["MUSC_SAM"] = where
    r = run([os.path.join(BIN, "muscato")] + args, cwd, env=env)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    logs = list((cwd / "muscato_logs").iterdir())
    assert len(logs) == 1
    return r, (logs[0] / "muscato.log").read_text().splitlines(), json.loads((logs[0] / "config.json").read_text())


def _sam_lines(log):
    return [ln.split(" ", 1)[1] for ln in log if "sam" in ln.lower()]


@pytest.mark.parametrize("case,rev", MUSCATO_CASES)
def test_cli_sam_reference_fixture(golden_dir, tmp_path, case, rev):
    got = {}
    for where in (None, "host", "device"):
        top = tmp_path / str(where)
        top.mkdir()
        d = _stage_case(golden_dir, top, case, rev)
        args = ["-ConfigFileName=data/muscato/%s/config.json" % case]
        if where:
            args += ["-SamFileName=data/muscato/%s/result.sam" % case] + (["-SamRev"] if rev else [])
        r, log, saved = _run(top, args, where)
        _check_outputs(d)
        got[where] = (r.stderr, log, saved, {f: (d / f).read_bytes() for f in OUTPUTS},
                      (d / "result.sam").read_bytes() if (d / "result.sam").exists() else None)
    # without the flag: no SAM file, no word of it in the log or in the saved configuration
    assert got[None][4] is None and not _sam_lines(got[None][1]) and not any("Sam" in k for k in got[None][2])
    for where in ("host", "device"):
        assert got[where][3] == got[None][3]
        assert got[where][2]["SamFileName"].endswith("result.sam") and got[where][2]["SamRev"] is rev
        lines = _sam_lines(got[where][1])
        assert sum(ln.startswith("sam file on the %s: " % where) for ln in lines) == 1, lines
        assert not any(ln.startswith("sam file on the %s" % ("host" if where == "device" else "device")) for ln in lines)
        # the log of a run with the flag is the log without it plus the stage's own lines
        strip = lambda log: [re.sub(r"\d+(\.\d+)?", "#", ln.split(" ", 1)[1]) for ln in log if "sam" not in ln.lower()]
        assert strip(got[where][1]) == strip(got[None][1])
    assert sum(ln.startswith("sam on the device: ") for ln in _sam_lines(got["device"][1])) == 1
    assert got["host"][4] == got["device"][4] and got["host"][4]
    # ... and they are the model's bytes, over the lines of result_e.txt in the file's order
    c, lines = fixture_case(golden_dir, case, rev, rev)
    hdr = sc.header(c.targets, c.rests, (), rev)
    recs = sc.records(c.reads, c.targets, c.rests, c.tails, c.hits, rev)
    assert got["device"][4] == hdr + b"".join(recs)
    # back through the inverse to result_e.txt
    sam = got["device"][4].splitlines(True)
    nh = sum(ln.startswith(b"@") for ln in sam)
    assert b"".join(sam[:nh]) == hdr and len(sam) - nh == len(lines)
    for rec, col in zip(sam[nh:], lines):
        assert sc.invert(hdr, rec) == (col[0], col[1], int(col[2]), col[4])
    if rev:
        assert any(int(r.split(b"\t")[1]) & 16 for r in sam[nh:])


def test_cli_sam_multi_mapped_reads(tmp_path):
    """Twenty homologous genes, most reads on several of them: NH above one, secondary records, mismatches in MD."""
    cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
           "ResultsFileName": "result.txt", "Windows": [0, 20], "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2,
           "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best", "SamFileName": "result.sam"}
    got = {}
    for where in ("host", "device"):
        d = tmp_path / where
        d.mkdir()
        _workload(d)
        (d / "config.json").write_text(json.dumps(cfg))  # the flags as JSON keys
        r, log, saved = _run(d, ["-ConfigFileName=config.json"], where)
        assert saved["SamFileName"] == "result.sam" and saved["SamRev"] is False
        assert sum(ln.startswith("sam file on the %s: " % where) for ln in _sam_lines(log)) == 1
        got[where] = ((d / "result.sam").read_bytes(), (d / "result.txt").read_bytes())
    assert got["host"] == got["device"]
    sam, res = got["device"]
    recs = [ln for ln in sam.splitlines() if not ln.startswith(b"@")]
    assert len(recs) == res.count(b"\n") > 300
    assert any(b"\tNH:i:1\t" not in r for r in recs) and any(int(r.split(b"\t")[1]) & 256 for r in recs)
    assert any(b"MD:Z:" in r and not r.split(b"MD:Z:")[1].split(b"\t")[0].isdigit() for r in recs)
    for rec, line in zip(recs, res.splitlines()):
        col = line.split(b"\t")
        assert rec.split(b"\t")[9] == col[0] and int(rec.split(b"\t")[3]) == int(col[2]) + 1 and rec.split(b"\t")[2] == col[4]


def test_cli_sam_rev_on_a_database_without_pairs(tmp_path):
    """-SamRev with three targets: the device stage refuses (12), one line says so, and the host function, which holds
    the same rule, ends the run with its reason; results.txt has been written by then."""
    d = tmp_path
    (d / "genes.txt").write_bytes(b"g0\tACGTTGCATGCATGCCGATAGCTAGCTAACG\ng1\tTTGACCGATAGGCTAGCTTAGCGATCGATCG\ng2\tGGATCGATTAGCTAGGCTAGCTAGGATCGAT\n")
    (d / "reads.fastq").write_bytes(b"@r1\nTGCATGCATGCCGATAGC\n+\nFFFFFFFFFFFFFFFFFF\n")
    assert run([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], d).returncode == 0
    args = ["-ReadFileName=reads.fastq", "-GeneFileName=musc_genes.txt.sz", "-GeneIdFileName=musc_ids_genes.txt.sz",
            "-ResultsFileName=result.txt", "-Windows=0", "-WindowWidth=8", "-MaxReadLength=30", "-SamFileName=result.sam", "-SamRev"]
    r, log, _ = _run(d, args, "device", ok=False)
    assert b"SamFileName: rev_pairs with an odd number of targets" in r.stderr
    assert sum(ln.startswith("sam on the host: the device stage returned 12") for ln in _sam_lines(log)) == 1
    assert (d / "result.txt").read_bytes().count(b"\n") == 1 and not (d / "result.sam").exists()


def test_help_names_both_flags(tmp_path):
    r = run([os.path.join(BIN, "muscato"), "--help"], tmp_path)
    assert r.returncode == 0 and b"-SamFileName string" in r.stdout and b"-SamRev\n" in r.stdout
    assert r.stdout.count(b"(addition)") >= 6
