"""The CLI's coverage files (-CoverageFileName and its three flags, MUSC_COVERAGE): the same bytes whether
the host function or the device makes them, both the model's (tests/cov_cases.py); the other four outputs, the log and
the saved configuration of a run without the flag untouched; the device's refusal falling back to the host function."""
import json
import os
import re

import pytest

from muscato_amd import build as mbuild

import cov_cases as cc
from test_cli import BIN, MUSCATO_CASES, _check_outputs, _stage_case, run
from test_cli_results import OUTPUTS, _workload
from test_cov_cases import from_differences, parse
from test_sam_cases import fixture_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _run(cwd, args, where, ok=True):
    env = {k: v for k, v in os.environ.items() if k not in ("MUSC_COVERAGE", "MUSC_SAM", "MUSC_SIDE", "MUSC_RESULTS")}
    if where:
        env["MUSC_COVERAGE"] = where
    r = run([os.path.join(BIN, "muscato")] + args, cwd, env=env)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    logs = list((cwd / "muscato_logs").iterdir())
    assert len(logs) == 1
    return r, (logs[0] / "muscato.log").read_text().splitlines(), json.loads((logs[0] / "config.json").read_text())


def _cov_lines(log):
    return [ln.split(" ", 1)[1] for ln in log if "coverage" in ln.lower()]


def _files(d, name):
    return tuple((d / n).read_bytes() if (d / n).exists() else None for n in (name, name + "_targets"))


@pytest.mark.parametrize("case,rev", MUSCATO_CASES)
def test_cli_coverage_reference_fixture(golden_dir, tmp_path, case, rev):
    got = {}
    for where in (None, "host", "device"):
        top = tmp_path / str(where)
        top.mkdir()
        d = _stage_case(golden_dir, top, case, rev)
        args = ["-ConfigFileName=data/muscato/%s/config.json" % case]
        if where:
            args += ["-CoverageFileName=data/muscato/%s/result.bedgraph" % case, "-CoverageWeighted"] + (["-CoverageRev"] if rev else [])
        r, log, saved = _run(top, args, where)
        _check_outputs(d)
        got[where] = (r.stderr, log, saved, {f: (d / f).read_bytes() for f in OUTPUTS}, _files(d, "result.bedgraph"))
    # without the flag: no coverage file, no word of it in the log or in the saved configuration
    assert got[None][4] == (None, None) and not _cov_lines(got[None][1]) and not any("Coverage" in k for k in got[None][2])
    for where in ("host", "device"):
        assert got[where][3] == got[None][3]
        saved = got[where][2]
        assert saved["CoverageFileName"].endswith("result.bedgraph") and saved["CoverageRev"] is rev
        assert saved["CoverageWeighted"] is True and saved["CoverageUnique"] is False and not any("Sam" in k for k in saved)
        lines = _cov_lines(got[where][1])
        assert sum(ln.startswith("coverage files on the %s: " % where) for ln in lines) == 1, lines
        assert not any(ln.startswith("coverage files on the %s" % ("host" if where == "device" else "device")) for ln in lines)
        # the log of a run with the flag is the log without it plus the stage's own lines
        strip = lambda log: [re.sub(r"\d+(\.\d+)?", "#", ln.split(" ", 1)[1]) for ln in log if "coverage" not in ln.lower()]
        assert strip(got[where][1]) == strip(got[None][1])
    assert sum(ln.startswith("coverage on the device: ") for ln in _cov_lines(got["device"][1])) == 1
    assert got["host"][4] == got["device"][4] and all(got["host"][4])
    # ... and they are the model's bytes, over the lines of result_e.txt
    c, lines = fixture_case(golden_dir, case, rev, rev)
    bed, summary = cc.cov_of(c, c.hits, rev, True, False)
    assert got["device"][4] == (b"".join(bed), b"".join(summary)) and len(bed) > 0
    if rev:
        assert not any(rec.split(b"\t")[0].endswith(b"_r") for rec in summary)


def test_cli_coverage_multi_mapped_reads(tmp_path):
    """Twenty homologous genes, most reads on several of them, the flags as JSON keys: only the uniquely placed reads
    count, and numreads adds up to the lines of results.txt whose read is on no other line."""
    cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
           "ResultsFileName": "result.txt", "Windows": [0, 20], "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2,
           "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best", "CoverageFileName": "cov.bg", "CoverageUnique": True}
    got = {}
    for where in ("host", "device"):
        d = tmp_path / where
        d.mkdir()
        _workload(d)
        (d / "config.json").write_text(json.dumps(cfg))
        r, log, saved = _run(d, ["-ConfigFileName=config.json"], where)
        assert saved["CoverageFileName"] == "cov.bg" and saved["CoverageUnique"] is True and saved["CoverageWeighted"] is False
        assert sum(ln.startswith("coverage files on the %s: " % where) for ln in _cov_lines(log)) == 1
        got[where] = _files(d, "cov.bg") + ((d / "result.txt").read_bytes(),)
    assert got["host"] == got["device"]
    bed, summary, res = got["device"]
    per_read = {}
    for ln in res.splitlines():
        per_read[ln.split(b"\t")[0]] = per_read.get(ln.split(b"\t")[0], 0) + 1
    assert max(per_read.values()) > 1 and len(res.splitlines()) > 300
    single = sum(1 for v in per_read.values() if v == 1)
    assert single > 0 and sum(int(rec.split(b"\t")[2]) for rec in summary.splitlines()) == single
    assert len(summary.splitlines()) == 20 and len(bed.splitlines()) > 0


def test_cli_coverage_rev_on_a_database_without_pairs(tmp_path):
    """-CoverageRev with three targets: the device stage refuses (12), one line says so, and the host function, which
    holds the same rule, ends the run with its reason; results.txt has been written by then."""
    d = tmp_path
    (d / "genes.txt").write_bytes(b"g0\tACGTTGCATGCATGCCGATAGCTAGCTAACG\ng1\tTTGACCGATAGGCTAGCTTAGCGATCGATCG\ng2\tGGATCGATTAGCTAGGCTAGCTAGGATCGAT\n")
    (d / "reads.fastq").write_bytes(b"@r1\nTGCATGCATGCCGATAGC\n+\nFFFFFFFFFFFFFFFFFF\n")
    assert run([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], d).returncode == 0
    args = ["-ReadFileName=reads.fastq", "-GeneFileName=musc_genes.txt.sz", "-GeneIdFileName=musc_ids_genes.txt.sz",
            "-ResultsFileName=result.txt", "-Windows=0", "-WindowWidth=8", "-MaxReadLength=30", "-CoverageFileName=cov.bg"]
    r, log, _ = _run(d, args + ["-CoverageRev"], "device", ok=False)
    assert b"CoverageFileName: rev_pairs with an odd number of targets" in r.stderr
    assert sum(ln.startswith("coverage on the host: the device stage returned 12") for ln in _cov_lines(log)) == 1
    assert (d / "result.txt").read_bytes().count(b"\n") == 1 and not (d / "cov.bg").exists()


def test_cli_coverage_beside_the_sam_file(tmp_path):
    """Both additions in one run, each on either side: the same four files."""
    got = {}
    for cov, sam in (("host", "host"), ("device", "device"), ("host", "device"), ("device", "host")):
        d = tmp_path / (cov + sam)
        d.mkdir()
        (d / "genes.txt").write_bytes(b"g0\tACGTTGCATGCATGCCGATAGCTAGCTAACG\ng1\tTTGACCGATAGGCTAGCTTAGCGATCGATCG\n")
        (d / "reads.fastq").write_bytes(b"@r1\nTGCATGCATGCCGATAGC\n+\nFFFFFFFFFFFFFFFFFF\n@r2\nTGCATGCATGCCGATAGC\n+\nFFFFFFFFFFFFFFFFFF\n"
                                        b"@r3\nGATAGGCTAGCTTAGCGA\n+\nFFFFFFFFFFFFFFFFFF\n")
        assert run([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], d).returncode == 0
        args = ["-ReadFileName=reads.fastq", "-GeneFileName=musc_genes.txt.sz", "-GeneIdFileName=musc_ids_genes.txt.sz",
                "-ResultsFileName=result.txt", "-Windows=0", "-WindowWidth=8", "-MaxReadLength=30", "-CoverageFileName=cov.bg",
                "-CoverageWeighted", "-SamFileName=out.sam"]
        env = {k: v for k, v in os.environ.items() if k not in ("MUSC_SIDE", "MUSC_RESULTS")}
        env.update(MUSC_COVERAGE=cov, MUSC_SAM=sam)
        r = run([os.path.join(BIN, "muscato")] + args, d, env=env)
        assert r.returncode == 0, r.stderr.decode()
        log = (next((d / "muscato_logs").iterdir()) / "muscato.log").read_text()
        assert "coverage files on the %s: " % cov in log and "sam file on the %s: " % sam in log
        got[cov, sam] = _files(d, "cov.bg") + ((d / "out.sam").read_bytes(), (d / "result.txt").read_bytes())
    assert len(set(got.values())) == 1
    bed, summary, _, res = got["device", "device"]
    cols = [ln.split(b"\t") for ln in res.splitlines()]
    pieces = [(col[4], int(col[2]), len(col[1]), int(col[6])) for col in cols]
    assert len(cols) >= 1 and any(int(col[6]) == 2 for col in cols)
    assert parse(bed.splitlines(True), summary.splitlines(True)) == from_differences({b"g0": 31, b"g1": 31}, pieces)


def test_help_names_the_flags(tmp_path):
    r = run([os.path.join(BIN, "muscato"), "--help"], tmp_path)
    assert r.returncode == 0 and b"-CoverageFileName string" in r.stdout
    for flag in (b"-CoverageRev\n", b"-CoverageWeighted\n", b"-CoverageUnique\n"):
        assert flag in r.stdout
