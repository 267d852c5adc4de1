"""The CLI's side outputs on the device (MUSC_SIDE): the nonmatch FASTQ and the two stats files must be
byte-identical whether the host parses results.txt again or the device makes them from the resident tuples -- on the
reference's five fixtures, on a multi-mapping workload with genes that share names, and with a hand-made id file whose
names hold a blank, where the device declines and the host functions run."""
import json
import os
import re

import pytest

from muscato_amd import build as mbuild

from test_cli import BIN, MUSCATO_CASES, _check_outputs, _stage_case, _sz, run
from test_cli_results import OUTPUTS, _workload

pytestmark = pytest.mark.gpu

DEVICE_LINE = "side outputs on the device: prepare "
FALLBACK_LINE = "side outputs on the host: "


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _run(cwd, config, where):
    env = {k: v for k, v in os.environ.items() if k not in ("MUSC_SIDE", "MUSC_RESULTS")}
    if where:
        env["MUSC_SIDE"] = where
    r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=" + config], cwd, env=env)
    assert r.returncode == 0, r.stderr.decode()
    logs = list((cwd / "muscato_logs").iterdir())
    assert len(logs) == 1
    return r.stderr, (logs[0] / "muscato.log").read_text().splitlines()


def _shape(lines):
    """Log lines without their clock and their figures: what must not differ between the two paths."""
    return [re.sub(r"\d+(\.\d+)?", "#", ln.split(" ", 1)[1]) for ln in lines if DEVICE_LINE not in ln and FALLBACK_LINE not in ln]


def _compare(host, device, want_device=True):
    (err_h, log_h, files_h), (err_d, log_d, files_d) = host, device
    for f in files_h:
        assert files_d[f] == files_h[f], f
    assert err_d == err_h
    assert _shape(log_d) == _shape(log_h)
    assert not any(DEVICE_LINE in ln or FALLBACK_LINE in ln for ln in log_h)
    assert sum(DEVICE_LINE in ln for ln in log_d) == (1 if want_device else 0), log_d
    assert sum(FALLBACK_LINE in ln for ln in log_d) == (0 if want_device else 1), log_d
    assert any("results on the device:" in ln for ln in log_d)


@pytest.mark.parametrize("case,rev", MUSCATO_CASES)
def test_cli_side_reference_fixture(golden_dir, tmp_path, case, rev):
    got = {}
    for where in ("host", "device"):
        top = tmp_path / where
        top.mkdir()
        d = _stage_case(golden_dir, top, case, rev)
        err, log = _run(top, "data/muscato/%s/config.json" % case, where)
        _check_outputs(d)  # result.nonmatch_e.txt among them
        got[where] = (err, log, {f: (d / f).read_bytes() for f in OUTPUTS})
    _compare(got["host"], got["device"])


CFG = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
       "ResultsFileName": "result.txt", "Windows": [0, 20], "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2,
       "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best"}


def _synthetic(tmp_path, hand_made_ids):
    got = {}
    for where in ("host", "device", None):
        d = tmp_path / str(where)
        d.mkdir()
        _workload(d)  # twenty homologous genes under thirteen names, multi-mapped reads, one read without a match
        cfg = dict(CFG)
        if hand_made_ids:
            genes = [ln.split(b"\t") for ln in (d / "genes.txt").read_bytes().splitlines()]
            ids = b"".join(b"%011d\tgene %d\t%d\n" % (g, g % 13, len(t)) for g, (_, t) in enumerate(genes))
            (d / "ids_by_hand.txt.sz").write_bytes(_sz(ids))
            cfg["GeneIdFileName"] = "ids_by_hand.txt.sz"
        (d / "config.json").write_text(json.dumps(cfg))
        err, log = _run(d, "config.json", where)
        got[where] = (err, log, {f: (d / f).read_bytes() for f in OUTPUTS})
    return got


def test_cli_side_duplicate_names_and_multi_mapped_reads(tmp_path):
    got = _synthetic(tmp_path, False)
    _compare(got["host"], got["device"])
    _compare(got["host"], got[None])  # the device is the default when results.txt came from it
    files = got["device"][2]
    lines = files["result.txt"].splitlines()
    assert len(lines) > 300 and len({ln.split(b"\t")[0] for ln in lines}) < len(lines) // 2  # most reads multi-map
    gs = files["result_genestats.txt"].splitlines()
    assert 1 < len(gs) <= 13 and sum(int(ln.split(b"\t")[1]) for ln in gs) == len(lines)
    assert files["result.nonmatch.txt.fastq"].count(b"\n") >= 4 and files["result_readstats.txt"].count(b";") > len(gs)


def test_cli_side_falls_back_for_a_gene_name_with_a_blank(tmp_path):
    got = _synthetic(tmp_path, True)
    _compare(got["host"], got["device"], want_device=False)
    _compare(got["host"], got[None], want_device=False)
    assert b"\tgene 3\t" in got["device"][2]["result.txt"]
