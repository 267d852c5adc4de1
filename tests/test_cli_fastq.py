"""The CLI's read prep with the FASTQ parse on the device (MUSC_PREP): every output must be byte-identical
to the host path's -- results.txt, the nonmatch file, both stats files, seqinfo.json and the decoded
reads_sorted.txt.sz -- on the reference's fixtures (which must also equal their expected results) and on a read file
made of the awkward texts of tests/fastq_cases.py.  Without MUSC_PREP the host path runs, as before."""
import json
import os
import random

import pytest

from muscato_amd import build as mbuild
from oracle import muscato_oracle as orc

import fastq_cases as fc
from cases import mutate, rand_seq
from test_cli import BIN, MUSCATO_CASES, _check_outputs, _stage_case, run

pytestmark = pytest.mark.gpu

OUTPUTS = ("result.txt", "result.nonmatch.txt.fastq", "result_genestats.txt", "result_readstats.txt")


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _run(cwd, d, config, where):
    """One run of the CLI from cwd (outputs in d) -> {file: bytes}, with seqinfo.json and the decoded reads_sorted.txt.sz."""
    env = {k: v for k, v in os.environ.items() if k != "MUSC_PREP"}
    if where:
        env["MUSC_PREP"] = where
    r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=%s" % config, "--NoCleanTemp"], cwd, env=env)
    assert r.returncode == 0, r.stderr.decode()
    logs = list((cwd / "muscato_logs").iterdir())
    tmps = list((cwd / "muscato_tmp").iterdir())
    assert len(logs) == 1 and len(tmps) == 1
    log = (logs[0] / "muscato.log").read_text()
    assert ("read prep on the device: " in log) == (where == "device"), log
    assert "read prep on the host" not in log  # (the line of a device stage that found no memory)
    got = {f: (d / f).read_bytes() for f in OUTPUTS}
    got["seqinfo.json"] = (logs[0] / "seqinfo.json").read_bytes()
    got["reads_sorted.txt"] = orc.snappy_framed_decode((tmps[0] / "reads_sorted.txt.sz").read_bytes())
    return got, log


@pytest.mark.parametrize("case,rev", MUSCATO_CASES)
def test_reference_fixture_host_and_device(golden_dir, tmp_path, case, rev):
    got = {}
    for where in ("host", "device"):
        cwd = tmp_path / where
        cwd.mkdir()
        d = _stage_case(golden_dir, cwd, case, rev)
        got[where], log = _run(cwd, d, "data/muscato/%s/config.json" % case, where)
        _check_outputs(d)
    assert sorted(got["host"]) == sorted(got["device"]) and len(got["host"]) == 6
    for f in got["host"]:
        assert got["device"][f] == got["host"][f], f
    assert got["host"]["reads_sorted.txt"].count(b"\n") == json.loads(got["host"]["seqinfo.json"])["NumUnique"] > 0


def _awkward_reads(d):
    """Genes, and a read file in which reads drawn from them come as the awkward texts do: CRLF, names with tabs, names
    of 1000 and 1001 bytes, duplicates under names out of order, lowercase and N, a read below MinReadLength, one cut at
    MaxReadLength, the + and quality lines starting with @, and a dangling last record without a newline."""
    rng = random.Random(41)
    genes = [rand_seq(rng, 200, b"ACGT")]
    while len(genes) < 12:
        genes.append(mutate(rng, rng.choice(genes), 0.02, b"ACGT"))
    (d / "genes.txt").write_bytes(b"".join(b"gene%d\t%s\n" % (i, t) for i, t in enumerate(genes)))

    def draw(n=60):
        g = rng.choice(genes)
        p = rng.randint(0, 200 - n)
        return mutate(rng, g[p:p + n], 0.02, b"ACGT")

    dup, dup2 = draw(), draw(45)
    parts = [fc.record(b"r%d" % i, draw(rng.choice((40, 60)))) for i in range(60)]
    parts += [fc.record(b"crlf%d" % i, draw(), eol=b"\r\n") for i in range(5)]
    parts += [fc.record(n, dup) for n in (b"zeta", b"b\tzz", b"a\tyy", b"b", b"Zed", b"b!")]
    parts += [fc.record(b"n" * 999, dup2), fc.record(b"m" * 1000, dup2), fc.record(b"tab\there\tand here", dup2)]
    parts += [fc.record(b"q%02d" % i + b"x" * 120, dup2) for i in range(9)]
    parts += [fc.record(b"lower", draw().lower()), fc.record(b"withN", draw()[:30] + b"NN" + draw()[:28])]
    parts += [fc.record(b"short", draw(19)), fc.record(b"long", draw(90)), fc.record(b"cr_inside", draw(30) + b"\r" + draw(29))]
    parts += [fc.record(b"at", draw(), plus=b"@at again", qual=b"@" * 60), fc.record(b"nomatch", rand_seq(rng, 60, b"ACGT"))]
    rng.shuffle(parts)
    raw = b"".join(parts) + fc.record(b"last", draw())[:-1] + b"\n@dangling\nACGTACGTACGTACGTACGTACGTACGT"
    (d / "reads.fastq").write_bytes(raw)
    r = run([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], d)
    assert r.returncode == 0, r.stderr
    return raw


def test_awkward_read_file_host_device_and_default(tmp_path):
    cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
           "ResultsFileName": "result.txt", "Windows": [0, 20], "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2,
           "MinReadLength": 20, "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best"}
    got = {}
    for where in ("host", "device", None):
        d = tmp_path / str(where)
        d.mkdir()
        raw = _awkward_reads(d)
        (d / "config.json").write_text(json.dumps(cfg))
        got[where], log = _run(d, d, "config.json", where)
    for f in got["host"]:
        assert got["device"][f] == got["host"][f], f
        assert got[None][f] == got["host"][f], f
    # and both are what the model says the read file holds
    m = fc.model(raw, 20, 60)
    exp = b"".join(b"%s\t%d\t%s\n" % u for u in fc.unique(m))
    assert got["device"]["reads_sorted.txt"] == exp
    assert m.n_short == 1 and m.n_records == m.n_reads + 1 and b"X" in exp and b"\r" not in exp
    assert json.loads(got["device"]["seqinfo.json"]) == {"NumUnique": exp.count(b"\n"), "NumTotal": m.n_reads}
    assert got["device"]["result.txt"].count(b"\n") > 60
