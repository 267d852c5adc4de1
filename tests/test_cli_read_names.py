"""The CLI's read prep with the names of the reads on the device (MUSC_PREP_NAMES): with the parse on the
device either way, every output is byte-identical with MUSC_PREP_NAMES=host and =device -- results.txt, the nonmatch
file, both stats files, seqinfo.json, stderr, the exit code and reads_sorted.txt.sz as framed -- on the reference's
fixtures and on a read file with a group of 70 reads and a name of 1 100 bytes.  Without MUSC_PREP=device the variable
changes nothing."""
import json
import os
import random

import pytest

from muscato_amd import build as mbuild
from oracle import muscato_oracle as orc

import fastq_cases as fc
import read_names_cases as rn
from cases import mutate, rand_seq
from test_cli import BIN, MUSCATO_CASES, _check_outputs, _stage_case, run

pytestmark = pytest.mark.gpu

OUTPUTS = ("result.txt", "result.nonmatch.txt.fastq", "result_genestats.txt", "result_readstats.txt")


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _run(cwd, d, config, names, prep="device"):
    """One run of the CLI from cwd (outputs in d) -> ({file: bytes}, the log): the four outputs, seqinfo.json, stderr, the
    exit code and reads_sorted.txt.sz."""
    env = {k: v for k, v in os.environ.items() if k not in ("MUSC_PREP", "MUSC_PREP_NAMES")}
    if prep:
        env["MUSC_PREP"] = prep
    if names:
        env["MUSC_PREP_NAMES"] = names
    r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=%s" % config, "--NoCleanTemp"], cwd, env=env)
    assert r.returncode == 0, r.stderr.decode()
    logs = list((cwd / "muscato_logs").iterdir())
    tmps = list((cwd / "muscato_tmp").iterdir())
    assert len(logs) == 1 and len(tmps) == 1
    log = (logs[0] / "muscato.log").read_text()
    assert ("read names on the device: " in log) == (names == "device" and prep == "device"), log
    assert "read names on the host" not in log and "read prep on the host" not in log  # (a device stage that found no memory)
    got = {f: (d / f).read_bytes() for f in OUTPUTS}
    got["seqinfo.json"] = (logs[0] / "seqinfo.json").read_bytes()
    got["reads_sorted.txt.sz"] = (tmps[0] / "reads_sorted.txt.sz").read_bytes()
    got["stderr"] = r.stderr
    got["exit"] = r.returncode
    return got, log


def _same(a, b):
    assert sorted(a) == sorted(b) and len(a) == 8
    for f in a:
        assert a[f] == b[f], f


@pytest.mark.parametrize("case,rev", MUSCATO_CASES)
def test_reference_fixture_names_host_and_device(golden_dir, tmp_path, case, rev):
    got = {}
    for names in ("host", "device"):
        cwd = tmp_path / names
        cwd.mkdir()
        d = _stage_case(golden_dir, cwd, case, rev)
        got[names], log = _run(cwd, d, "data/muscato/%s/config.json" % case, names)
        _check_outputs(d)
    _same(got["host"], got["device"])
    lines = orc.snappy_framed_decode(got["device"]["reads_sorted.txt.sz"])
    assert lines.count(b"\n") == json.loads(got["device"]["seqinfo.json"])["NumUnique"] > 0


def _read_file(d):
    """Genes, and a read file with a group of 70 reads under names out of order (tabs, a shared prefix, equal names), a
    name of 1 100 bytes, a group of three, and single reads."""
    rng = random.Random(43)
    genes = [rand_seq(rng, 200, b"ACGT")]
    while len(genes) < 12:
        genes.append(mutate(rng, rng.choice(genes), 0.02, b"ACGT"))
    (d / "genes.txt").write_bytes(b"".join(b"gene%d\t%s\n" % (i, t) for i, t in enumerate(genes)))

    def draw(n=60):
        g = rng.choice(genes)
        p = rng.randint(0, 200 - n)
        return mutate(rng, g[p:p + n], 0.02, b"ACGT")

    big, three = draw(), draw(45)
    names = [b"m%03d" % ((j * 37) % 70) + (b"\tcomment %d" % j if j % 3 == 0 else b"") for j in range(66)]
    names += [b"m", b"m0", b"m000", b"m000"]
    parts = [fc.record(n, big) for n in names]
    parts += [fc.record(b"L" * 1100, three), fc.record(b"L" * 994 + b"a", three), fc.record(b"K", three)]
    parts += [fc.record(b"r%d" % i, draw(rng.choice((40, 60)))) for i in range(40)]
    parts += [fc.record(b"withN", draw()[:30] + b"NN" + draw()[:28]), fc.record(b"nomatch", rand_seq(rng, 60, b"ACGT"))]
    rng.shuffle(parts)
    raw = b"".join(parts)
    (d / "reads.fastq").write_bytes(raw)
    r = run([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], d)
    assert r.returncode == 0, r.stderr
    return raw


def test_group_of_70_and_a_long_name(tmp_path):
    cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
           "ResultsFileName": "result.txt", "Windows": [0, 20], "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2,
           "MinReadLength": 20, "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best"}
    got = {}
    for names, prep in (("host", "device"), ("device", "device"), (None, "device"), ("device", None)):
        d = tmp_path / ("%s_%s" % (names, prep))
        d.mkdir()
        raw = _read_file(d)
        (d / "config.json").write_text(json.dumps(cfg))
        got[names, prep], log = _run(d, d, "config.json", names, prep)
        if (names, prep) == ("device", "device"):
            assert "1 sorted (70 pairs, " in log, log
    for k in got:
        _same(got["host", "device"], got[k])
    # and all are what the model says the read file holds
    m = rn.model(raw, 20, 60)
    assert m.info["n_sorted_groups"] == 1 and m.info["max_group"] == 70 and m.info["n_clipped_names"] == 1
    assert orc.snappy_framed_decode(got["device", "device"]["reads_sorted.txt.sz"]) == m.line_text
    assert got["device", "device"]["result.txt"].count(b"\n") > 40
