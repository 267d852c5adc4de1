"""The CLI's target stage with the gene file on the device (MUSC_TARGETS): results.txt, the nonmatch file,
both stats files, stderr, the exit code and muscato.log -- but for the stage's own line and the times -- must be the
same with MUSC_TARGETS=host and MUSC_TARGETS=device, for a plain gene file, a framed one of uncompressed chunks, one
from the test's compressor, one with odd bytes (the same warning and the same demotion of the results), one with a chunk
beyond the format's 65 536 bytes (the device refuses, the host chain takes over) and a corrupt one (the run ends with
the host decoder's message and exit code).  Without MUSC_TARGETS the compiled default decides: the device."""
import json
import os
import random
import re

import pytest

from muscato_amd import build as mbuild

import sz_cases as sc
from cases import mutate, rand_seq
from test_cli import BIN, run

pytestmark = pytest.mark.gpu

OUTPUTS = ("result.txt", "result.nonmatch.txt.fastq", "result_genestats.txt", "result_readstats.txt")
CFG = {"ReadFileName": "reads.fastq", "GeneIdFileName": "ids.txt.sz", "ResultsFileName": "result.txt", "Windows": [0, 20],
       "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2, "MinReadLength": 20, "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best"}


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _inputs(odd=False, long_gene=False):
    """Genes (mutated copies of one another, so that reads land on several), their id lines, and reads drawn from them."""
    rng = random.Random(17)
    genes = [rand_seq(rng, 300, b"ACGT")]
    while len(genes) < 14:
        genes.append(mutate(rng, rng.choice(genes), 0.02, b"ACGT"))
    genes.insert(5, b"")
    if long_gene:
        genes.insert(3, rand_seq(rng, 70000, b"ACGT"))
    reads = []
    for i in range(80):
        g = rng.choice([g for g in genes if g])
        p = rng.randint(0, len(g) - 60)
        reads.append(b"@r%d\n%s\n+\n%s\n" % (i, mutate(rng, g[p:p + 60], 0.02, b"ACGT"), b"!" * 60))
    reads.append(b"@nowhere\n%s\n+\n%s\n" % (rand_seq(rng, 60, b"ACGT"), b"!" * 60))
    reads.append(b"@over_the_odd_byte\n%s\n+\n%s\n" % (genes[2][80:140], b"!" * 60))
    if odd:
        genes[2] = genes[2][:100] + b"N" + genes[2][101:150] + b"n" + genes[2][151:]
        genes[7] = genes[7][:-1] + b"R"
    text = b"".join(g + b"\t%011d\tgene%d\n" % (i, i) for i, g in enumerate(genes))  # (the columns behind the tab are cut)
    ids = b"".join(b"%011d\tgene%d\t%d\n" % (i, i, len(g)) for i, g in enumerate(genes))
    return text, ids, b"".join(reads)


def _normal_log(log):
    lines = []
    for ln in log.splitlines():
        ln = re.sub(r"^\d\d:\d\d:\d\d ", "", ln)
        if ln.startswith("targets on the "):
            continue
        lines.append(re.sub(r"\d+\.\d+", "#", ln))
    return lines


def _run(d, gene_name, gene_bytes, ids, reads, where, gpus=1):
    d.mkdir()
    (d / gene_name).write_bytes(gene_bytes)
    (d / "ids.txt.sz").write_bytes(sc.frame(ids, False))
    (d / "reads.fastq").write_bytes(reads)
    (d / "config.json").write_text(json.dumps(dict(CFG, GeneFileName=gene_name)))
    env = {k: v for k, v in os.environ.items() if k != "MUSC_TARGETS"}
    if where:
        env["MUSC_TARGETS"] = where
    r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json", "-GPUs=%d" % gpus], d, env=env)
    logs = list((d / "muscato_logs").iterdir())
    assert len(logs) == 1
    log = (logs[0] / "muscato.log").read_text()
    out = {f: (d / f).read_bytes() for f in OUTPUTS if (d / f).exists()}
    return r, log, out


def _both(tmp_path, gene_name, gene_bytes, ids, reads, gpus=1):
    h = _run(tmp_path / "host", gene_name, gene_bytes, ids, reads, "host", gpus)
    v = _run(tmp_path / "device", gene_name, gene_bytes, ids, reads, "device", gpus)
    assert h[0].returncode == v[0].returncode
    assert h[0].stderr == v[0].stderr
    assert h[2] == v[2]
    assert _normal_log(h[1]) == _normal_log(v[1])
    assert "targets on the " not in h[1]
    return h, v


@pytest.mark.parametrize("form", ["plain", "sz-uncompressed", "sz-compressed"])
def test_host_and_device_agree(tmp_path, form):
    text, ids, reads = _inputs()
    name, data = {"plain": ("genes.txt", text), "sz-uncompressed": ("genes.txt.sz", sc.frame(text, False, chunk_bytes=1500)),
                  "sz-compressed": ("genes.txt.sz", sc.frame(text, True))}[form]
    h, v = _both(tmp_path, name, data, ids, reads)
    assert h[0].returncode == 0, h[0].stderr.decode()
    assert len(h[2]) == 4 and h[2]["result.txt"].count(b"\n") > 80
    n_chunks = {"plain": 0, "sz-uncompressed": (len(text) + 1499) // 1500, "sz-compressed": 1}[form]
    assert "targets on the device: 15 targets, 4200 bases, %d bytes of text in %d chunks, " % (len(text), n_chunks) in v[1]
    # without the variable the compiled default decides: the device (DESIGN.md 21's measurement)
    d = _run(tmp_path / "default", name, data, ids, reads, None)
    assert d[0].returncode == 0 and d[2] == h[2] and "targets on the device: 15 targets" in d[1]
    assert _normal_log(d[1]) == _normal_log(h[1])


def test_a_framed_stream_under_a_plain_name(tmp_path):
    """The stream identifier decides, as for every input of the reference's tools."""
    text, ids, reads = _inputs()
    h, v = _both(tmp_path, "genes.txt", sc.frame(text, True), ids, reads)
    assert h[0].returncode == 0 and "targets on the device: 15 targets" in v[1] and len(h[2]) == 4


def test_odd_target_bytes(tmp_path):
    text, ids, reads = _inputs(odd=True)
    h, v = _both(tmp_path, "genes.txt.sz", sc.frame(text, True), ids, reads)
    assert h[0].returncode == 0, h[0].stderr.decode()
    assert b"Warning: 3 target bytes are none of ACGTX (first in target 2); they are treated as X" in v[0].stderr
    assert "3 target bytes are none of ACGTX (first in target 2)" in v[1]
    assert "results on the host: the targets hold bytes that are none of ACGTX" in v[1] and "targets on the device: " in v[1]
    assert any(b"N" in ln.split(b"\t")[1] for ln in v[2]["result.txt"].splitlines())  # the target's own bytes are quoted


def test_a_chunk_beyond_the_format_is_refused_and_the_host_takes_over(tmp_path):
    text, ids, reads = _inputs(long_gene=True)
    assert len(text) > 65537 + 2000
    stream = sc.STREAM_ID + sc.plain_chunk(text[:2000]) + sc.plain_chunk(text[2000:2000 + 65537]) + sc.frame(text[2000 + 65537:], True, ident=False)
    h, v = _both(tmp_path, "genes.txt.sz", stream, ids, reads)
    assert h[0].returncode == 0, h[0].stderr.decode()
    assert "targets on the host: the device stage returned 12 (musc_db_load_text: chunk 2: sz: a chunk declares more than 65536 " \
           "uncompressed bytes)" in v[1]
    assert len(h[2]) == 4 and h[2]["result.txt"].count(b"\n") > 80


def test_a_corrupt_stream_ends_the_run_as_on_the_host(tmp_path):
    text, ids, reads = _inputs()
    stream = bytearray(sc.frame(text, True))
    stream[len(stream) // 2] ^= 0x40
    h, v = _both(tmp_path, "genes.txt.sz", bytes(stream), ids, reads)
    assert h[0].returncode != 0 and (b"sz: " in h[0].stderr or b"snappy: " in h[0].stderr)
    assert "targets on the host: the device stage returned 13 (musc_db_load_text: chunk 1: " in v[1]
    assert not h[2] and not v[2]


def test_two_gpus(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    text, ids, reads = _inputs()
    h, v = _both(tmp_path, "genes.txt.sz", sc.frame(text, True), ids, reads, gpus=2)
    assert h[0].returncode == 0, h[0].stderr.decode()
    assert "targets on the device: 15 targets" in v[1] and len(h[2]) == 4
