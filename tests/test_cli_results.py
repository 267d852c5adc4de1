"""The CLI's results stage on the device (MUSC_RESULTS): results.txt and the three side outputs must be
byte-identical whether the lines are ordered and rendered on the host, on the device, or wherever the default puts
them -- on a multi-mapping workload, after the MaxMatches replay (a host list) and with the database in partitions.
A gene file with a letter the device cannot quote (an N that muscato_prep_targets left in the last FASTA record) keeps
the host path on every setting."""
import json
import os
import random

import pytest

from muscato_amd import build as mbuild
from oracle import muscato_oracle as orc

from cases import mutate, rand_seq
from test_cli import BIN, run

OUTPUTS = ("result.txt", "result.nonmatch.txt.fastq", "result_genestats.txt", "result_readstats.txt")


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _workload(d, fasta_with_n=False):
    """Twenty homologous genes (copies of one another with a few substitutions) and reads sampled from them: most reads
    map to several genes, many at the same position with the same mismatch count.  fasta_with_n: the genes come as a
    FASTA file whose last record holds an N, which muscato_prep_targets leaves as it is
    (cmd/muscato_prep_targets/main.go:204-212)."""
    rng = random.Random(21)
    genes = [rand_seq(rng, 200, b"ACGT")]
    while len(genes) < 20:
        genes.append(mutate(rng, rng.choice(genes), 0.02, b"ACGT"))
    reads = []
    for i in range(150):
        g = rng.choice(genes)
        p = rng.randint(0, 140)
        reads.append(mutate(rng, g[p:p + rng.choice((40, 60))], 0.02, b"ACGT"))
    reads += reads[:10]  # duplicates: counts above one, several names
    if fasta_with_n:  # (after the reads were drawn: no read holds the N, so the reference counts what the GPU counts)
        genes[-1] = genes[-1][:100] + b"N" + genes[-1][101:]
    reads.append(rand_seq(rng, 60, b"ACGT"))  # a read without a match
    names = [b"gene%d" % (i % 13) for i in range(len(genes))]  # some genes share a name
    if fasta_with_n:
        (d / "genes.fasta").write_bytes(b"".join(b">%s\n%s\n%s\n" % (n, t[:80], t[80:]) for n, t in zip(names, genes)))
    else:
        (d / "genes.txt").write_bytes(b"".join(b"%s\t%s\n" % (n, t) for n, t in zip(names, genes)))
    (d / "reads.fastq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"F" * len(r)) for i, r in enumerate(reads)))
    r = run([os.path.join(BIN, "muscato_prep_targets"), "genes.fasta" if fasta_with_n else "genes.txt"], d)
    assert r.returncode == 0, r.stderr


CASES = {
    "plain": ({}, None, None),
    "replay": ({"MaxMatches": 10}, b"replaying the reference's truncation", None),
    "partitions": ({"DbPartitionBases": 1400}, None, "database in 3 partitions (targets "),
    # an N in the last gene, inside the span of many hits: results.txt quotes the N, which only the host can
    "n_in_target": ({}, b"target bytes are none of ACGTX", None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_cli_results_identical_on_host_and_device(tmp_path, case):
    extra, stderr_has, log_has = CASES[case]
    got = {}
    for where in ("host", "device", None):
        d = tmp_path / str(where)
        d.mkdir()
        gfile = "genes.fasta" if case == "n_in_target" else "genes.txt"
        _workload(d, case == "n_in_target")
        cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_%s.sz" % gfile, "GeneIdFileName": "musc_ids_%s.sz" % gfile,
               "ResultsFileName": "result.txt", "Windows": [0, 20], "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2,
               "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best"}
        cfg.update(extra)
        (d / "config.json").write_text(json.dumps(cfg))
        env = {k: v for k, v in os.environ.items() if k != "MUSC_RESULTS"}
        if where:
            env["MUSC_RESULTS"] = where
        r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], d, env=env)
        assert r.returncode == 0, r.stderr.decode()
        if stderr_has:
            assert stderr_has in r.stderr
        logs = list((d / "muscato_logs").iterdir())
        log = (logs[0] / "muscato.log").read_text()
        if log_has:
            assert log_has in log, log
        # which path wrote the file: the device unless the host is asked for (it is the default with one GPU) -- but for
        # targets with letters the device cannot quote, which stay on the host whatever is asked for
        path = "host" if where == "host" or case == "n_in_target" else "device"
        assert "results on the %s:" % path in log, log
        assert ("results on the %s:" % ("device" if path == "host" else "host")) not in log, log
        got[where] = {f: (d / f).read_bytes() for f in OUTPUTS}
    lines = got["host"]["result.txt"].splitlines()
    assert len(lines) > 300 and len({ln.split(b"\t")[0] for ln in lines}) < len(lines) // 2  # most reads multi-map
    for f in OUTPUTS:
        assert got["device"][f] == got["host"][f], f
        assert got[None][f] == got["host"][f], f
    if case == "n_in_target":
        spans = [ln.split(b"\t")[1] for ln in lines]
        assert sum(b"N" in sp for sp in spans) >= 5 and not any(b"X" in sp for sp in spans)
    if case != "replay":
        ocfg = orc.Config(Windows=[0, 20], WindowWidth=12, PMatch=0.9, MinDinuc=2, MaxReadLength=60, MMTol=2, MatchMode="best")
        d = tmp_path / "host"
        seqs, ids = orc.prep_targets_file(str(d / gfile), False)
        ureads = orc.uniqify(orc.prep_reads(orc.read_fastq((d / "reads.fastq").read_bytes()), ocfg))
        hits = orc.match_direct([u.seq for u in ureads], seqs, ocfg)
        assert got["device"]["result.txt"] == orc.results_text(hits, ureads, seqs, ids, ocfg)
