"""The CLI with the MaxMatches truncation replayed on the host (MUSC_MAXMATCHES=host) and on the device (=device): the
four output files are the same byte for byte, on the cases of test_cli.test_cli_replays_maxmatches_truncation, and the
device run takes results.txt and the side outputs from the device."""
import json
import os
import random
import subprocess

import pytest

from muscato_amd import build as mbuild

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "muscato_amd", "bin")
OUTPUTS = ("result.txt", "result.nonmatch.txt.fastq", "result_genestats.txt", "result_readstats.txt")


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _run(d, mode, seed, where):
    rng = random.Random(seed)
    alpha = b"AC"
    targets = [bytes(rng.choice(alpha) for _ in range(rng.randint(20, 40))) for _ in range(30)]
    reads = sorted({bytes(rng.choice(alpha) for _ in range(rng.randint(10, 14))) for _ in range(25)})
    d.mkdir()
    (d / "genes.txt").write_bytes(b"".join(b"g%d\t%s\n" % (i, t) for i, t in enumerate(targets)))
    (d / "reads.fastq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"F" * len(r)) for i, r in enumerate(reads)))
    r = subprocess.run([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
           "ResultsFileName": "result.txt", "Windows": [0, 5], "WindowWidth": 4, "PMatch": 0.7, "MinDinuc": 0,
           "MaxReadLength": 50, "MaxMatches": 6, "MMTol": 2, "MatchMode": mode}
    (d / "config.json").write_text(json.dumps(cfg))
    env = {k: v for k, v in os.environ.items() if k not in ("MUSC_RESULTS", "MUSC_SIDE", "MUSC_MAXMATCHES")}
    env["MUSC_MAXMATCHES"] = where
    r = subprocess.run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], cwd=d, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"replaying the reference's truncation" in r.stderr
    logs = list((d / "muscato_logs").iterdir())
    assert len(logs) == 1
    return {o: (d / o).read_bytes() for o in OUTPUTS}, (logs[0] / "muscato.log").read_text()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [("first", 1), ("best", 1), ("first", 2), ("best", 3)])
def test_cli_host_and_device_replay_write_the_same_files(tmp_path, mode, seed):
    host, hlog = _run(tmp_path / "host", mode, seed, "host")
    dev, dlog = _run(tmp_path / "device", mode, seed, "device")
    for o in OUTPUTS:
        assert dev[o] == host[o], o
    assert host["result.txt"]
    assert "MaxMatches replay on the host" in hlog and "MaxMatches replay on the device" not in hlog
    assert "MaxMatches replay on the device" in dlog and "MaxMatches replay on the host" not in dlog
    for log in (hlog, dlog):
        assert "suspect probes" in log and "blocks truncated" in log
    # the device replay leaves its selection resident: results.txt and the side outputs are made from it there
    assert "results on the device" in dlog and "side outputs on the device" in dlog
    trunc = lambda log: [ln.split("MaxMatches: ")[1] for ln in log.splitlines() if "blocks truncated" in ln]
    assert trunc(hlog) == trunc(dlog)
