"""The CLI over two GPUs (-GPUs=2): one thread and one context per shard, the gather, the other contexts gone before
the MaxMatches replay, and the whole post-chain on the host -- the four output files must be those of one GPU."""
import json
import os

import pytest

from muscato_amd import build as mbuild

from test_cli import BIN, run
from test_cli_results import CASES, OUTPUTS, _workload

PLACEMENT_KNOBS = ("MUSC_PREP", "MUSC_RESULTS", "MUSC_SIDE", "MUSC_MAXMATCHES", "MUSC_GATHER")


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _n_gpus():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.gpu
@pytest.mark.skipif(_n_gpus() < 2, reason="needs two GPUs: muscato -GPUs=2")
@pytest.mark.parametrize("case", ["plain", "replay"])
def test_cli_two_gpus_match_one(tmp_path, case):
    extra, stderr_has, _ = CASES[case]
    env = {k: v for k, v in os.environ.items() if k not in PLACEMENT_KNOBS}
    got = {}
    for gpus in (1, 2):
        d = tmp_path / str(gpus)
        d.mkdir()
        _workload(d)
        cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
               "ResultsFileName": "result.txt", "Windows": [0, 20], "WindowWidth": 12, "PMatch": 0.9, "MinDinuc": 2,
               "MaxReadLength": 60, "MMTol": 2, "MatchMode": "best"}
        cfg.update(extra)
        (d / "config.json").write_text(json.dumps(cfg))
        r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json", "-GPUs=%d" % gpus], d, env=env)
        assert r.returncode == 0, r.stderr.decode()
        if stderr_has:
            assert stderr_has in r.stderr
        logs = list((d / "muscato_logs").iterdir())
        log = (logs[0] / "muscato.log").read_text()
        assert ("results on the %s:" % ("device" if gpus == 1 else "host")) in log, log
        if gpus == 2:
            assert "results on the device:" not in log and "side outputs on the device" not in log, log
            assert "gpu 0: reads " in log and "gpu 1: reads " in log, log
            if case == "replay":
                assert "MaxMatches replay on the host: the post-chain of 2 GPUs" in log, log
        got[gpus] = {f: (d / f).read_bytes() for f in OUTPUTS}
    assert len(got[1]["result.txt"].splitlines()) > 300
    for f in OUTPUTS:
        assert got[2][f] == got[1][f], f
