"""The CLI's -DbPartitionBases addition: the database matched in partitions of whole targets must give byte-identical
output files.  The flag surface itself (help text, a negative value) needs no GPU."""
import json
import os
import random

import pytest

from muscato_amd import build as mbuild
from oracle import muscato_oracle as orc

from test_cli import BIN, MUSCATO_CASES, _check_outputs, _stage_case, run


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _plan_logged(root):
    logs = list((root / "muscato_logs").iterdir())
    assert len(logs) == 1
    log = (logs[0] / "muscato.log").read_text()
    saved = json.loads((logs[0] / "config.json").read_text())
    return log, saved


def test_cli_partition_flag_help_and_errors(tmp_path):
    exe = os.path.join(BIN, "muscato")
    r = run([exe, "--help"], tmp_path)
    assert r.returncode == 0 and b"-DbPartitionBases int" in r.stdout
    assert b"most target bases indexed at once; 0 = automatic" in r.stdout
    # rejected by checkArgs, before any file or GPU is touched
    r = run([exe, "-ReadFileName=r.fastq", "-GeneFileName=g", "-GeneIdFileName=i", "-Windows=0", "-WindowWidth=4",
             "-MaxReadLength=10", "-DbPartitionBases=-5"], tmp_path)
    assert r.returncode == 1 and b"DbPartitionBases must be >= 0" in r.stderr


def test_lib_exports_partition_entry_points():
    from muscato_amd import _lib
    assert "musc_db_set_partition_bases" in _lib.SYMBOLS and "musc_db_partitions" in _lib.SYMBOLS
    import abi_header as ah
    assert ah.prototype("musc_db_set_partition_bases") == ("int", ["musc_ctx* ctx", "uint64_t max_bases"])
    assert ah.prototype("musc_db_partitions") == ("int", ["musc_ctx* ctx", "uint32_t* first_target", "uint32_t cap", "uint32_t* n"])
    from muscato_amd import Config
    assert Config().DbPartitionBases == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case,rev", MUSCATO_CASES + [("00", True), ("02", True)])
def test_cli_reference_fixture_partitioned(golden_dir, tmp_path, case, rev):
    d = _stage_case(golden_dir, tmp_path, case, rev)
    r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=data/muscato/%s/config.json" % case, "-DbPartitionBases=40",
             "--CPUProfile"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    _check_outputs(d)
    log, saved = _plan_logged(tmp_path)
    assert saved["DbPartitionBases"] == 40
    assert " partitions (targets " in log, log
    prof = json.loads((list((tmp_path / "muscato_logs").iterdir())[0] / "muscato_gpu_profile.json").read_text())
    assert prof[0]["partitions"] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [("first", 1), ("best", 3)])
def test_cli_replays_maxmatches_truncation_partitioned(tmp_path, mode, seed):
    """test_cli_replays_maxmatches_truncation with the database in partitions: the whole-database verdict starts the
    replay, and the replay (on the same setting) gives the literal oracle's output."""
    from oracle import literal
    rng = random.Random(seed)
    alpha = b"AC"
    targets = [bytes(rng.choice(alpha) for _ in range(rng.randint(20, 40))) for _ in range(30)]
    reads = sorted({bytes(rng.choice(alpha) for _ in range(rng.randint(10, 14))) for _ in range(25)})
    ocfg = orc.Config(Windows=[0, 5], WindowWidth=4, PMatch=0.7, MinDinuc=0, MaxReadLength=50,
                      MaxMatches=6, MMTol=2, MatchMode=mode)
    d = tmp_path
    (d / "genes.txt").write_bytes(b"".join(b"g%d\t%s\n" % (i, t) for i, t in enumerate(targets)))
    (d / "reads.fastq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"F" * len(r)) for i, r in enumerate(reads)))
    r = run([os.path.join(BIN, "muscato_prep_targets"), "genes.txt"], d)
    assert r.returncode == 0, r.stderr
    cfg = {"ReadFileName": "reads.fastq", "GeneFileName": "musc_genes.txt.sz", "GeneIdFileName": "musc_ids_genes.txt.sz",
           "ResultsFileName": "result.txt", "Windows": [0, 5], "WindowWidth": 4, "PMatch": 0.7, "MinDinuc": 0,
           "MaxReadLength": 50, "MaxMatches": 6, "MMTol": 2, "MatchMode": mode, "DbPartitionBases": 100}
    (d / "config.json").write_text(json.dumps(cfg))
    r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=config.json"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert b"replaying the reference's truncation" in r.stderr
    log, _ = _plan_logged(d)
    assert " partitions (targets " in log
    seqs, ids = orc.prep_targets_file(str(d / "genes.txt"), False)
    ureads = orc.uniqify(orc.prep_reads(orc.read_fastq((d / "reads.fastq").read_bytes()), ocfg))
    hits = literal.match_literal([u.seq for u in ureads], seqs, ocfg, bloom_size=4000000, num_hash=20)
    assert (d / "result.txt").read_bytes() == orc.results_text(hits, ureads, seqs, ids, ocfg)
