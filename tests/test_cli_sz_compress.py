"""The tools with MUSC_SZ_WRITE.  Without a GPU: `muscato_prep_targets` on the reference's eight fixtures
writes, with `compressed`, two files that decode to the expected texts, are the model's bytes
(tests/sz_compress_cases.py) and are smaller than the stored ones; with the variable unset, `stored` or misspelt it
writes what it always wrote.  With a GPU (the stage tools and `muscato` need one): the device path of
`muscato_prep_targets` writes the host path's compressed files; `muscato_screen`, `muscato_confirm` and `muscato` give
the same results with the variable set, and their .sz files decode to the same texts."""
import json
import os
import shutil
import subprocess

import pytest

from muscato_amd import build as mbuild

import sz_cases as sc
import sz_compress_cases as zc
import targets_prep_cases as tp
from cases import make_case

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "muscato_amd", "bin")
FIXTURES = [("00", "genes.fasta", False), ("01", "genes.fasta", True), ("02", "genes.txt", False), ("03", "genes.txt", True),
            ("04", "genes.txt.gz", False), ("05", "genes.txt.gz", True), ("06", "genes.txt.sz", True), ("07", "genes.txt.sz", True)]
SMALL = 400  # a text of a few hundred bytes may not shrink: a chunk's first tile finds only its own near candidates


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def run(cmd, cwd, **env):
    e = dict(os.environ)
    for k in ("MUSC_SZ_WRITE", "MUSC_PREP_TARGETS"):
        e.pop(k, None)
    e.update({k: v for k, v in env.items() if v is not None})
    return subprocess.run(cmd, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def prep(d, fname, rev, write, side="host"):
    """muscato_prep_targets on d/fname in a directory of its own -> (exit code, stderr lines, {file: bytes})"""
    w = d / ("%s_%s" % (side, write))
    w.mkdir()
    shutil.copy(d / fname, w / fname)
    r = run([os.path.join(BIN, "muscato_prep_targets")] + (["-rev"] if rev else []) + [fname], w, MUSC_SZ_WRITE=write, MUSC_PREP_TARGETS=side)
    return r.returncode, r.stderr.decode(errors="replace").splitlines(), {f: (w / f).read_bytes() for f in sorted(os.listdir(w)) if f != fname}


def fixture(golden_dir, tmp_path, case, fname):
    shutil.copy(os.path.join(golden_dir, "prep_targets", case, fname), tmp_path / fname)
    os.chmod(tmp_path / fname, 0o644)
    stem = fname[:-3] if fname.endswith((".gz", ".sz")) else fname
    texts = {}
    for f, exp in (("musc_%s.sz" % stem, "expected_sequences.txt"), ("musc_ids_%s.sz" % stem, "expected_ids.txt")):
        with open(os.path.join(golden_dir, "prep_targets", case, exp), "rb") as g:
            texts[f] = g.read()
    return texts


@pytest.mark.parametrize("case,fname,rev", FIXTURES)
def test_fixtures_compressed_on_the_host(golden_dir, tmp_path, case, fname, rev):
    texts = fixture(golden_dir, tmp_path, case, fname)
    code, err, files = prep(tmp_path, fname, rev, "compressed")
    assert code == 0 and sorted(files) == sorted(texts), err
    for f, text in texts.items():
        assert sc.ref_decode(files[f]) == text
        assert files[f] == zc.model(text)
        assert len(files[f]) <= len(sc.frame(text, False))
        if len(text) > SMALL:
            assert len(files[f]) < len(sc.frame(text, False)), "%s: %d bytes of text" % (f, len(text))


@pytest.mark.parametrize("name,rev", [("fa_lens_big", True), ("tx_nrec_2100", False)])
def test_larger_texts_shrink_on_the_host(tmp_path, name, rev):
    """(The fixtures' texts are of 39 to 136 bytes; these are of many kilobytes.)"""
    c = {c.name: c for c in tp.all_cases()}[name]
    fname = "genes.fasta" if c.fasta else "genes.txt"
    (tmp_path / fname).write_bytes(c.text)
    seqs, ids = tp.texts_of(tp.model(c.text, c.fasta, rev))
    code, err, files = prep(tmp_path, fname, rev, "compressed")
    assert code == 0 and files == {"musc_%s.sz" % fname: zc.model(seqs), "musc_ids_%s.sz" % fname: zc.model(ids)}, err
    assert len(seqs) > SMALL
    for f, text in (("musc_%s.sz" % fname, seqs), ("musc_ids_%s.sz" % fname, ids)):
        assert len(text) <= SMALL or len(files[f]) < len(sc.frame(text, False))
    assert name != "tx_nrec_2100" or len(ids) > SMALL


@pytest.mark.parametrize("write", [None, "stored", "", "Compressed", "yes"])
def test_fixtures_stored_by_default(golden_dir, tmp_path, write):
    for case, fname, rev in (FIXTURES[1], FIXTURES[7]):
        d = tmp_path / case
        d.mkdir()
        texts = fixture(golden_dir, d, case, fname)
        code, err, files = prep(d, fname, rev, write)
        assert code == 0 and files == {f: sc.frame(t, False) for f, t in texts.items()}, err


# ---------------------------------------------------------------- with a GPU

@pytest.mark.gpu
@pytest.mark.parametrize("case,fname,rev", FIXTURES)
def test_fixtures_compressed_on_the_device(golden_dir, tmp_path, case, fname, rev):
    fixture(golden_dir, tmp_path, case, fname)
    hc, herr, hfiles = prep(tmp_path, fname, rev, "compressed", "host")
    dc, derr, dfiles = prep(tmp_path, fname, rev, "compressed", "device")
    own = [l for l in derr if l.startswith("targets prep on the ")]
    assert len(own) == 1 and own[0].startswith("targets prep on the device: "), derr
    assert dc == hc == 0 and [l for l in derr if l not in own] == herr and dfiles == hfiles
    sc_, ss, sfiles = prep(tmp_path, fname, rev, "stored", "device")  # and the stored files as before
    assert sc_ == 0 and {f: sc.ref_decode(b) for f, b in sfiles.items()} == {f: sc.ref_decode(b) for f, b in hfiles.items()}
    assert all(b == sc.frame(sc.ref_decode(b), False) for b in sfiles.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name,rev", [("fa_3_tiles", True), ("fa_lens_big", False), ("tx_lens_big", True), ("tx_nrec_2100", False), ("empty_fa", True)])
def test_seeded_cases_compressed_on_the_device(tmp_path, name, rev):
    c = {c.name: c for c in tp.all_cases()}[name]
    fname = "genes.fasta" if c.fasta else "genes.txt"
    (tmp_path / fname).write_bytes(c.text)
    seqs, ids = tp.texts_of(tp.model(c.text, c.fasta, rev))
    want = {"musc_%s.sz" % fname: zc.model(seqs), "musc_ids_%s.sz" % fname: zc.model(ids)}
    assert prep(tmp_path, fname, rev, "compressed", "host")[::2] == (0, want)
    assert prep(tmp_path, fname, rev, "compressed", "device")[::2] == (0, want)


@pytest.mark.gpu
@pytest.mark.parametrize("case,rev", [("00", False), ("04", True)])
def test_muscato_with_compressed_files(golden_dir, tmp_path, case, rev):
    """The whole tool on a reference fixture: the same results and side outputs, reads_sorted.txt.sz the same text."""
    outs = {}
    for write in ("stored", "compressed"):
        root = tmp_path / write
        d = root / "data" / "muscato" / case
        shutil.copytree(os.path.join(golden_dir, "muscato", case), d)
        os.chmod(d, 0o755)
        for f in d.iterdir():
            os.chmod(f, 0o644)
        r = run([os.path.join(BIN, "muscato_prep_targets")] + (["-rev"] if rev else []) + ["genes.txt"], d, MUSC_SZ_WRITE=write)
        assert r.returncode == 0, r.stderr
        shutil.copy(d / "musc_genes.txt.sz", d / "genes.txt.sz")
        shutil.copy(d / "musc_ids_genes.txt.sz", d / "genes_ids.txt.sz")
        r = run([os.path.join(BIN, "muscato"), "-ConfigFileName=data/muscato/%s/config.json" % case, "--NoCleanTemp"], root, MUSC_SZ_WRITE=write)
        assert r.returncode == 0, r.stderr.decode()
        tmps = list((root / "muscato_tmp").iterdir())
        assert len(tmps) == 1
        outs[write] = ({f: (d / f).read_bytes() for f in ("result.txt", "result.nonmatch.txt.fastq", "result_genestats.txt", "result_readstats.txt")},
                       {f: (d / f).read_bytes() for f in ("genes.txt.sz", "genes_ids.txt.sz")}, (tmps[0] / "reads_sorted.txt.sz").read_bytes())
    (res_s, gene_s, reads_s), (res_c, gene_c, reads_c) = outs["stored"], outs["compressed"]
    assert res_c == res_s and res_s["result.txt"] == (tmp_path / "stored" / "data" / "muscato" / case / "result_e.txt").read_bytes()
    text = sc.ref_decode(reads_s)
    # (the fixture's read text is six lines, under 200 bytes: it need not shrink, but it never grows)
    assert text and reads_s == sc.frame(text, False) and reads_c == zc.model(text) and len(reads_c) <= len(reads_s)
    for f in gene_s:
        assert gene_c[f] == zc.model(sc.ref_decode(gene_s[f]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [4, 12])
def test_stage_tools_with_compressed_files(tmp_path, seed):
    """muscato_screen and muscato_confirm read compressed inputs and write compressed bmatch_k / rmatch_k files whose
    lines are those of the stored run."""
    ocfg, reads, targets = make_case(seed)
    texts = {}
    for write in ("stored", "compressed"):
        enc = zc.model if write == "compressed" else (lambda t: sc.frame(t, False))
        root = tmp_path / write
        tmp, logd = root / "tmp", root / "logs"
        tmp.mkdir(parents=True)
        logd.mkdir()
        (root / "genes.txt.sz").write_bytes(enc(b"".join(t + b"\n" for t in targets)))
        (tmp / "reads_sorted.txt.sz").write_bytes(enc(b"".join(r + b"\t1\tn%d\n" % i for i, r in enumerate(reads))))
        cfg = {"ReadFileName": "x.fastq", "GeneFileName": str(root / "genes.txt.sz"), "GeneIdFileName": "unused",
               "ResultsFileName": "unused", "Windows": ocfg.Windows, "WindowWidth": ocfg.WindowWidth,
               "PMatch": ocfg.PMatch, "MinDinuc": ocfg.MinDinuc, "MaxReadLength": ocfg.MaxReadLength,
               "MaxMatches": ocfg.MaxMatches, "MatchMode": ocfg.MatchMode, "MMTol": ocfg.MMTol,
               "TempDir": str(tmp), "LogDir": str(logd), "BloomSize": 4000000, "NumHash": 20}
        (logd / "config.json").write_text(json.dumps(cfg))
        r = run([os.path.join(BIN, "muscato_screen"), str(logd / "config.json")], root, MUSC_SZ_WRITE=write)
        assert r.returncode == 0, r.stderr.decode()
        ww = ocfg.WindowWidth
        got = {}
        for k, q1 in enumerate(ocfg.Windows):
            raw = (tmp / ("bmatch_%d.txt.sz" % k)).read_bytes()
            bm = sc.ref_decode(raw)
            assert raw == enc(bm)
            got["bmatch_%d" % k] = bm
            lines = [l for l in bm.split(b"\n") if l]
            win = sorted(rd[q1:q1 + ww] + b"\t" + rd[:q1] + b"\t" + rd[q1 + ww:] for rd in reads if len(rd) >= q1 + ww)
            (tmp / ("win_%d_sorted.txt.sz" % k)).write_bytes(enc(b"".join(l + b"\n" for l in win)))
            (tmp / ("smatch_%d.txt.sz" % k)).write_bytes(enc(b"".join(l + b"\n" for l in sorted(lines))))
            r = run([os.path.join(BIN, "muscato_confirm"), str(logd / "config.json"), str(k)], root, MUSC_SZ_WRITE=write)
            assert r.returncode == 0, r.stderr.decode()
            raw = (tmp / ("rmatch_%d.txt.sz" % k)).read_bytes()
            got["rmatch_%d" % k] = sc.ref_decode(raw)
            assert raw == enc(got["rmatch_%d" % k])
        texts[write] = got
    # (the tools write a window's lines in no fixed order, as tests/test_stage_tools.py knows: the lines are compared sorted)
    lines = {w: {f: sorted(t.split(b"\n")) for f, t in got.items()} for w, got in texts.items()}
    assert lines["compressed"] == lines["stored"] and any(len(t) > SMALL for t in texts["stored"].values())
