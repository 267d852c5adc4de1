"""tests/sz_compress_cases.py held without a GPU: the model of the compressing writer decodes under the
strict decoder of tests/sz_cases.py and under the oracle's; the cases show, in their own parses, everything REQUIRED
lists; the model's bytes are the host writer's (`muscato_prep_targets` with MUSC_SZ_WRITE=compressed on the host path);
on the text corpora the rule's elements take no more bytes than those of the sequential compressor of sz_cases.py, and
the exact sizes are pinned.

The host writer is reached through the tool, whose sequence text cannot be any bytes: a text of ACGT lines goes in as
name<TAB>sequence lines and comes out as it is; every other case goes in as one FASTA record, whose sequence text is the
record's lines joined and a newline (the last record is not subx-ed) -- the model is held on that text."""
import os
import struct
import subprocess

import pytest

from muscato_amd import build as mbuild
from oracle import muscato_oracle as orc

import sz_cases as sc
import sz_compress_cases as zc

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "muscato_amd", "bin")
CASES = zc.cases()

# bytes of the elements of each corpus' one chunk under the rule (deterministic: DESIGN.md 27 quotes them); the
# sequential model's beside them
PINNED = {"dna-lines": (29967, 32944), "id-lines": (29892, 31146), "read-lines": (29691, 33269), "id-pair-lines": (25797, 29309)}


@pytest.fixture(scope="module")
def tools():
    mbuild.build()


def test_every_required_property_is_shown():
    assert len({c.name for c in CASES}) == len(CASES)
    shown = set()
    for c in CASES:
        got = zc.shows(c.plain)
        assert c.covers <= got, "%s claims %s" % (c.name, sorted(c.covers - got))
        shown |= c.covers
    assert shown == set(zc.REQUIRED) and len(zc.REQUIRED) == len(set(zc.REQUIRED))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_model_decodes(case):
    s = zc.model(case.plain)
    assert sc.ref_decode(s) == case.plain
    assert orc.snappy_framed_decode(s) == case.plain
    assert len(s) <= zc.bound(len(case.plain)) == len(sc.frame(case.plain, False))
    assert s[:10] == sc.STREAM_ID and (case.plain or s == sc.STREAM_ID)
    # chunk by chunk: a kept block is below n - n / 8, a stored chunk is the plain bytes
    pos = 10
    for k, P in enumerate(zc.parses(case.plain)):
        ln = int.from_bytes(s[pos + 1:pos + 4], "little")
        assert s[pos] == (1 if P.stored else 0) and ln == 4 + (P.n if P.stored else len(P.block))
        assert P.stored == (len(P.block) >= P.n - P.n // 8)
        assert all(4 <= m <= zc.MAX_MATCH and 1 <= off <= 65532 for _, off, m in P.copies)
        pos += 4 + ln
    assert pos == len(s)


def test_the_hash_and_the_colliding_keys():
    assert zc.hash4(0) == 0 and zc.hash4(1) == 0x1E35A7BD >> 18 and zc.hash4(0xFFFFFFFF) == ((-0x1E35A7BD) & 0xFFFFFFFF) >> 18
    a, b = zc.colliding_keys()
    assert a != b and zc.hash4(struct.unpack("<I", a)[0]) == zc.hash4(struct.unpack("<I", b)[0])


def test_both_sides_of_the_stored_threshold():
    rep = zc.threshold_rep()
    below, at = zc.Parse(zc.threshold_text(rep - 1)), zc.Parse(zc.threshold_text(rep))
    assert below.stored and not at.stored
    assert len(below.block) >= below.n - below.n // 8 and len(at.block) < at.n - at.n // 8
    assert zc.model(zc.threshold_text(rep - 1)) == sc.frame(zc.threshold_text(rep - 1), False)
    assert any(c.covers & {"threshold-stored"} for c in CASES) and any(c.covers & {"threshold-compressed"} for c in CASES)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_not_worse_than_the_sequential_model(name):
    """The condition the rule has to meet on text: its elements take no more bytes than those of sz_cases.compress on the
    same chunk.  (Without the near candidate it misses it on both id texts: 33 062 and 31 983 bytes.)"""
    data = zc.corpus(name)
    assert len(data) == zc.CHUNK
    ours = zc.parses(data)[0]
    greedy = sum(len(e[1]) for e in sc.compress(data))
    print("%s: %d bytes of elements, the sequential model %d" % (name, ours.element_bytes, greedy))
    assert ours.element_bytes <= greedy
    assert (ours.element_bytes, greedy) == PINNED[name]
    assert not ours.stored and len(zc.model(data)) == 10 + 8 + 3 + ours.element_bytes


# ---------------------------------------------------------------- the host writer

def tool_input(plain):
    """-> (file name, the tool's input, the sequence text it must make of it)"""
    if plain.endswith(b"\n") and set(plain) <= set(b"ACGT\n") and b"\n\n" not in plain and not plain.startswith(b"\n"):
        lines = plain.split(b"\n")[:-1]
        return "genes.txt", b"".join(b"n%d\t%s\n" % (i, l) for i, l in enumerate(lines)), plain
    lines = plain.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    assert all(l and not l.startswith(b">") for l in lines)
    seq = b"".join(lines)
    return "genes.fasta", b">c\n" + plain, (seq + b"\n" if seq else b"")


def host_writes(tmp_path, fname, data, mode):
    d = tmp_path / ("w_%s" % mode)
    d.mkdir(exist_ok=True)
    (d / fname).write_bytes(data)
    env = dict(os.environ, MUSC_PREP_TARGETS="host")
    env.pop("MUSC_SZ_WRITE", None)
    if mode is not None:
        env["MUSC_SZ_WRITE"] = mode
    r = subprocess.run([os.path.join(BIN, "muscato_prep_targets"), fname], cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    return (d / ("musc_" + fname + ".sz")).read_bytes(), (d / ("musc_ids_" + fname + ".sz")).read_bytes()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_host_writer_writes_the_model(tools, tmp_path, case):
    fname, data, text = tool_input(case.plain)
    seq_sz, id_sz = host_writes(tmp_path, fname, data, "compressed")
    assert seq_sz == zc.model(text)
    ids = sc.ref_decode(id_sz)
    assert id_sz == zc.model(ids) and (ids != b"") == (text != b"")


def test_the_host_writer_on_texts_that_pass_unchanged(tools, tmp_path):
    """ACGT lines: the tool's sequence text is the text itself, one to three chunks and a chunk's end inside a line."""
    text = zc.dna_lines(5, 3 * zc.CHUNK + 5000)
    for k, n in enumerate((3003, zc.CHUNK + 1001, 3 * zc.CHUNK + 5000)):
        plain = text[:text.rfind(b"\n", 0, n) + 1]
        fname, data, same = tool_input(plain)
        assert fname == "genes.txt" and same == plain
        (tmp_path / str(k)).mkdir()
        seq_sz, _ = host_writes(tmp_path / str(k), fname, data, "compressed")
        assert seq_sz == zc.model(plain) and len(seq_sz) < len(plain) // 2 + 100
        assert host_writes(tmp_path / str(k), fname, data, "stored")[0] == sc.frame(plain, False)
