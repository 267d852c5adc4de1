"""The read-name cases and their model, without a GPU: the model in its parallel form against the string
code of tests/fastq_cases.py, against the oracle's prep_reads + uniqify and against the reference's own fixtures, and
what each case covers -- every case names the branches it is there for and the model's counters show they were taken."""
import os

import pytest

from oracle import muscato_oracle as orc

import fastq_cases as fc
import read_names_cases as rn

CASES = {c.name: c for c in rn.cases()}


def test_case_names_are_unique():
    assert len(CASES) == len(rn.cases())


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_string_code(name):
    """count, names and order of every group as fastq_cases.unique / join_names give them; both texts follow."""
    c = CASES[name]
    m = rn.model_of(c)
    exp = fc.unique(m.prep)
    assert [(s, k) for s, k in zip(m.seqs, m.counts)] == [(s, k) for s, k, _ in exp]
    assert m.records == [b"%d\t%s" % (k, na) for _, k, na in exp]
    assert m.lines == [s + b"\t%d\t" % k + na + b"\n" for s, k, na in exp]
    assert m.info["n_text_bytes"] == len(m.text) and m.info["n_line_bytes"] == len(m.line_text)
    assert m.info["n_single"] + m.info["n_wave_groups"] + m.info["n_sorted_groups"] == m.info["n_unique"] == len(exp)
    for g, ranked in enumerate(m.members):  # a permutation of the group, equal clipped names in file order
        names = [fc.short_name(m.prep.names[r]) for r in ranked]
        assert names == sorted(names) and len(ranked) == m.counts[g]
        assert all(a < b for a, b, x, y in zip(ranked, ranked[1:], names, names[1:]) if x == y)


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_oracle(name):
    """oracle.read_fastq -> prep_reads -> sort -> uniqify, on every case without a carriage return (the oracle keeps them)."""
    c = CASES[name]
    if b"\r" in c.raw:
        assert name in ("fq_crlf", "fq_lone_cr")
        return
    cfg = orc.Config(Windows=[0], WindowWidth=4, MinReadLength=c.min_len, MaxReadLength=c.max_len)
    exp = orc.uniqify(sorted(orc.prep_reads(orc.read_fastq(c.raw), cfg)))
    m = rn.model_of(c)
    assert m.lines == [u.seq + b"\t%d\t" % u.count + u.names + b"\n" for u in exp]


def test_model_on_the_reference_fixtures(golden_dir):
    """The reads of the reference's end-to-end fixtures; at least one of them holds a read twice."""
    dups = 0
    for case in sorted(os.listdir(os.path.join(golden_dir, "muscato"))):
        with open(os.path.join(golden_dir, "muscato", case, "reads.fastq"), "rb") as f:
            raw = f.read()
        m = rn.model(raw, 1, 1000)
        cfg = orc.Config(Windows=[0], WindowWidth=4, MinReadLength=1, MaxReadLength=1000)
        exp = orc.uniqify(sorted(orc.prep_reads(orc.read_fastq(raw), cfg)))
        assert m.lines == [u.seq + b"\t%d\t" % u.count + u.names + b"\n" for u in exp] and m.lines
        dups += any(k > 1 for k in m.counts)
    assert dups >= 1


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.covers))
def test_each_case_covers_what_it_is_there_for(name):
    c = CASES[name]
    missing = [b for b in c.covers if b not in rn.model_of(c).cover]
    assert not missing, missing


def test_the_cases_cover_the_issue_list():
    seen = set()
    for c in rn.cases():
        seen |= rn.model_of(c).cover
    want = ["len:%d" % n for n in (0, 1, 7, 8, 9, 994, 995, 996, 997, 998, 999, 1000, 1001, 1100)]
    want += ["diff:%d" % d for d in list(range(17)) + [993, 994]] + ["tie_beyond:%d" % d for d in (995, 996, 997)]
    want += ["phase:%d:%d" % (d, a) for d in range(17) for a in range(8)] + ["align:%d" % a for a in range(16)]
    want += ["prefix", "prefix_in_word", "equal", "equal_clipped", "reordered"]
    want += ["bytes:00:7f", "bytes:7f:80", "bytes:80:ff", "bytes:00:ff"]
    want += ["tab_first", "tab_last", "tab_mid", "tabs:0", "tabs:1", "tabs:2", "long_tab:994:kept", "long_tab:995:cut_away", "empty_token_inside"]
    want += ["group:%d" % k for k in (1, 2, 3, 63, 64, 65, 256, 257, 5000, 9, 10, 99, 100, 999, 1000)]
    want += ["digits:%d" % d for d in (1, 2, 3, 4)] + ["path:single", "path:wave", "path:sorted"]
    want += ["join:%d" % n for n in (999, 1000, 1001, 1002)] + ["cut:mid", "cut:on_sep", "cut:after_sep", "overflow:wave", "overflow:sorted", "first_998"]
    assert not [w for w in want if w not in seen]


def test_whole_texts_are_the_fastq_cases():
    assert {c.name for c in rn.cases() if c.name.startswith("fq_")} == {"fq_" + c.name for c in fc.cases()}
    m = rn.model_of(CASES["fq_big"])
    assert m.prep.n_reads == 40000 and 5900 < m.info["n_unique"] <= 6000 and m.info["n_wave_groups"] > 5000
    m = rn.model_of(CASES["fq_dup_names"])
    assert sorted(m.records) == [b"1\t@alpha", b"6\t@Zed;@a;@b;@b;@b!;@zeta"]  # (the two sequences are random: either order)


def test_constants_are_the_plan_headers():
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "muscato_amd", "csrc", "read_names_plan.hpp")).read()

    def const(n):
        return int(re.search(r"\b%s = (\d+)" % n, src).group(1))
    assert (const("NAME_LIMIT"), const("NAME_KEEP"), const("JOIN_LIMIT"), const("JOIN_KEEP"), const("DOTS"), const("WAVE_GROUP_MAX")) == \
        (rn.NAME_LIMIT, rn.NAME_KEEP, rn.JOIN_LIMIT, rn.JOIN_KEEP, rn.DOTS, rn.WAVE_GROUP_MAX)
