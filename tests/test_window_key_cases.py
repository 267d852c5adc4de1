"""The inputs of the window-key tests (tests/window_key_cases.py), checked without a GPU: oracle/literal.cpp takes every
case without an error code, the two CPU oracles agree on it tuple for tuple, and every case still holds, in the
ORACLE's tuples, what it exists for -- tuples reported through each window, reads on both sides of each window's
MinDinuc gate, every sweep position with the verdict the sweep is about, blocks over the small MaxMatches, and a best +
MMTol selection that drops something.  These are conditions on the inputs: the seeds are pinned so that they hold."""
import numpy as np
import pytest

from oracle import muscato_oracle as orc

import stats_model as sm
import window_key_cases as wk


def by_read(name):
    out = {}
    for r, g, p, nx in wk.oracle_hits(name).tolist():
        out.setdefault(r, []).append((g, p, nx))
    return out


def test_shapes():
    widths = {s[0] for s in wk.SPECS.values()}
    assert widths == {16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 128, 4096}
    geom = {}
    for name, (ww, wins, L, pm, x) in wk.SPECS.items():
        geom.setdefault(name[0], []).append((ww, wins, L, x))
        assert max(wins) + ww <= L                       # MaxReadLength >= max(Windows) + ww
        assert min(wins) > 0 or ww <= 50, name           # the reference's panic domain: 100 - ww < ww with a window at 0
        assert int((1 - pm) * float(max(wins) + ww - 1)) >= 1  # every sweep read has a budget of at least one
    # 120-base context buckets: at most 120 bases of context, records of 8 words; every key class, and 33 and 64, in
    # every X variant
    for ww, wins, L, x in geom["n"]:
        assert max(wins) - min(wins) + L <= 120 and (-(-2 * L // 32) + 1 + 3) // 4 * 4 == 8
    for x in ("", "xr", "xd", "xw"):
        assert {16, 32, 33, 64} <= {g[0] for g in geom["n"] if g[3] == x}
    # wide buckets: 121 to 200 bases of context, reads of 150 bases (records of 12 words), up to four windows
    for ww, wins, L, x in geom["w"]:
        assert 120 < max(wins) - min(wins) + L <= 200 and L == 150
    assert {16, 32, 33, 64, 128} <= {g[0] for g in geom["w"]} and {len(g[1]) for g in geom["w"]} == {2, 3, 4}
    assert {16, 32, 65} <= {g[0] for g in geom["w"] if len(g[1]) == 3}  # three windows in every key class
    # the runtime stride: reads of 250 to 450 bases (records of 20 to 32 words: no instance of their own), beyond the
    # context path, one window far into the read
    for ww, wins, L, x in geom["r"]:
        assert 250 <= L <= 450 and max(wins) - min(wins) + L > 200 and (-(-2 * L // 32) + 1 + 3) // 4 * 4 > 16 and max(wins) >= 130
    assert {16, 32, 33, 64, 97, 128} <= {g[0] for g in geom["r"]} and {len(g[1]) for g in geom["r"]} == {2, 3}
    assert geom["k"] == [(4096, (1, 60), 4200, "")]
    assert set(wk.SEAMS) <= set(wk.places(4096)) and wk.places(128) == list(range(128)) and {0, 4095, 2048} <= set(wk.places(4096))


@pytest.mark.parametrize("name", wk.NAMES)
def test_the_oracles_agree(name):
    c = wk.case(name)
    assert c is wk.case(name)  # made once, shared
    lit = wk.oracle_hits(name)  # (literal.match_arrays raises on any error code of oracle/literal.cpp)
    direct = np.array(sorted(orc.match_direct(c.reads, c.targets, c.ocfg())), dtype=np.uint32).reshape(-1, 4)
    assert direct.shape == lit.shape and (direct == lit).all()
    assert not lit.flags.writeable and lit is wk.oracle_hits(name) and len(lit) > (50 if c.ww > 128 else 100)


@pytest.mark.parametrize("name", wk.NAMES)
def test_coverage(name):
    c = wk.case(name)
    cfg = c.ocfg()
    ww, wins, L = c.ww, c.windows, c.lmax
    hits = by_read(name)
    assert c.reads == sorted(set(c.reads)) and len(c.reads) % 64 == 37 and max(map(len, c.reads)) == L
    assert 10000 <= c.total_bases <= (130000 if ww > 128 else 80000), c.total_bases  # (a dinuc place of the widest costs 4 kb)
    lens = {len(r) for r in c.reads}
    assert {max(wins) + ww, max(wins) + ww - 1} <= lens and min(lens) < min(wins) + ww
    # tuples reported through each window; reads on both sides of each window's gate
    for k, q in enumerate(wins):
        valid = [orc.window_valid(r, k, cfg) for r in c.reads]
        through = sum(1 for ri, hs in hits.items() if valid[ri] for g, p, _ in hs
                      if c.targets[g][p + q:p + q + ww] == c.reads[ri][q:q + ww] and sm.fits(q, ww, len(c.reads[ri]), len(c.targets[g]), p + q))
        assert through >= 20, (k, through)
        assert sum(valid) >= 50 and sum(1 for r, v in zip(c.reads, valid) if not v and len(r) >= q + ww) >= 2, k
    # the random part places reads at position 0 and flush with a target's end
    assert any(p == 0 for hs in hits.values() for g, p, _ in hs if g < c.n_random_targets)
    assert any(p + len(c.reads[ri]) == len(c.targets[g]) for ri, hs in hits.items() for g, p, _ in hs if g < c.n_random_targets)
    # eq: the other window reports the tuple, once -- unless it covers the changed base as well
    if len(wins) == 2:
        seen = {(k, v): 0 for k in (0, 1) for v in (True, False)}
        for k, q in enumerate(wins):
            for p in wk.places(ww):
                ri = c.roles[("eq", k, p)]
                r = c.reads[ri]
                src = c.targets[c.eq_gene][wk.EQ_AT:wk.EQ_AT + L]
                assert len(r) == L and [i for i in range(L) if r[i] != src[i]] == [q + p]
                mine = [h for h in hits.get(ri, []) if h[0] == c.eq_gene and h[1] == wk.EQ_AT]
                other_covers = wins[1 - k] <= q + p < wins[1 - k] + ww
                assert mine == ([] if other_covers else [(c.eq_gene, wk.EQ_AT, 1)]), (k, p, mine)
                seen[k, other_covers] += 1
        assert seen[0, False] >= 2 and seen[1, False] >= 2  # (each window reports on the other's behalf)
    else:
        assert c.eq_gene is None
    # dinuc (and the planted X windows): window k alone can report the tuple, and the gate decides
    verdicts = set()
    for k in range(len(wins)):
        for p in wk.places(ww):
            assert ("dinuc", k, p) in c.planted
    for role, (g, pos, nsub, ok) in c.planted.items():
        ri = c.roles[role]
        r, k = c.reads[ri], role[1]
        assert c.targets[g][pos + wins[k]:pos + wins[k] + ww] == r[wins[k]:wins[k] + ww]
        assert orc.window_valid(r, k, cfg) == ok, role
        n = orc.count_dinuc(r[wins[k]:wins[k] + ww])
        if role[0] == "dinuc":
            assert n == (3 if 0 < role[2] < ww - 1 else 2) and ok == (n == 3)
        # (in the planted target: a poly-A window may also sit, with its one C, in a low-complexity target)
        assert [h for h in hits.get(ri, []) if h[0] == g] == ([(g, pos, nsub)] if ok else []), (role, hits.get(ri))
        verdicts.add((role[0], ok))
    assert {("dinuc", True), ("dinuc", False)} <= verdicts
    if ww > 32:
        assert all(("dinuc", k, p) in c.planted for k in range(len(wins)) for p in wk.SEAMS if p < ww)
    # the X variants
    xreads = [ri for ri, r in enumerate(c.reads) if X_IN(r)]
    db_x = any(X_IN(t) for t in c.targets)
    assert bool(xreads) == (c.x != "") and db_x == (c.x in ("xd", "xw"))
    inside = [ri for ri in xreads if any(c.reads[ri][i] == wk.X and c.in_window(i, len(c.reads[ri])) for i in range(len(c.reads[ri])))]
    assert all(c.reads[ri].count(b"X") <= 3 for ri in xreads)  # (every read lists its X in its xpos word, wide or not)
    if c.x == "xr":
        assert len(inside) >= 10 and len(xreads) - len(inside) >= 30
        assert sum(1 for ri in xreads if ri in hits) >= 20 and any(ri in hits for ri in inside)
    elif c.x == "xd":
        assert not inside and sum(1 for ri in xreads if ri in hits) >= 5
        assert not any(c.reads[ri][i] == wk.X and c.in_window(i, L) for ri in xreads for i in range(len(c.reads[ri])))
        assert any(nx == 0 for ri in xreads for _, _, nx in hits.get(ri, []))  # X == X matches
    elif c.x == "xw":
        # a tuple reported through a window that holds an X on both sides
        thr = [ri for ri in inside for g, p, _ in hits.get(ri, []) for q in wins
               if q + ww <= len(c.reads[ri]) and wk.X in c.reads[ri][q:q + ww] and c.targets[g][p + q:p + q + ww] == c.reads[ri][q:q + ww]]
        assert len(thr) >= 3
        assert ({("xchunk", True), ("xchunk", False)} <= verdicts) == (ww > 32)
    # best + MMTol is a strict subset of the union
    full = wk.oracle_hits(name)
    b0, b1 = wk.best_hits(name, 0), wk.best_hits(name, wk.MMTOL)
    assert len(b0) < len(b1) < len(full)
    # blocks over the small MaxMatches, none over 10^6
    hot = wk.hot(name)
    assert len(hot) >= 10 and {k for _, k in hot} == set(range(len(wins)))
    # the same blocks by this module's own count; in 256 buckets whole buckets overflow: more probes, not all of them
    probes, counts = wk.block_counts(name)
    assert {(ri, k) for ri, k in probes if counts[k].get(c.reads[ri][wins[k]:wins[k] + ww], 0) > wk.SMALL_MM} == hot
    if c.x == "":
        in8 = wk.bucket_hot(name, 8)
        assert hot <= in8 and len(hot) < len(in8) < len(probes)


def X_IN(s):
    return wk.X in s


def test_random_case_for_further_seeds():
    for x in ("xd", "xw"):
        c = wk.random_case(33, (3, 20), 100, 0.93, x, 5)
        assert not c.roles and not c.planted and c.eq_gene is None and len(c.targets) == c.n_random_targets
        assert len(c.reads) % 64 == 37 and c.windows == (3, 20) and c.seed == 5
        d = wk.random_case(33, (3, 20), 100, 0.93, x, 6)
        assert d.reads != c.reads
        a = sorted(orc.match_direct(c.reads, c.targets, c.ocfg()))
        assert [tuple(h) for h in wk.literal_hits(c).tolist()] == a and len(a) > 100


def test_the_gpu_runs_cover_every_path():
    """The run list of tests/test_gpu_window_keys.py: every key class, and 33 and 64, on every path; every launch
    descriptor a run names is one the library's resolvers can return; every case runs."""
    from muscato_amd.api import instances
    import test_gpu_window_keys as gk
    have = {tuple(sorted(d.items())) for d in instances()}
    by_path, kernels = {}, set()
    for name, path in gk.RUNS:
        c = wk.case(name)
        kind, want = gk.expected_launch(c, path)
        assert kind == {"fused": 1 + (name[0] == "w"), "dma": 1, "lines": 3}.get(path.split("-")[0], 0), (name, path)
        for d in want.values():
            assert tuple(sorted(d.items())) in have, (name, path, d)
            kernels.add(tuple(d.get(f) for f in ("kernel", "RW", "mask", "w2", "XM", "WIDE", "lines", "W")))
        cls = (path + (":" + c.x if c.x else "")) if name[0] == "n" else name[0] + ":" + path
        by_path.setdefault(cls, set()).add(c.ww)
    every = [p for p in gk.PATHS if p != "auto"] + ["%s:%s" % (p, x) for p in ("fused", "classic", "lines") for x in ("xr", "xd")]
    every += ["auto:xw", "lines:xw", "w:fused", "r:auto", "r:lines"]
    for cls in every:
        assert set(gk.ALL_PATHS_WIDTHS) <= by_path[cls], (cls, sorted(by_path[cls]))
    assert {97, 128} <= by_path["r:auto"] and {96, 97, 128} <= by_path["w:fused"] and by_path["k:auto"] == by_path["k:lines"] == {4096}
    assert by_path["fused"] == {16, 17, 31, 32, 33, 48, 63, 64} and {16, 32, 33, 64, 65} <= by_path["w:classic"] == by_path["w:lines"]
    # three and more windows (k_confirm's w2 = false) in every key class, on the classic and the line layout
    for paths in (("classic", "auto"), ("lines",)):  # (left to itself a two-kernel run takes the classic layout)
        assert set(gk.ALL_PATHS_WIDTHS) <= {wk.case(n).ww for n, p in gk.RUNS if p in paths and len(wk.case(n).windows) > 2}
    assert {wk.case(n).ww for n, p in gk.RUNS if p == "fused" and len(wk.case(n).windows) == 3} >= {16, 32, 65}
    assert set(wk.NAMES) == {name for name, _ in gk.RUNS} and len(gk.RUNS) == len(set(gk.RUNS))
    # k_match_t in every X mode on both bucket widths, with two, three and four windows; k_match_g; k_confirm with w2
    # both ways on a stride of its own and on the runtime one; k_screen with and without the mask plane on both layouts;
    # k_screen_t
    assert {k[0] for k in kernels} == {"k_match_t", "k_match_g", "k_screen", "k_screen_t", "k_confirm"}
    assert {(k[4], k[5]) for k in kernels if k[0] == "k_match_t"} == {(xm, wd) for xm in (0, 1, 2) for wd in (0, 1)}
    assert {k[7] for k in kernels if k[0] == "k_match_t"} == {2, 3, 4}
    assert {(k[1], k[3]) for k in kernels if k[0] == "k_confirm"} >= {(8, 1), (12, 0), (0, 1), (0, 0)}
    assert {(k[2], k[6]) for k in kernels if k[0] == "k_screen"} == {(m, ln) for m in (0, 1) for ln in (0, 1)}
    assert {k[1] for k in kernels if k[0] == "k_screen_t"} == {8, 12}
