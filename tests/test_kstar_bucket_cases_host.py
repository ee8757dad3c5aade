"""Host: the case matrix of tests/kstar_bucket_cases.py against the launch ladders of ppbo_amd/csrc/predict.hip, read as
text.  The ladders are named once (`using <Name> = DpLadder<...>;`), the limit of kstar_curv_kernel's acceleration twins is
a named constant, and every launch_kstar* function dispatches through a named ladder (`<Name>::dispatch(`) or, for
camphor-copper, launches a fixed DP (`std::integral_constant<int, DP>`).  This test reads those declarations and which
ladder each launcher uses, and holds the matrix to them, so that a new rung or a new launcher fails here until the matrix
(and with it tests/test_gpu_kstar_buckets.py) is extended."""
import collections
import os
import re

import kstar_bucket_cases as kc

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "ppbo_amd", "csrc", "predict.hip")
LADDER = re.compile(r"^using\s+(\w+)\s*=\s*DpLadder<([\d,\s]+)>;", re.M)
ACC_LIMIT = re.compile(r"^constexpr int KSTAR_CURV_ACC_MAX_DP = (\d+);", re.M)
LAUNCHER = re.compile(r"^(?:int|void)\s+(launch_kstar\w*)\s*\(", re.M)
DISPATCH = re.compile(r"\b(\w+)::dispatch\s*\(")
FIXED = re.compile(r"\bstd::integral_constant<int,\s*(\d+)>")


def ladders(text):
    """{launcher: {chain: sorted DP values}} of every launch_kstar* function in the source text: one chain per named ladder
    it dispatches through, "fixed" for the DP values it launches without a ladder, and "acc" for the rungs of
    launch_kstar_curv that have an acceleration twin."""
    named = {name: sorted(int(n) for n in rungs.split(",")) for name, rungs in LADDER.findall(text)}
    (acc_limit,) = ACC_LIMIT.findall(text)
    heads = list(LAUNCHER.finditer(text))
    out = {}
    for i, h in enumerate(heads):
        end = text.index("\n}\n", h.end())           # the function's closing brace, in column 0
        assert i + 1 == len(heads) or end < heads[i + 1].start()
        body = text[h.end():end]
        used = DISPATCH.findall(body)
        assert used, f"{h.group(1)}: no ladder dispatch found"
        per = {name: named[name] for name in used}   # (KeyError: a dispatch through a ladder that is not declared)
        fixed = sorted({int(n) for n in FIXED.findall(body)})
        if fixed:
            per["fixed"] = fixed
        if "KSTAR_CURV_ACC_MAX_DP" in body:
            per["acc"] = [n for name in used for n in named[name] if n <= int(acc_limit)]
        out[h.group(1)] = per
    return out


def missing(found, cases):
    """The (launcher, chain, rung, D) that no case of the matrix runs: every rung needs a case at D = rung and one at the
    rung's lower edge, in each ladder's own chain and in the launcher's chain of all its rungs.  (A fixed DP is no bucket
    of D: it has no edges of its own.)"""
    have = {c.D for c in cases}
    out = []
    for launcher, per in found.items():
        chains = {k: v for k, v in per.items() if k != "fixed"}
        chains["all"] = sorted(set().union(*per.values()))
        for name, chain in chains.items():
            for n in chain:
                out += [(launcher, name, n, D) for D in (n, kc.lower_edge(chain, n)) if D not in have]
    return out


def read_ladders():
    with open(SOURCE) as fh:
        return ladders(fh.read())


def test_the_launchers_are_the_ones_the_matrix_is_run_through():
    assert set(read_ladders()) == set(kc.LAUNCHERS)


def test_the_ladders_are_the_ones_the_matrix_was_built_for():
    """The union of every launcher's rungs is BUCKETS or a coarser subset of it (the camphor instances use 6 and 12 of
    them), and launch_kstar, _pair, _slope, _grad and _curv carry all eleven."""
    found = read_ladders()
    for launcher, per in found.items():
        rungs = set().union(*per.values())
        assert rungs <= set(kc.BUCKETS), (launcher, sorted(rungs - set(kc.BUCKETS)))
        if launcher != "launch_kstar_func":
            assert rungs == set(kc.BUCKETS), (launcher, sorted(set(kc.BUCKETS) - rungs))
            assert per["KstarLadder"] == list(kc.BUCKETS), launcher
    assert found["launch_kstar_func"] == {"KstarFuncLadder": [8, 20, 32, 48, 64]}
    assert found["launch_kstar"]["KstarFp32Ladder"] == [6, 20, 64]
    assert max(found["launch_kstar_curv"]["acc"]) == 16                 # the ACC twins: D <= 16


def test_every_rung_has_a_case_at_both_of_its_edges():
    assert missing(read_ladders(), kc.CASES) == []


def test_a_missing_case_or_an_added_rung_is_noticed():
    found = read_ladders()
    for drop in (9, 24, 49):                         # a lower edge, an upper edge, kstar_func_kernel's last lower edge
        assert missing(found, [c for c in kc.CASES if c.D != drop])
    more = {k: dict(v) for k, v in found.items()}
    more["launch_kstar_pair"]["KstarLadder"] = sorted(more["launch_kstar_pair"]["KstarLadder"] + [40])
    assert {(m[0], m[3]) for m in missing(more, kc.CASES)} == {("launch_kstar_pair", 40), ("launch_kstar_pair", 41)}
    # the same probe through the source text: a rung 40 in a ladder of the pair launcher's own
    with open(SOURCE) as fh:
        text = fh.read()
    head = LAUNCHER.search(text, text.index("void launch_kstar_pair(")).start()
    body_end = text.index("\n}\n", head)
    probe = (text[:head].replace("using KstarFuncLadder", "using ProbeLadder = DpLadder<4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64>;\n"
                                 "using KstarFuncLadder", 1)
             + text[head:body_end].replace("KstarLadder::dispatch", "ProbeLadder::dispatch") + text[body_end:])
    assert {(m[0], m[3]) for m in missing(ladders(probe), kc.CASES)} == {("launch_kstar_pair", 40), ("launch_kstar_pair", 41)}


def test_the_matrix_rule():
    nb, nk = len(kc.BUCKETS), len(kc.FAMILIES)
    assert len(kc.CASES) == nb * nk == 44
    assert collections.Counter((c.b, c.k) for c in kc.CASES) == {(b, k): 1 for b in range(nb) for k in range(nk)}
    assert len({kc.case_id(c) for c in kc.CASES}) == 44
    for c in kc.CASES:
        assert c.kernel == kc.FAMILIES[c.k]
        lo = 2 if c.b == 0 else kc.BUCKETS[c.b - 1] + 1
        assert (c.D, c.edge) == ((kc.BUCKETS[c.b], "upper") if (c.b + c.k) % 2 == 0 else (lo, "lower"))
        assert lo <= c.D <= kc.BUCKETS[c.b]
        assert c.form == ("node" if (c.b + c.k // 2) % 2 == 0 else "edge")
        assert (c.n_q, c.m) == ((8, 3) if c.b % 2 == 0 else (3, 25))
    for b in range(nb):
        # every bucket: both edges in both forms; every family once
        assert {(c.edge, c.form) for c in kc.CASES if c.b == b} == {(e, f) for e in ("upper", "lower") for f in ("node", "edge")}
        assert sorted(c.k for c in kc.CASES if c.b == b) == list(range(nk))
    # every family sees every bucket, at an edge that alternates from one bucket to the next
    for k in range(nk):
        mine = [c for c in kc.CASES if c.k == k]
        assert [c.b for c in mine] == list(range(nb))
        assert all(a.edge != b.edge for a, b in zip(mine, mine[1:]))
