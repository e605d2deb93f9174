"""CPU checks of tests/matmul_domain.py, the case lists of tests/test_paillier_matmul_domain_gpu.py:
the model's constants are the literal ones of the source, its window cut is a partition of |y|, the
lists reach every schedule class and sit exactly on every boundary (conditions, not measurements),
the oracle agrees with the naive product, and the oracle work of the GPU module stays small. Reads
source text and runs Python only."""
import json
import os
import random
import re

import pytest

import matmul_domain as md
from conftest import GOLDEN, PKG
from oracle import paillier as P

with open(os.path.join(GOLDEN, "paillier_kat.json")) as f:
    KEYS = {8 * k["n_bytes"]: k for k in json.load(f)["keys"]}
N2 = int(KEYS[512]["n"], 16) ** 2


def _src(name):
    with open(os.path.join(PKG, "csrc", name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def launches():
    """[(list, case, setting, Schedule)] of every radix-2^28 launch of the 512-bit key"""
    out = []
    for lst, case, settings in md.plan(N2) + [("WIDE", c, s) for c, s in md.wide_plan(N2)]:
        out += [(lst, case, s, md.schedule(case, s)) for s in settings]
    return out


@pytest.fixture(scope="module")
def groups(launches):
    return [(lst, case, g) for lst, case, _, sched in launches for g in sched.groups]


def test_model_constants_are_the_sources():
    """Every constant the model restates, as the literal text of its definition. A failure names
    the case list whose boundaries moved with it."""
    sl, pl = _src("paillier_sliced.hip"), _src("paillier.hip")
    for pattern, text, revisit in (
            (rf"#define EFL_MAT_WIN {md.MAT_WIN}\b", sl, "window_mask and the CAP list (windows per y)"),
            (rf"kEvBlock = 128, kEvHistLevels = {md.EV_HIST_LEVELS};", sl, "LEVELS (tops 127 / 128 / 129)"),
            (rf"kEvLevelShift = {md.EV_LEVEL_SHIFT}, kEvNegBit = {md.EV_NEG_BIT};", sl,
             "LEVELS (tops 1023 / 1024 / 1025)"),
            (r"kEvLevels = 1ll << \(32 - kEvLevelShift\);", sl, "LEVELS (tops 1023 / 1024 / 1025)"),
            (r"if \(ok && top <= kEvHistLevels\)", sl, "LEVELS (tops 127 / 128 / 129)"),
            (rf"bool ok = j1 - j0 <= {md.TERM_FIELD} && top <= kEvLevels;", sl, "WIDE and LEVELS"),
            (rf"terms \* {md.CAP_PER_TERM} < {md.CAP_MAX} \? terms \* {md.CAP_PER_TERM} : {md.CAP_MAX};", sl, "CAP"),
            (r"if \(cap \* NL > \(1ll << 28\)\) cap = \(1ll << 28\) / NL;", sl, "CAP (the slab clamp)"),
            (r"const long long NL = UW \* S, terms = \(v \+ S - 1\) / S;", sl, "CAP"),
            (rf"while \(2 \* S <= {md.AUTO_SPLITS_MAX} && 2 \* S <= v && UW \* G \* S < kOneRound\) S \*= 2;", sl,
             "the automatic S of every list"),
            (r"kOneRound = 256ll \* 4 \* 64 \* ", sl, "the automatic S of every list"),
            (r"while \(2 \* S <= fixed && 2 \* S <= v\) S \*= 2;", sl, "the fixed S of every list"),
            (r"const int j0 = \(int\)\(\(long long\)v \* sp / S\), "
             r"j1 = \(int\)\(\(long long\)v \* \(sp \+ 1\) / S\);", sl, "the uneven splits of GEO and WIDE"),
            (r"constexpr int kSlBlock = 64;", sl, "the wave-mixing condition (E = 64 / G)"),
            (rf"if \(limbs_per_lane > {md.FIXED_SPLITS_MAX}\) \{{ set_error\(\"matmul term splits", pl,
             "GEO (S = 16)")):
        assert re.search(pattern, text), f"{pattern!r} is no longer in the source: revisit {revisit}"
    assert md.EV_LEVELS == 1024 and md.EV_WORDS_MAX == 1 << 28 and md.ONE_ROUND_MIN == 65536


def test_window_model():
    """window_mask / windows over every y of VALUES and 10,000 seeded int64: the windows partition
    the set bits of |y|, each starts at a set bit, starts are at least 5 apart, every value is odd
    and below 32, and sum(value << start) is |y|."""
    rng = random.Random(5)
    ys = [y for c in md.values_cases(N2) for r in c.ym for y in r]
    assert -(1 << 63) in ys and (1 << 63) - 1 in ys and 0 in ys
    ys += [rng.randrange(-(1 << 63), 1 << 63) for _ in range(10000)]
    ys += [md._nwin(k) for k in range(1, 13)]
    for y in ys:
        ay, ws = abs(y), md.windows(y)
        assert md.window_mask(y) == sum(1 << s for s, _ in ws) < 1 << 64
        covered = 0
        for s, val in ws:
            assert (ay >> s) & 1 and val & 1 and val < 32, (y, s, val)
            span = ((1 << md.MAT_WIN) - 1) << s
            assert not covered & span, (y, s)
            covered |= span
        assert all(b - a >= md.MAT_WIN for (a, _), (b, _) in zip(ws, ws[1:])), y
        assert ay & ~covered == 0 and sum(val << s for s, val in ws) == ay, y
    assert [len(md.windows(md._nwin(k))) for k in (1, 2, 5, 6)] == [1, 2, 5, 6]


def test_every_class_is_reached(groups):
    reached = {g.cls for _, _, g in groups}
    assert reached == set(md.CLASSES)
    # and by the reduced lists of the larger keys, all but the two that need many terms
    reduced = {g.cls for _, case, ss in md.plan(N2, reduced=True) for s in ss for g in md.schedule(case, s).groups}
    assert reduced >= {"hist", "scan", "unlisted-levels", "unlisted-cap"}


def test_every_boundary_is_hit_exactly(groups, launches):
    by_top = {}
    for _, _, g in groups:
        by_top.setdefault(g.top, set()).add(g.cls)
    for top, cls in ((1, "hist"), (127, "hist"), (128, "hist"), (129, "scan"), (1023, "scan"), (1024, "scan"),
                     (1025, "unlisted-levels"), (1100, "unlisted-levels")):
        assert cls in by_top.get(top, ()), f"no {cls} group with top level {top}"
    for cap in (10, 20, 4096):
        for path, tops in (("the counting sort", range(1, 129)), ("the level scan", range(129, 1025))):
            at = [g for _, _, g in groups if g.cap == cap and g.events == cap and g.top in tops]
            past = [g for _, _, g in groups if g.cap == cap and g.events == cap + 1 and g.top in tops]
            assert at and all(g.cls in ("hist", "scan") for g in at), f"no list of exactly {cap} events through {path}"
            assert past and all(g.cls == "unlisted-cap" for g in past), f"no list of {cap} + 1 events through {path}"
    width = {}
    for _, case, g in groups:
        width.setdefault(g.j1 - g.j0, []).append((case, g))
    assert any(g.cls == "hist" and case.ym[g.j1 - 1][g.col] for case, g in width[65536]), "term index 65,535 unused"
    assert all(g.cls == "unlisted-wide" for _, g in width[65537])
    assert all(g.cls == "hist" for w in (32768, 32769) for _, g in width[w])
    # the slab clamp (2^28 / NL words per list) is out of reach: no launch comes near it
    assert all(s.cap * len(s.groups) < md.EV_WORDS_MAX // 1000 for *_, s in launches)


@pytest.mark.parametrize("lanes", [4, 2, 1])
def test_listed_and_unlisted_groups_share_a_wave(launches, lanes):
    """E = 16 / 32 / 64 outputs per 64-lane block (the 512-bit key's G = 4 / 2 / 1)."""
    mixed = [case.name for _, case, _, sched in launches for wv in md.waves(sched, lanes)
             if {g.cls for g in wv} & {"hist", "scan"} and any(g.cls.startswith("unlisted") for g in wv)]
    assert {"levels-six-tops-v4", "cap20-both", "cap4096", "values"} <= set(mixed)


def test_wide_term_splits_are_granted():
    """S = 8 and 16 are really taken (v >= 8, v >= 16), with the uneven splits of v = 9 and 17, and
    v = 1 stays at S = 1 whatever is asked."""
    by_shape = {md.shape(c): c for c in md.geo_cases(N2)}
    assert set(by_shape) == set(md.GEO_SHAPES)
    for v, setting, want, widths in ((9, 8, 8, {1, 2}), (9, 0, 8, {1, 2}), (9, 16, 8, {1, 2}), (17, 16, 16, {1, 2}),
                                     (17, 0, 8, {2, 3}), (33, 16, 16, {2, 3}), (16, 16, 16, {1}), (8, 8, 8, {1}),
                                     (1, 16, 1, {1}), (3, 4, 2, {1, 2}), (2, 16, 2, {1})):
        case = next(c for s, c in by_shape.items() if s[1] == v)
        sched = md.schedule(case, setting)
        assert sched.S == want and {g.j1 - g.j0 for g in sched.groups} == widths, (v, setting)
    for u, v, w in md.GEO_SHAPES:   # below, at and past one block, and u that does not divide E
        assert u * w * md.MAX_LANES * md.AUTO_SPLITS_MAX < md.ONE_ROUND_MIN
    assert {u * w for u, _, w in md.GEO_SHAPES} >= {1, 5, 65, 66, 68, 128}


def _naive(n2, case):
    u, v, w = md.shape(case)
    zm = [[1] * w for _ in range(u)]
    ze = [[0] * w for _ in range(u)]
    for i in range(u):
        for k in range(w):
            ze[i][k] = min(case.xe[i][j] + case.ye[j][k] for j in range(v))
            for j in range(v):
                y, x = case.ym[j][k], case.xm[i][j]
                if y < 0:
                    x, y = pow(x, -1, n2), -y
                zm[i][k] = zm[i][k] * pow(x, y << (case.xe[i][j] + case.ye[j][k] - ze[i][k]), n2) % n2
    return zm, ze


def test_oracle_is_the_naive_product():
    """oracle.paillier.matmul on three small cases (signs, zeros, -2^63, a y = 0 term holding the
    minimum exponent) equals prod pow(x, y << d, n^2), the inverse taken for y < 0."""
    k = KEYS[512]
    okp = P.Keypair(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, 1)
    zero_min = next(c for c in md.levels_cases(N2) if c.name.startswith("levels-zero-min"))
    for case in (md.geo_case(N2, 7, 9, 5), md.values_cases(N2)[0], zero_min):
        assert P.matmul(okp, case.xm, case.xe, case.ym, case.ye) == _naive(N2, case), case.name


def test_first_difference_reports_what_the_gpu_test_compares():
    """The comparison the GPU module asserts on: silent on the oracle's own result (flattened row by
    row, as the GPU returns it), and naming the output and the classes of its splits when one
    mantissa or one exponent is off by one."""
    k = KEYS[512]
    okp = P.Keypair(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, 1)
    case = md.levels_six_tops(N2)
    want_m, want_e = P.matmul(okp, case.xm, case.xe, case.ym, case.ye)
    flat_m, flat_e = [c for r in want_m for c in r], [e for r in want_e for e in r]
    assert md.first_difference(case, 0, flat_m, flat_e, want_m, want_e) is None
    for setting, o, classes in ((1, 5, "unlisted-levels top 1025"), (2, 3, "scan top 1023"), (4, 1, "hist top 128")):
        bad = list(flat_m)
        bad[o] ^= 1
        msg = md.first_difference(case, setting, bad, flat_e, want_m, want_e)
        assert f"mantissa of output ({o // 3}, {o % 3})" in msg and classes in msg and f"S = {setting}" in msg, msg
        bad = list(flat_e)
        bad[o] += 1
        msg = md.first_difference(case, setting, flat_m, bad, want_m, want_e)
        assert f"exponent of output ({o // 3}, {o % 3})" in msg, msg


def test_oracle_budget(launches):
    """The memoised oracle work of the whole GPU module, from the measured per-term costs: under
    20 s at the 512-bit key, under 15 s for the reduced lists of the 1024- and 4096-bit keys."""
    full = {case.name: md.oracle_seconds(case, 512) for _, case, _, _ in launches}
    assert sum(full.values()) < 20, sorted(full.items(), key=lambda kv: -kv[1])[:5]
    assert max(full.values()) < 3
    larger = 0.0
    for bits in (1024, 4096):
        n2 = int(KEYS[bits]["n"], 16) ** 2
        reduced = {case.name: md.oracle_seconds(case, bits) for _, case, _ in md.plan(n2, reduced=True)}
        assert max(reduced.values()) < 4, reduced
        larger += sum(reduced.values())
    assert larger < 15
