"""The launch domain of efl_pl_matmul, for tests (a plain helper, no fixtures).

Which code a PaillierMatmul runs is decided by hard constants in run_matmul28 and k_mmevents
(csrc/paillier_sliced.hip): the term splits S, the event-list capacity, the three schedule builders
per (output, split) and the 16-bit term field. Every one of them guards an index into LDS or into
the event slab. This module restates those DECISIONS in Python (no ciphertext arithmetic) and builds
the case lists that put a launch exactly on every boundary:

* the schedule model: window_mask(), splits_granted(), capacity() and schedule(), which gives every
  (output, split) its mn, j0, j1, top level, event count and class
  ("hist" / "scan" / "unlisted-levels" / "unlisted-cap" / "unlisted-wide" / "empty");
* the case builders geo_cases(), levels_cases(), cap_cases(), values_cases() and wide_case(): each
  case is (name, xm, xe, ym, ye), xm seeded random integers below n^2 (no encryption is needed: the
  kernels take any residue), and plan() / wide_plan() pair each case with the term-split settings
  it runs at;
* oracle_seconds(): what the Python-int oracle costs for a case, from measured per-term costs.

The model only CLASSIFIES: tests/test_matmul_domain_host.py ties its constants to the source text
and checks that the lists reach every class and boundary; results on the GPU are judged by
oracle.paillier.matmul alone (tests/test_paillier_matmul_domain_gpu.py).
"""
from __future__ import annotations

import random
import zlib
from typing import NamedTuple

# csrc/paillier_sliced.hip (test_matmul_domain_host.py asserts the literal definitions)
MAT_WIN = 5                      # EFL_MAT_WIN: bits of a window of |y|
EV_HIST_LEVELS = 128             # kEvHistLevels: top levels the LDS counting sort takes
EV_LEVEL_SHIFT = 22              # kEvLevelShift: the level sits in bits [22, 32) of an event word
EV_NEG_BIT = 21                  # kEvNegBit
EV_LEVELS = 1 << (32 - EV_LEVEL_SHIFT)   # kEvLevels = 1024: top levels a list can hold
TERM_FIELD = 65536               # the term index j - j0 sits in 16 bits
CAP_PER_TERM = 5                 # cap = min(CAP_PER_TERM * ceil(v / S), CAP_MAX) ...
CAP_MAX = 4096
EV_WORDS_MAX = 1 << 28           # ... clamped again to EV_WORDS_MAX / NL (out of reach of any test)
AUTO_SPLITS_MAX = 8              # run_matmul28: while (2 * S <= 8 && ...)
FIXED_SPLITS_MAX = 16            # efl_pl_tune(ln, 3, S) refuses S > 16
ONE_ROUND_MIN = 256 * 4 * 64     # kOneRound at one wave per SIMD, its smallest build value
MAX_LANES = 32                   # G of the widest instantiation

CLASSES = ("hist", "scan", "unlisted-levels", "unlisted-cap", "unlisted-wide", "empty")

BOUNDARY_TOPS = (1, 127, 128, 129, 1023, 1024, 1025, 1100)


class Case(NamedTuple):
    name: str
    xm: list        # [u][v] ints below n^2
    xe: list        # [u][v]
    ym: list        # [v][w] int64 values
    ye: list        # [v][w]


class Group(NamedTuple):
    """One (output, split) of a launch: list l of k_mmevents, group i of k_matmul28."""
    l: int
    row: int
    col: int
    sp: int
    mn: int
    j0: int
    j1: int
    top: int
    events: int
    cap: int
    cls: str


class Schedule(NamedTuple):
    S: int
    cap: int
    groups: list    # of Group, in launch order (l ascending)


def shape(case):
    return len(case.xm), len(case.ym), len(case.ym[0])


# ---- the schedule model ---------------------------------------------------------------------

def window_mask(y: int) -> int:
    """k_wmask: bit s set = a window of up to MAT_WIN bits of |y| begins at bit s (right to left,
    each at a set bit)."""
    ay, mask, s = abs(y), 0, 0
    while ay >> s:
        if (ay >> s) & 1:
            mask |= 1 << s
            s += MAT_WIN
        else:
            s += 1
    return mask


def windows(y: int):
    """[(start, value)] of |y|'s windows; value = the MAT_WIN bits from start (odd)."""
    ay, m = abs(y), window_mask(y)
    return [(s, (ay >> s) & ((1 << MAT_WIN) - 1)) for s in range(m.bit_length()) if (m >> s) & 1]


def splits_granted(v: int, setting: int, uw: int = 1) -> int:
    """The S run_matmul28 takes: a fixed setting rounded down to a power of two, at most v; or
    (setting 0) the largest power of two <= min(8, v) while UW * G * S stays under one round of
    waves, which holds for every shape of these lists at every G (asserted)."""
    S = 1
    if setting > 0:
        while 2 * S <= setting and 2 * S <= v:
            S *= 2
        return S
    assert uw * MAX_LANES * AUTO_SPLITS_MAX < ONE_ROUND_MIN, "the automatic split would depend on G"
    while 2 * S <= AUTO_SPLITS_MAX and 2 * S <= v:
        S *= 2
    return S


def capacity(v: int, S: int, nl: int) -> int:
    """Event words per list: five per term of the widest split, 4096 at most, and the slab of all
    NL lists at most 2^28 words."""
    terms = (v + S - 1) // S
    cap = min(terms * CAP_PER_TERM, CAP_MAX)
    if cap * nl > EV_WORDS_MAX:
        cap = EV_WORDS_MAX // nl
    return cap


def classify(width: int, top: int, events: int, cap: int, any_term: bool) -> str:
    if not any_term:
        return "empty"
    if width > TERM_FIELD:
        return "unlisted-wide"
    if top > EV_LEVELS:
        return "unlisted-levels"
    if events > cap:
        return "unlisted-cap"
    return "hist" if top <= EV_HIST_LEVELS else "scan"


def schedule(case, setting: int) -> Schedule:
    """What k_mmevents decides for every (output, split) of the case at a term-split setting."""
    u, v, w = shape(case)
    uw = u * w
    S = splits_granted(v, setting, uw)
    nl = uw * S
    cap = capacity(v, S, nl)
    nwin = [[bin(window_mask(y)).count("1") for y in r] for r in case.ym]
    blen = [[abs(y).bit_length() for y in r] for r in case.ym]
    groups = []
    for sp in range(S):
        j0, j1 = v * sp // S, v * (sp + 1) // S
        for col in range(w):
            for row in range(u):
                xr = case.xe[row]
                mn = min(xr[j] + case.ye[j][col] for j in range(v))
                top = events = 0
                any_term = False
                for j in range(j0, j1):
                    if case.ym[j][col] == 0:
                        continue
                    any_term = True
                    top = max(top, xr[j] + case.ye[j][col] - mn + blen[j][col])
                    events += nwin[j][col]
                groups.append(Group(sp * uw + col * u + row, row, col, sp, mn, j0, j1, top, events, cap,
                                    classify(j1 - j0, top, events, cap, any_term)))
    return Schedule(S, cap, groups)


def waves(sched: Schedule, lanes: int):
    """The groups of each 64-lane block of k_matmul28 when a number takes `lanes` lanes."""
    E = 64 // lanes
    return [sched.groups[i:i + E] for i in range(0, len(sched.groups), E)]


# ---- case builders --------------------------------------------------------------------------

def _rng(name):
    return random.Random(zlib.crc32(name.encode()))


def _xm(name, n2, u, v):
    rng = random.Random(zlib.crc32(("x:" + name).encode()))
    return [[rng.randrange(2, n2) for _ in range(v)] for _ in range(u)]


def _mant(rng, bits):
    """a signed mantissa of exactly `bits` bits"""
    a = rng.randrange(1 << (bits - 1), 1 << bits)
    return -a if rng.random() < 0.5 else a


GEO_SHAPES = ((1, 1, 1), (1, 1, 5), (5, 1, 1), (64, 1, 2), (1, 16, 1), (65, 2, 1), (1, 2, 65),
              (17, 3, 4), (33, 8, 2), (7, 9, 5), (3, 17, 3), (2, 33, 2))
GEO_REDUCED = ((17, 3, 4), (7, 9, 5))
GEO_SPLITS = (0, 1, 2, 4, 8, 16)


def geo_case(n2, u, v, w):
    """11-bit signed y, about one in seven zero (never all: a shape keeps a non-zero term), the
    exponent spread under 20: every list is a short "hist" one; the shape is the subject."""
    name = f"geo-{u}x{v}x{w}"
    rng = _rng(name)
    xe = [[rng.randrange(-30, -20) for _ in range(v)] for _ in range(u)]
    ye = [[rng.randrange(-25, -15) for _ in range(w)] for _ in range(v)]
    ym = [[0 if rng.random() < 1 / 7 else _mant(rng, rng.choice((9, 10, 11))) for _ in range(w)] for _ in range(v)]
    if v > 1:
        ym[0][0] = 0
    ym[v - 1][w - 1] = _mant(rng, 11)
    return Case(name, _xm(name, n2, u, v), xe, ym, ye)


def geo_cases(n2, shapes=GEO_SHAPES):
    return [geo_case(n2, *s) for s in shapes]


def _levels(name, n2, v, row_off, col_tops, far, near_bits=11):
    """Shape (2, v, 3). Term `far` of every output is y = +-1 at exponent row_off[row] +
    col_tops[col] - 1 above the other terms' (which share exponent 0 and hold 11-bit y, so levels up
    to 11): output (row, col) has top level exactly row_off[row] + col_tops[col]. Every y = +-1 when
    the top is 1."""
    rng = _rng(name)
    u, w = 2, 3
    xe = [[row_off[r] if j == far else 0 for j in range(v)] for r in range(u)]
    ye = [[col_tops[c] - 1 if j == far else 0 for c in range(w)] for j in range(v)]
    ym = [[rng.choice((-1, 1)) if j == far or near_bits == 1 else _mant(rng, near_bits) for c in range(w)]
          for j in range(v)]
    return Case(name, _xm(name, n2, u, v), xe, ym, ye)


def levels_six_tops(n2, v=4):
    """One launch, six outputs in one wave: tops 127, 128, 129 (row 0) and 1023, 1024, 1025 (row 1)."""
    return _levels(f"levels-six-tops-v{v}", n2, v, (0, 896), (127, 128, 129), far=v - 1)


def levels_cases(n2, v=4):
    """Top levels exactly on and around kEvHistLevels and kEvLevels (see _levels), the minimum
    exponent at a y = 0 term, and every exponent moved by +-2^40."""
    out = [levels_six_tops(n2, v)]
    for t in BOUNDARY_TOPS:
        out.append(_levels(f"levels-all-{t}-v{v}", n2, v, (0, 0), (t, t, t), far=1 % v, near_bits=1 if t == 1 else 11))
    base = _levels(f"levels-zero-min-v{v}", n2, v, (0, 1), (77, 78, 79), far=v - 1)
    # term 0 is y = 0 everywhere and 50 below every other exponent: the outputs' exponent is its,
    # and every real term starts 50 levels higher (tops 127, 128, 129 / 128, 129, 130)
    out.append(base._replace(ym=[[0] * 3 if j == 0 else r for j, r in enumerate(base.ym)],
                             xe=[[e - 50 if j == 0 else e for j, e in enumerate(r)] for r in base.xe]))
    for sign, tag in ((1, "plus"), (-1, "minus")):
        six = levels_six_tops(n2, v)
        off = sign << 40
        out.append(six._replace(name=f"levels-offset-{tag}-v{v}", xe=[[e + off for e in r] for r in six.xe],
                                ye=[[e + off for e in r] for r in six.ye]))
    return out


LEVELS_SPLITS = (0, 1, 2, 4)


def _nwin(k):
    """|y| with exactly k windows, each of value 1"""
    return sum(1 << (MAT_WIN * i) for i in range(k))


def _cap_case(name, n2, u, cols, far_top=0):
    """cols[c] = the window counts of column c's terms (signs alternate). Exponents spread under 20
    ("hist"); far_top > 0 lifts term 0 so the top level is about far_top ("scan")."""
    rng = _rng(name)
    v, w = len(cols[0]), len(cols)
    xe = [[rng.randrange(-8, 0) for _ in range(v)] for _ in range(u)]
    ye = [[rng.randrange(-8, 0) for _ in range(w)] for _ in range(v)]
    if far_top:
        for r in xe:
            r[0] += far_top
    ym = [[(-1 if (j + c) % 3 == 1 else 1) * _nwin(cols[c][j]) for c in range(w)] for j in range(v)]
    return Case(name, _xm(name, n2, u, v), xe, ym, ye)


def cap_cases(n2, big=True):
    """[(case, S setting)]: event counts exactly cap and cap + 1 for cap = 20 (v = 4, S = 1), 10
    (v = 4, S = 2: one split at cap, its neighbour past it, and the reverse) and 4096 (v = 820,
    S = 1), through the counting sort and through the level-major scan."""
    at, past = [5, 5, 5, 5], [5, 5, 5, 6]
    out = [(_cap_case("cap20-at", n2, 3, [at, at]), 1),
           (_cap_case("cap20-past", n2, 3, [past, past]), 1),
           (_cap_case("cap20-both", n2, 3, [at, past]), 1),
           (_cap_case("cap20-both-scan", n2, 3, [at, past], far_top=200), 1),
           (_cap_case("cap10-splits", n2, 3, [[5, 5, 5, 6], [6, 5, 5, 5]]), 2),
           (_cap_case("cap10-splits-scan", n2, 3, [[5, 5, 5, 6], [6, 5, 5, 5]], far_top=200), 2)]
    if big:
        full, over = [5] * 819 + [1], [5] * 819 + [2]
        out += [(_cap_case("cap4096", n2, 1, [full, over]), 1),
                (_cap_case("cap4096-scan", n2, 1, [full, over], far_top=200), 1)]
    return out


VALUES_SPLITS = (0, 1, 2, 4)
I63 = (1 << 63) - 1


def values_cases(n2):
    """Shape (3, 6, 8): one column per kind of y. 0 all zero; 1 all negative; 2 all positive; 3 one
    non-zero term; 4 the int64 extremes and the alternating patterns; 5 +-1, +-2, 31, 32; 6 dense
    63-bit values; 7 33, 0, and 11- and 24-bit mantissas of both signs. The second case holds the
    magnitudes only (2^63 - 1 for -2^63): no negative anywhere."""
    name = "values"
    rng = _rng(name)
    u, v, w = 3, 6, 8
    cols = [[0] * v,
            [-abs(_mant(rng, b)) for b in (11, 24, 11, 5, 24, 11)],
            [abs(_mant(rng, b)) for b in (11, 24, 11, 5, 24, 11)],
            [0, 0, 0, 0, _mant(rng, 24), 0],
            [1 << 62, I63, -I63, -(1 << 63), 0x5555555555555555, 0x2AAAAAAAAAAAAAAA],
            [1, -1, 2, -2, 31, 32],
            [(1 if j % 2 else -1) * (rng.getrandbits(63) | (1 << 62)) for j in range(v)],
            [33, 0, abs(_mant(rng, 11)), -abs(_mant(rng, 11)), abs(_mant(rng, 24)), -abs(_mant(rng, 24))]]
    ym = [[cols[c][j] for c in range(w)] for j in range(v)]
    xe = [[rng.randrange(-30, -20) for _ in range(v)] for _ in range(u)]
    ye = [[rng.randrange(-25, -15) for _ in range(w)] for _ in range(v)]
    mixed = Case(name, _xm(name, n2, u, v), xe, ym, ye)
    nonneg = mixed._replace(name="values-nonneg", ym=[[min(abs(y), I63) for y in r] for r in ym])
    return [mixed, nonneg]


def wide_case(n2, v):
    """(u, w) = (1, 2): y non-zero only at the ends and around the middle of the term range, every
    term with an exponent of its own (the minimum runs over all v)."""
    name = f"wide-{v}"
    rng = _rng(name)
    ye = [[rng.randrange(-12, 0), rng.randrange(-12, 0)] for _ in range(v)]
    xe = [[rng.randrange(-8, 0) for _ in range(v)]]
    ym = [[0, 0] for _ in range(v)]
    for j in (0, 1, 32767, 32768, 32769, v - 2, v - 1):
        ym[j] = [_mant(rng, 11), _mant(rng, 11)]
    return Case(name, _xm(name, n2, 1, v), xe, ym, ye)


def wide_plan(n2):
    """[(case, S settings)]: term index 65,535 in a list; a split one term too wide for the 16-bit
    field; the same terms as two splits of 32,768 and 32,769."""
    return [(wide_case(n2, TERM_FIELD), (1,)), (wide_case(n2, TERM_FIELD + 1), (1, 2))]


def plan(n2, reduced=False):
    """[(list name, case, S settings)] of the radix-2^28 runs: the whole lists for the 512-bit key,
    or the reduced ones of the larger keys (two GEO shapes at S = 0 and 8, the six-tops LEVELS launch
    cut to two terms per output, the v = 4 CAP cases)."""
    if reduced:
        return ([("GEO", c, (0, 8)) for c in geo_cases(n2, GEO_REDUCED)] +
                [("LEVELS", levels_six_tops(n2, v=2), (0, 1))] +
                [("CAP", c, (s,)) for c, s in cap_cases(n2, big=False)])
    return ([("GEO", c, GEO_SPLITS) for c in geo_cases(n2)] +
            [("LEVELS", c, LEVELS_SPLITS) for c in levels_cases(n2)] +
            [("CAP", c, (s,)) for c, s in cap_cases(n2)] +
            [("VALUES", c, VALUES_SPLITS) for c in values_cases(n2)])


# ---- the oracle's cost ----------------------------------------------------------------------

# seconds of oracle.paillier.matmul per term, measured with CPython ints on the known-answer keys:
# (a 63-bit scalar power, one squaring of the 2^d shift, one inverse for y < 0); a shorter scalar
# costs in proportion to its bits, and every term pays one more product for the accumulation.
ORACLE_COST = {512: (0.36e-3, 10.6e-3 / 3000, 0.2e-3), 1024: (1.1e-3, 33e-3 / 3000, 0.35e-3),
               4096: (13e-3, 425e-3 / 3000, 6.5e-3)}
ZERO_TERM_COST = 2e-6      # pow(x, 0), pow(1, 2^d): no big-number work


def oracle_seconds(case, key_bits: int) -> float:
    """Estimated cost of oracle.paillier.matmul on the case."""
    c63, csq, cinv = ORACLE_COST[key_bits]
    u, v, w = shape(case)
    total = 0.0
    for col in range(w):
        for row in range(u):
            ex = [case.xe[row][j] + case.ye[j][col] for j in range(v)]
            mn = min(ex)
            for j in range(v):
                y = case.ym[j][col]
                if y == 0:
                    total += ZERO_TERM_COST
                else:
                    total += c63 * abs(y).bit_length() / 63 + csq * (ex[j] - mn + 2) + (cinv if y < 0 else 0.0)
    return total


def first_difference(case, setting, got_m, got_e, want_m, want_e):
    """None, or a line naming the first output that differs and the classes of its splits."""
    u, v, w = shape(case)
    sched = None
    for o in range(u * w):
        row, col = divmod(o, w)
        bad_e, bad_m = got_e[o] != want_e[row][col], got_m[o] != want_m[row][col]
        if bad_e or bad_m:
            sched = sched or schedule(case, setting)
            gs = [g for g in sched.groups if g.row == row and g.col == col]
            what = "exponent" if bad_e else "mantissa"
            return (f"{case.name} at split setting {setting} (S = {sched.S}, cap {sched.cap}): {what} of output "
                    f"({row}, {col}) differs; its splits: " +
                    ", ".join(f"[{g.j0},{g.j1}) {g.cls} top {g.top} events {g.events}" for g in gs))
    return None
