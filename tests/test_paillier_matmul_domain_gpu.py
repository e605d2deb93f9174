"""GPU: efl_pl_matmul exactly on its shape, split and schedule boundaries, against
oracle.paillier.matmul bit for bit (mantissas and exponents; there is no tolerance).

The cases come from tests/matmul_domain.py, whose schedule model says which class every (output,
split) of a launch falls in; tests/test_matmul_domain_host.py proves on the CPU that the lists reach
every class ("hist": the LDS counting sort of k_mmevents, "scan": its level-major scan,
"unlisted-levels" / "unlisted-cap" / "unlisted-wide": k_matmul28 scans the terms itself, "empty": a
split of zeros) and sit exactly on every boundary: top levels 127 / 128 / 129 and 1023 / 1024 /
1025, event counts cap and cap + 1 for cap 10, 20 and 4096, split widths 65,536 and 65,537, term
splits up to 16 with uneven widths. The model only names what a failing output ran through; the
oracle alone judges.

Three kernel configurations, each asserted from the key descriptor before it runs:

* the radix-2^28 kernels (k_wmask, k_mmevents, k_tomont28<C, G>, k_matmul28<C, G>, k_matcomb28<C, G>):
  the key is built inside family(c), so its radix-2^28 table is the family's own;
* the 32-bit sliced k_matmul<C, G> (csrc/paillier_sliced.hip): the key's table was built for
  another lane count;
* the one-lane k_matmul<LN> (csrc/paillier.hip): family 0.

The term-split setting (efl_pl_tune(ln, 3, S)) only exists in the first. Oracle results are memoised
per (key, case): they depend on neither the family nor S, and they are nearly all of the run time.
Every test names the kernel instantiations and classes it reaches, so that a change of the launch
constants can see what has to be covered again."""
import pytest
import torch

import matmul_domain as md
from oracle import paillier as P
from test_paillier_gpu import ALL, SLICINGS, family, fams, keypair

pytestmark = pytest.mark.gpu

K512, K1024, K4096 = ALL[0], ALL[1], ALL[3]
_ORACLE, _KEYS, _PLANS = {}, {}, {}


@pytest.fixture(scope="module")
def efl():
    import efl as _efl
    _efl.lib.require_gpu()
    return _efl


def n2_of(k):
    return int(k["n"], 16) ** 2


def plans(k, which):
    """The case lists of a key, built once (xm is drawn below the key's n^2)."""
    key = (k["n_bytes"], which)
    if key not in _PLANS:
        n2 = n2_of(k)
        _PLANS[key] = {"full": lambda: md.plan(n2), "reduced": lambda: md.plan(n2, reduced=True),
                       "wide": lambda: [("WIDE", c, s) for c, s in md.wide_plan(n2)]}[which]()
    return _PLANS[key]


def key_for(efl, k, c):
    """A public key built while family c is selected (c None: the default family), kept for the
    module: its radix-2^28 table, if any, belongs to that family's lane count."""
    ln = k["n_bytes"] // 4
    if (ln, c) not in _KEYS:
        if c is None:
            _KEYS[ln, c] = keypair(efl, k, private=False)
        else:
            with family(ln, False, c):
                _KEYS[ln, c] = keypair(efl, k, private=False)
    return _KEYS[ln, c]


def runs_radix28(kp, ln, c):
    d = kp.key.desc
    return c > 0 and d.off_table28 >= 0 and (1 << d.table28_log2g) == 2 * ln // c


def oracle(k, case):
    key = (k["n_bytes"], case.name)
    if key not in _ORACLE:
        okp = P.Keypair(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, 1)
        _ORACLE[key] = P.matmul(okp, case.xm, case.xe, case.ym, case.ye)
    return _ORACLE[key]


def run_case(efl, kp, k, case, setting=None):
    """One launch (at a term-split setting, radix-2^28 only) against the oracle."""
    u, v, w = md.shape(case)
    lib, ln = efl.lib.raw(), k["n_bytes"] // 4
    x = efl.HexTensor.from_ints([c for row in case.xm for c in row], (u, v))
    args = [torch.tensor(t, dtype=torch.int64) for t in (case.xe, case.ym, case.ye)]
    prev = lib.efl_pl_tune(ln, 3, setting) if setting is not None else None
    try:
        assert setting is None or lib.efl_pl_tune(ln, 3, -1) == setting
        zm, ze = kp.matmul(x, *args)
    finally:
        if setting is not None:
            lib.efl_pl_tune(ln, 3, prev)
    want_m, want_e = oracle(k, case)
    msg = md.first_difference(case, setting or 0, zm.to_hex().to_ints(), ze.cpu().reshape(-1).tolist(), want_m, want_e)
    assert not msg, msg


def run_plan(efl, k, c, plan, only=None):
    """Every (case, setting) of the plan's lists in `only` through the radix-2^28 kernels of family c."""
    ln = k["n_bytes"] // 4
    kp = key_for(efl, k, c)
    with family(ln, False, c):
        assert runs_radix28(kp, ln, c), "the key's radix-2^28 table must be this family's"
        for lst, case, settings in plan:
            if only is None or lst in only:
                for s in settings:
                    run_case(efl, kp, k, case, s)


RADIX28_512 = [c for c in SLICINGS[16][0] if c]


@pytest.mark.parametrize("c", RADIX28_512)
def test_radix28_geometry(efl, c):
    """GEO x S in {0, 1, 2, 4, 8, 16}: k_tomont28 / k_matmul28 / k_matcomb28 <8, 4>, <16, 2>, <32, 1>
    (E = 16 / 32 / 64 outputs per block) and k_mmevents with outputs below, at and past one block, u
    that does not divide E (a wave straddles output columns), v = 1 (S stays 1), and the uneven
    splits of v = 9 at S = 8 and v = 17 / 33 at S = 16, where k_matcomb28 combines 8 and 16
    partials. Classes: "hist", and "empty" for a split whose only terms are zero."""
    run_plan(efl, K512, c, plans(K512, "full"), {"GEO"})


@pytest.mark.parametrize("c", RADIX28_512)
def test_radix28_level_boundaries(efl, c):
    """LEVELS x S in {0, 1, 2, 4}: top levels exactly 1, 127, 128 ("hist": the last rows of the LDS
    histogram), 129, 1023, 1024 ("scan": the last value of the 10-bit level field) and 1025, 1100
    ("unlisted-levels"), six different in one wave and one launch each; with S = 2 and 4 the far
    term's split and its neighbours take different builders. Also the minimum exponent at a y = 0
    term (the tops land on 127 / 128 / 129 because of it) and every exponent moved by +-2^40."""
    run_plan(efl, K512, c, plans(K512, "full"), {"LEVELS"})


@pytest.mark.parametrize("c", RADIX28_512)
def test_radix28_capacity_boundaries(efl, c):
    """CAP: lists of exactly cap events (listed: the last word of the list's span of the slab is
    written) and cap + 1 (unlisted), for cap = 20 (v = 4, S = 1), 10 (S = 2: a split at cap next to
    one past it) and the 4096 limit (v = 820), each through k_mmevents' counting sort ("hist") and
    through its level scan ("scan"), listed and "unlisted-cap" groups in one wave."""
    run_plan(efl, K512, c, plans(K512, "full"), {"CAP"})


@pytest.mark.parametrize("c", RADIX28_512)
def test_radix28_values(efl, c):
    """VALUES x S in {0, 1, 2, 4}: k_wmask and the window entries over y = 0, +-1, +-2, 31, 32, 33,
    2^62, +-(2^63 - 1), -2^63, the alternating patterns and dense 63-bit values ("unlisted-cap":
    about 12 windows a term); columns of zeros (the output is 1 at the minimum exponent: "empty"),
    of one sign only, of a single term (with S > 1 its other splits' partials are R); and a launch
    without any negative y (the host skips the inverse)."""
    run_plan(efl, K512, c, plans(K512, "full"), {"VALUES"})


def test_radix28_wide_splits(efl):
    """WIDE, default family: v = 65,536 at S = 1 (term index 65,535 in the 16-bit field, "hist"),
    v = 65,537 at S = 1 ("unlisted-wide": k_matmul28 scans 65,537 terms per level) and at S = 2
    (splits of 32,768 and 32,769 terms, listed again)."""
    from efl.privacy import paillier_cipher as pc
    c = pc.kernel_slicing(16, False)
    assert c > 0
    kp = key_for(efl, K512, None)
    assert runs_radix28(kp, 16, c)
    for _, case, settings in plans(K512, "wide"):
        for s in settings:
            run_case(efl, kp, K512, case, s)


def other_lists(k):
    """GEO, VALUES and the six-tops LEVELS launch: what the two older kernels run (no S there)."""
    return [case for lst, case, _ in plans(k, "full")
            if lst in ("GEO", "VALUES") or case.name.startswith("levels-six-tops")]


@pytest.mark.parametrize("built,c", [(8, 16), (16, 32), (32, 8)])
def test_sliced_kernel(efl, built, c):
    """The 32-bit sliced k_matmul<16, 2>, <32, 1>, <8, 4>: a key whose radix-2^28 table was built for
    another lane count. GEO, VALUES and the six tops in one launch (up to 1024 squarings of one term
    next to lanes that have none)."""
    kp = key_for(efl, K512, built)
    with family(16, False, c):
        d = kp.key.desc
        assert d.off_table28 >= 0 and (1 << d.table28_log2g) == 32 // built != 32 // c
        assert not runs_radix28(kp, 16, c)
        for case in other_lists(K512):
            run_case(efl, kp, K512, case)


def test_one_lane_kernel(efl):
    """The one-lane k_matmul<16> of csrc/paillier.hip (family 0; the key holds no radix-2^28 table):
    GEO, VALUES and the six tops in one launch."""
    from efl.privacy import paillier_cipher as pc
    kp = key_for(efl, K512, 0)
    with family(16, False, 0):
        assert kp.key.desc.off_table28 == -1 and pc.kernel_slicing(16, False) == 0
        for case in other_lists(K512):
            run_case(efl, kp, K512, case)


@pytest.mark.parametrize("lst", ["GEO", "LEVELS", "CAP"])
@pytest.mark.parametrize("k,c", fams([K1024, K4096]))
def test_larger_keys(efl, k, c, lst):
    """The examples' 1024-bit key (k_matmul28 / k_matcomb28 <8, 8>, <16, 4>, <32, 2>, and the one-lane
    k_matmul<32> for family 0) and the reference's default 4096-bit key (<8, 32>, <16, 16>, <32, 8>:
    10-, 19- and 37-limb radix-2^28 slices padded to 12, 20 and 40 words), every family, reduced
    lists: GEO (17, 3, 4) and (7, 9, 5) at S = 0 and 8; the six tops 127 .. 1025 in one launch with
    two terms per output ("hist", "scan", "unlisted-levels" in one wave); the v = 4 CAP cases (cap
    20 and 10, "hist" / "scan" / "unlisted-cap")."""
    ln = k["n_bytes"] // 4
    if c:
        run_plan(efl, k, c, plans(k, "reduced"), {lst})
        return
    from efl.privacy import paillier_cipher as pc
    kp = key_for(efl, k, 0)
    with family(ln, False, 0):
        assert kp.key.desc.off_table28 == -1 and pc.kernel_slicing(ln, False) == 0
        for name, case, _ in plans(k, "reduced"):
            if name == lst:
                run_case(efl, kp, k, case)
