"""GPU: the DP noise kernel's Box-Muller over every uniform it can draw (tests/box_muller_domain.py).

efl_dp_box_muller puts chosen Philox words through the device functions k_dp_noise runs
(csrc/mask.hip box_muller and box_muller_staged<NB>, with log_unit / radius_unit of
csrc/box_muller_math.h and csrc/sincos_angle.h) and hands out the stage values r, sn, cs beside the
normals. Every sweep runs at nb = 0 (per pair), 1, 2 and 4 (staged), the five outputs must be equal
bit for bit across nb, and the common value is compared with the reference once.

* Every radius (2^23 values of u1, at the angle of u = 0.25 where sn = 1.0 exactly): the radius is
  within 1 ulp of the oracle's float chain for every k. That is the gate the project's ULP_TOL = 4
  requires: the header's sin / cos with the oracle's own radius is up to 2 ulp from the oracle's
  normal, a radius 1 ulp off makes that 3, a radius 2 ulp off up to 5
  (tests/test_box_muller_domain_host.py asserts the reference's share of this).
* Every angle (2^23 values of u, at the radius of u1 = 0.5): sn and cs equal the host build of the
  header bit for bit (the chunk digests of tests/golden/box_muller_domain.json), and the normals are
  the float32 products of the returned stages (no contraction, no reordering).
* Both marginals paired by two bijections: the normals within ULP_TOL of oracle/mask.py.
* The entry speaks for the production kernel: k_dp_noise's normals at every blocks-per-lane setting
  equal the entry's on the same Philox words.
* Ragged last groups of the entry's own kernel.
"""
import numpy as np
import pytest
import torch

import box_muller_domain as bm
from oracle import mask
from test_dp_gpu import ULP_TOL, kernel_normals
from test_dp_oracle import CLAMP_BLOCK, CLAMP_SEED

pytestmark = pytest.mark.gpu

NBS = (0, 1, 2, 4)
NAMES = ("r", "sn", "cs", "z0", "z1")


@pytest.fixture(scope="module")
def lib():
    import efl
    efl.lib.require_gpu()
    return efl.lib.raw()


@pytest.fixture(scope="module")
def dp():
    import efl
    efl.lib.require_gpu()
    from efl.privacy import dp_optimizer
    return dp_optimizer


def dev_words(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).cuda()


def run(lib, x0: torch.Tensor, x1: torch.Tensor, nb: int, stages: bool = True, pad: int = 0):
    """One efl_dp_box_muller call: the five outputs as device tensors (r, sn, cs None without stages).
    `pad` extra elements behind each output hold a canary the kernel must leave alone."""
    import efl
    n = x0.numel()
    outs = [torch.full((n + pad,), 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)
            if stages or i >= 3 else None for i in range(5)]
    ptrs = [o.data_ptr() if o is not None else None for o in outs]
    efl.lib.check(lib.efl_dp_box_muller(x0.data_ptr(), x1.data_ptr(), n, nb, *ptrs, efl.lib.stream_handle(x0.device)))
    if pad:
        for o in outs:
            if o is not None:
                assert (o[n:].view(torch.int32) == 0x7FC0BEEF).all(), "a store past the last pair"
    return [o[:n] if o is not None else None for o in outs]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def sweep(lib, x0: np.ndarray, x1: np.ndarray) -> dict:
    """The five outputs of the words at nb = 0, required equal bit for bit at nb = 1, 2, 4; numpy."""
    d0, d1 = dev_words(x0), dev_words(x1)
    base = run(lib, d0, d1, 0)
    for nb in NBS[1:]:
        for name, a, b in zip(NAMES, base, run(lib, d0, d1, nb)):
            assert same_bits(a, b), (name, "nb", nb, "differs from the per-pair path")
    # without the stage outputs the normals are the same
    z = run(lib, d0, d1, 4, stages=False)
    assert z[0] is None and same_bits(z[3], base[3]) and same_bits(z[4], base[4])
    return {name: t.cpu().numpy() for name, t in zip(NAMES, base)}


def products_are_the_stages(out: dict):
    assert np.array_equal(bm.bits(out["z0"]), bm.bits(out["sn"] * out["r"])), "z0 is not fl(sn r)"
    assert np.array_equal(bm.bits(out["z1"]), bm.bits(out["cs"] * out["r"])), "z1 is not fl(cs r)"


def test_every_radius(lib):
    """Measured on an MI355X: 0 / 1 ulp from the oracle's chain for 6,987,992 /
    1,400,616 k. With round 5's log_unit / sqrt_normal it was 0 / 1 / 2 ulp for 6,383,186 /
    1,994,520 / 10,902 k (k = 4070 the first), which is what csrc/box_muller_math.h now corrects."""
    x0, x1 = bm.radius_words()
    out = sweep(lib, x0, x1)
    r = out["r"]
    assert (bm.bits(out["sn"]) == 0x3F800000).all()
    assert bm.load_fixture()["quarter"]["sn"] == "3f800000"
    assert np.array_equal(bm.bits(out["z0"]), bm.bits(r))
    products_are_the_stages(out)
    assert int(bm.bits(r[:1])[0]) == bm.R_CLAMP_BITS
    assert not np.isnan(r).any() and (r > 0).all()
    up = np.nonzero(np.diff(r.astype(np.float64)) > 0)[0]
    assert up.size == 0, ("the radius rises at k =", up[:8] + 1)
    d = bm.ulps(r, bm.oracle_radius())
    worst = np.nonzero(d == d.max())[0]
    print("radius vs the oracle's chain: count per ulp distance", np.bincount(d).tolist(), "worst at k =", worst[:8])
    d64 = bm.ulps(r, bm.radius_f64(x0))
    print("radius vs the rounded float64 radius: count per ulp distance", np.bincount(d64).tolist())
    assert d.max() <= 1, (np.bincount(d).tolist(), worst[:16])
    # Uint32ToFloat masks the high nine bits of both words
    hi = np.uint32(bm.HIGH)
    d0, d1 = dev_words(x0 | hi), dev_words(x1 | hi)
    for nb in NBS:
        for name, t in zip(NAMES, run(lib, d0, d1, nb)):
            assert np.array_equal(bm.bits(t.cpu().numpy()), bm.bits(out[name])), (name, nb)


def test_every_angle(lib):
    x0, x1 = bm.angle_words()
    out = sweep(lib, x0, x1)
    fx = bm.load_fixture()["digests"]
    for name in ("sn", "cs"):
        got = bm.chunk_digests(out[name])
        bad = [i for i in range(bm.CHUNKS) if got[i] != fx[name][i]]
        assert not bad, (name, "differs from the host header in the chunks", bad[:8])
    assert (bm.bits(out["r"]) == bm.bits(out["r"][:1])[0]).all()
    assert bm.ulps(out["r"][:1], bm.oracle_radius()[bm.HALF:bm.HALF + 1]).max() <= 1
    products_are_the_stages(out)


@pytest.mark.parametrize("multiplier", bm.MULTIPLIERS)
def test_both_marginals_paired(lib, multiplier):
    """Measured on an MI355X: worst 3 ulp at both multipliers (about 19,500 z0 and
    29,000 z1 at 3). With round 5's radius: 4 ulp at 0x9E3779B1, 5 ulp for two pairs at 0x85EBCA6B."""
    x0, x1 = bm.paired_words(multiplier)
    assert bm.is_bijection(x0) and bm.is_bijection(x1)
    out = sweep(lib, x0, x1)
    products_are_the_stages(out)
    for name in NAMES:
        assert not np.isnan(out[name]).any(), name
    w0, w1 = bm.oracle_paired(multiplier)
    d0, d1 = bm.ulps(out["z0"], w0), bm.ulps(out["z1"], w1)
    print("multiplier %#x: z0 count per ulp distance" % multiplier, np.bincount(d0).tolist(),
          "z1", np.bincount(d1).tolist())
    assert max(d0.max(), d1.max()) <= ULP_TOL, (np.bincount(d0).tolist(), np.bincount(d1).tolist())


FULL_AND_TAIL = 4 * 256 * 4 * 3 + 7         # three full tiles of the widest kernel and a ragged tail
PRODUCTION = [(CLAMP_SEED, CLAMP_BLOCK, 5), (CLAMP_SEED, CLAMP_BLOCK - 1000, FULL_AND_TAIL),
              (0x9E3779B97F4A7C15, 7, 5), (0x9E3779B97F4A7C15, 2 ** 32 - 1536, FULL_AND_TAIL),
              (99, 17, 4 * 256 * 4)]


@pytest.mark.parametrize("seed,ctr0,n", PRODUCTION)
def test_entry_speaks_for_the_production_kernel(lib, dp, seed, ctr0, n):
    """k_dp_noise's normals (full tiles through normals<NB>, the tail through normal4) are the
    entry's on the same Philox words, at every blocks-per-lane setting."""
    w = mask.philox_blocks(seed, ctr0, (n + 3) // 4)
    if (seed, ctr0) == (CLAMP_SEED, CLAMP_BLOCK):
        assert w[0, 2] & 0x7FFFFF == 0                       # the clamp is among the words
    x0, x1 = dev_words(w[:, 0::2].reshape(-1)), dev_words(w[:, 1::2].reshape(-1))
    old = lib.efl_fxp_tune(20, -1)
    try:
        for nb in (1, 2, 4):
            assert lib.efl_fxp_tune(20, nb) >= 0
            z = kernel_normals(dp, seed, ctr0, n)
            for enb in (0, nb):
                out = run(lib, x0, x1, enb)
                want = torch.stack([out[3], out[4]], dim=1).reshape(-1)[:n].cpu().numpy()
                bad = np.nonzero(bm.bits(z) != bm.bits(want))[0]
                assert bad.size == 0, ("kernel nb", nb, "entry nb", enb, "elements", bad[:8])
    finally:
        lib.efl_fxp_tune(20, old)


@pytest.mark.parametrize("nb", [1, 2, 4])
def test_ragged_groups(lib, nb):
    """A lane of the staged kernel owns 2 nb consecutive pairs; the last lane's short group runs pair
    by pair. Same bits as the per-pair kernel, and nothing stored past pair n - 1."""
    rng = np.random.default_rng(23)
    for n in (1, 2 * nb - 1, 2 * nb + 1, 64 * 2 * nb + 1, 12345):
        a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        b = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        a[0] &= np.uint32(bm.HIGH)                           # the clamp, first
        a[-1] |= np.uint32(bm.MASK)                          # the largest u1, last
        x0, x1 = dev_words(a), dev_words(b)
        want = run(lib, x0, x1, 0, pad=64)
        got = run(lib, x0, x1, nb, pad=64)
        for name, g, w in zip(NAMES, got, want):
            assert same_bits(g, w), (name, n)
        z = run(lib, x0, x1, nb, stages=False, pad=64)
        assert same_bits(z[3], want[3]) and same_bits(z[4], want[4])


def test_empty_call_touches_nothing(lib):
    e = torch.empty(0, dtype=torch.int32, device="cuda")
    out = run(lib, e, e, 4, pad=8)
    assert all(o.numel() == 0 for o in out)
    assert lib.efl_dp_box_muller(None, None, 0, 0, None, None, None, None, None, None) == 0
    assert lib.efl_dp_box_muller(e.data_ptr(), e.data_ptr(), 4, 3, None, None, None, None, None, None) == -3
