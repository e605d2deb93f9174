"""GPU: the Philox streams of the mask and DP-noise kernels (csrc/mask.hip) over the whole 64-bit
key and counter domain, against the numpy oracle (oracle/mask.py), bit for bit (the normals within
test_dp_gpu.ULP_TOL).

In production the key's high word is never zero (NoiseStream seeds itself from os.urandom(8)) and the
block counter passes 2^32 after 256 masks of 64 Mi elements; the other GPU tests use small seeds and
counters, for which k1 = seed >> 32 and c[1] = ctr >> 32 are zero in every launch. Here every kernel
that forms a Philox key and counter (draw4, uniforms<NB>, normal4, normals<NB> and the block index
arithmetic in front of them) runs with

* the seeds A = 0xDEADBEEFCAFEF00D (k0 != k1, both non-zero), B = 0xFFFFFFFF00000000 (k0 == 0) and
  C = 2^64 - 1;
* for a call of G Philox blocks, the counters 2^32 - k and 2^64 - k for k in {1, G // 2, G - 1}
  (the carry into the high word, or the wrap to 0, on the second block, in mid-call, and on the last
  block, which is the ragged tail where the shape has one) and 0x0123456789ABCDEF (a high word that
  is non-zero from the first block). Every counter runs with seed A; B and C run at 2^32 - G // 2.

Also here: the power-of-two divisors of efl_ss_noise (the DIV == 1 instantiations and the host's
choice between the reciprocal and the IEEE division, at the edge where 1 / d stops being normal).

The store flavour (efl_fxp_tune 28) stays at its default: it does not touch Philox. Every test names
the kernel instantiations its shapes and knobs reach, so that a change of launch shapes can see what
has to be covered again."""
import numpy as np
import pytest
import torch

from oracle import mask
from test_dp_gpu import ULP_TOL, kernel_normals, ulps
from test_mask_gpu import bits, nbits, rand

pytestmark = pytest.mark.gpu

A = 0xDEADBEEFCAFEF00D
B = 0xFFFFFFFF00000000
C = 2**64 - 1
HIGH = 0x0123456789ABCDEF
M64 = 2**64 - 1


def stream_cases(G):
    """(seed, ctr0) of a call that consumes G Philox blocks (the module docstring's list)."""
    assert G >= 2
    ks = sorted({k for k in (1, G // 2, G - 1) if k >= 1})
    ctrs = [2**32 - k for k in ks] + [2**64 - k for k in ks] + [HIGH]
    return [(A, c) for c in ctrs] + [(B, 2**32 - G // 2), (C, 2**32 - G // 2)]


def test_stream_cases_cover_the_carries():
    """The case list itself: for G = 3073 the 32-bit carry and the 64-bit wrap each fall on block 1,
    block G // 2 and block G - 1; a two-block call has one carry position."""
    cs = stream_cases(3073)
    assert [(s, c) for s, c in cs if s == A] == [(A, c) for c in (
        2**32 - 1, 2**32 - 1536, 2**32 - 3072, 2**64 - 1, 2**64 - 1536, 2**64 - 3072, HIGH)]
    assert cs[-2:] == [(B, 2**32 - 1536), (C, 2**32 - 1536)]
    assert stream_cases(2) == [(A, 2**32 - 1), (A, 2**64 - 1), (A, HIGH), (B, 2**32 - 1), (C, 2**32 - 1)]


@pytest.fixture(scope="module")
def ss():
    import efl
    efl.lib.require_gpu()
    return efl.secret_sharing


@pytest.fixture(scope="module")
def dp():
    import efl
    efl.lib.require_gpu()
    from efl.privacy import dp_optimizer
    return dp_optimizer


@pytest.fixture(scope="module")
def lib():
    import efl
    efl.lib.require_gpu()
    return efl.lib.raw()


def tup(v):
    return v if isinstance(v, tuple) else (v,)


def oracle_noise(x, seed, ctr, op, div):
    with np.errstate(all="ignore"):          # inf - inf, overflow and underflow behave as the fp32 ops do
        return tup(mask.noise(x, seed, ctr, op, div))


def check_noise(ss, x, xd, op, div, seed, ctr, what):
    st = ss.NoiseStream(seed, ctr)
    got = tup(ss._noise(xd, op, div, stream=st))
    want = oracle_noise(x, seed, ctr, op, div)
    assert len(got) == len(want)
    for o, (g, w) in enumerate(zip(got, want)):
        bad = np.nonzero(bits(g) != nbits(w))[0]
        assert bad.size == 0, (what, op, div, hex(seed), hex(ctr), "output", o, "elements", bad[:8])
    assert st.counter == (ctr + (x.size + 3) // 4) & M64


NOISE_N = (5, 4 * 33 + 2, 4 * 256 * 4 * 3 + 4)
# (op, efl_fxp_tune(30, .), efl_fxp_tune(25, .))
NOISE_KNOBS = [(0, None, 1), (0, None, 2), (0, None, 4),
               (1, 1, None), (2, 1, None),
               (1, 0, 1), (1, 0, 2), (1, 0, 4), (2, 0, 1), (2, 0, 2), (2, 0, 4)]


@pytest.mark.parametrize("op,half,nb", NOISE_KNOBS)
def test_noise_whole_domain(ss, lib, op, half, nb):
    """efl_ss_noise. Op 0 at efl_fxp_tune(25, nb) runs k_noise<0, 0, NB, 0>; ops 1 and 2 run
    k_noise_half<OP, DIV, 7> at efl_fxp_tune(30, 1) and k_noise<OP, DIV, NB, 7> at (30, 0), with
    DIV 0 (ops 0, 1: divisor 1) and 2 (op 2: divisor 3, the IEEE division). n = 5 is a lone partial
    group (draw4 and the scalar tail), 4 * 33 + 2 a partial wave ending in a partial group (draw4),
    4 * 256 * 4 * 3 + 4 three full NB = 4 tiles (uniforms<NB>, for NB = 1 and 2 more tiles) plus one
    group that takes the per-group tail (draw4) at NB > 1."""
    prev_half = lib.efl_fxp_tune(30, half) if half is not None else None
    if nb is not None:
        assert lib.efl_fxp_tune(25, nb) >= 0
    try:
        for n in NOISE_N:
            x = rand(n, n + 11)
            xd = torch.from_numpy(x).cuda()
            for seed, ctr in stream_cases((n + 3) // 4):
                check_noise(ss, x, xd, op, 3.0 if op == 2 else 1.0, seed, ctr, n)
    finally:
        if prev_half is not None:
            lib.efl_fxp_tune(30, prev_half)
        lib.efl_fxp_tune(25, -2)


def check_mask(got, want, what):
    assert len(got) == len(want) == 3
    for o, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape
        bad = np.nonzero((bits(g) != nbits(w)).reshape(-1))[0]
        assert bad.size == 0, what + ("output", o, "elements", bad[:8])


@pytest.mark.parametrize("R,Cn", [(3, 8), (5, 24), (257, 1024), (7, 12), (33, 100)])
def test_mask_cols_whole_domain(ss, lib, R, Cn):
    """efl_ss_mask_cols. Columns % 8 == 0 run k_mask_cols4<NB, 2> at efl_fxp_tune(25, nb), nb in 1, 2,
    4: [3, 8] (6 groups) and [5, 24] (30 groups) are one partial wave each (draw4, the per-group
    path), [257, 1024] is 65,792 groups = 64 full NB = 4 tiles (uniforms<NB>) plus one workgroup whose
    lanes own only their first group (draw4), with div_groups by 256. [7, 12] and [33, 100] run
    k_mask_cols2 (one lane per column pair, draw4 on element index >> 2, word chosen per element)."""
    a = rand((R, Cn), R * 1000 + Cn)
    ad = torch.from_numpy(a).cuda()
    nbs = (1, 2, 4) if Cn % 8 == 0 else (None,)
    try:
        for seed, ctr in stream_cases((R * Cn + 3) // 4):
            with np.errstate(all="ignore"):
                want = mask.mask_cols(a, seed, ctr)
            for nb in nbs:
                if nb is not None:
                    assert lib.efl_fxp_tune(25, nb) >= 0
                st = ss.NoiseStream(seed, ctr)
                check_mask(ss.mask_cols(ad, stream=st), want, (R, Cn, nb, hex(seed), hex(ctr)))
                assert st.counter == (ctr + (R * Cn + 3) // 4) & M64
    finally:
        lib.efl_fxp_tune(25, -2)


@pytest.mark.parametrize("K,N", [(2, 4), (6, 132), (514, 1024), (10, 13), (6, 3)])
def test_mask_rows_whole_domain(ss, lib, K, N):
    """efl_ss_mask_rows. Columns % 4 == 0 run k_mask_rows_half<NB, 7> at efl_fxp_tune(29, 1) and
    k_mask_rows<4, NB, 7> at (29, 0), nb in 1, 2, 4 (kind 25): [2, 4] is one lane group (two Philox
    blocks, one per row of the pair), [6, 132] 33 groups a row pair (a partial wave; draw4 in
    k_mask_rows, uniforms<NB> with invalid lanes in the halves kernel), [514, 1024] 65,792 groups
    (uniforms<2 NB> over whole tiles, then the per-group draw4 path in the last workgroup), each
    group's block index made from its row and column by div_groups. [10, 13] and [6, 3] run
    k_mask_rows<1, 1, 0>, one column a lane (draw4 on element index >> 2, word chosen per element)."""
    b = rand((K, N), K * 1000 + N)
    bd = torch.from_numpy(b).cuda()
    variants = [(h, nb) for h in (0, 1) for nb in (1, 2, 4)] if N % 4 == 0 else [(None, None)]
    prev_half = lib.efl_fxp_tune(29, -1)
    try:
        for seed, ctr in stream_cases((K * N + 3) // 4):
            with np.errstate(all="ignore"):
                want = mask.mask_rows(b, seed, ctr)
            for h, nb in variants:
                if h is not None:
                    assert lib.efl_fxp_tune(29, h) >= 0 and lib.efl_fxp_tune(25, nb) >= 0
                st = ss.NoiseStream(seed, ctr)
                check_mask(ss.mask_rows(bd, stream=st), want, (K, N, h, nb, hex(seed), hex(ctr)))
                assert st.counter == (ctr + (K * N + 3) // 4) & M64
    finally:
        lib.efl_fxp_tune(29, prev_half)
        lib.efl_fxp_tune(25, -2)


@pytest.mark.parametrize("n", [7, 4097, 12292])
def test_dp_normals_whole_domain(dp, lib, n):
    """efl_dp_noise, the normals read back exactly (mode 1, x = 0, sigma = 1, divisor = 1:
    k_dp_noise<1, false, NB> at efl_fxp_tune(20, nb), nb in 1, 2, 4): within ULP_TOL of the oracle's
    normals and bit-identical between the three nb. n = 7 is one full and one partial group (normal4,
    the scalar tail); 4097 is 1,024 full groups (normals<NB> with blk0 + b * kBlock) and a lone
    element in a second workgroup (NB = 1: a fifth; normal4); 12292 is three full NB = 4 tiles
    (normals<4>) plus one group that takes normal4 at NB > 1."""
    old = lib.efl_fxp_tune(20, -1)
    try:
        for seed, ctr in stream_cases((n + 3) // 4):
            want = mask.normal(seed, ctr, n)
            zs = []
            for nb in (1, 2, 4):
                assert lib.efl_fxp_tune(20, nb) >= 0
                zs.append(kernel_normals(dp, seed, ctr, n))
                u = ulps(zs[-1], want)
                assert u.max() <= ULP_TOL, (n, nb, hex(seed), hex(ctr), int(u.argmax()), int(u.max()))
            for z in zs[1:]:
                assert np.array_equal(z.view(np.uint32), zs[0].view(np.uint32)), (n, hex(seed), hex(ctr))
    finally:
        lib.efl_fxp_tune(20, old)


def test_noise_stream_wraps_and_masks(ss):
    """NoiseStream at the top of the counter range: take() hands out the unwrapped start and wraps the
    counter to 64 bits, a mask drawn through it (k_noise<0, 0, 2, 0>, the default op-0 kernel, 20
    elements = 5 blocks of which the third is block 0) is the oracle's at that counter and the next
    mask continues from the wrapped counter; reset() (and so the constructor and set_seed) masks the
    counter to 64 bits as it masks the seed."""
    st = ss.NoiseStream(A, 2**64 - 2)
    assert st.take(20) == (A, 2**64 - 2)
    assert st.counter == 3
    x = rand(20, 20)
    xd = torch.from_numpy(x).cuda()
    st = ss.NoiseStream(A, 2**64 - 2)
    got = ss.generate_suitable_noise(xd, stream=st)
    assert np.array_equal(bits(got), nbits(oracle_noise(x, A, 2**64 - 2, 0, 1.0)[0]))
    assert st.counter == 3
    got = ss.generate_suitable_noise(xd, stream=st)
    assert np.array_equal(bits(got), nbits(oracle_noise(x, A, 3, 0, 1.0)[0]))
    assert st.counter == 8
    assert ss.NoiseStream(1, -1).counter == 2**64 - 1
    assert ss.NoiseStream(-1, 2**64 + 5).take(4) == (2**64 - 1, 5)
    st.reset(7, -3)
    assert (st.seed, st.counter) == (7, 2**64 - 3)


# a few inputs around the normal / subnormal line, so that u x / d lands on both sides of it for the
# divisors below
TINY = np.array([2.0**-140, -(2.0**-139), 1.5 * 2.0**-133, 2.0**-127, -1.75 * 2.0**-126, 2.0**-126,
                 1.25 * 2.0**-125, -(2.0**-120), 3.0 * 2.0**-122], np.float32)
POW2_DIVISORS = [4.0, -2.0, 2.0**-126, 2.0**126, 2.0**127, 2.0**-130]


def pow2_inputs(n):
    x = rand(n, n + 5)
    if n >= 64:
        x[9:9 + TINY.size] = TINY                # after rand's specials
        x[n - TINY.size:] = -TINY                # and in the last groups (the tail paths)
        return [x]
    t = np.resize(TINY, n).astype(np.float32)
    return [x, t, -t[::-1].copy()]


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nb", [1, 2, 4])
@pytest.mark.parametrize("op", [0, 1, 2])
def test_noise_power_of_two_divisors(ss, lib, op, nb, half):
    """efl_ss_noise with power-of-two divisors. 4, -2, 2^-126 and 2^126 (reciprocal 2^-126, the
    smallest normal) take the reciprocal: k_noise<OP, 1, NB, ST> (op 0 at every efl_fxp_tune(30, .);
    ops 1 and 2 at (30, 0)) and k_noise_half<OP, 1, 7> (ops 1 and 2 at (30, 1), whatever nb). 2^127
    (a subnormal reciprocal) and 2^-130 (a subnormal divisor whose reciprocal overflows) take the IEEE
    division, DIV == 2 of the same kernels. n = 5 is the scalar tail, 12292 full NB = 4 tiles plus a
    group in the per-group tail. The oracle divides in numpy float32; results on both sides of the
    normal / subnormal line, infinities and NaN included, are equal bit for bit."""
    for d in POW2_DIVISORS:                        # the divisors are what they are said to be
        assert np.float32(d) == d and np.frexp(abs(d))[0] == 0.5
    assert np.float32(1.0) / np.float32(2.0**126) == np.float32(2.0**-126) and 2.0**-126 == np.finfo(np.float32).tiny
    prev_half = lib.efl_fxp_tune(30, half)
    assert lib.efl_fxp_tune(25, nb) >= 0
    try:
        for n in (5, 12292):
            for x in pow2_inputs(n):
                xd = torch.from_numpy(x).cuda()
                for div in POW2_DIVISORS:
                    check_noise(ss, x, xd, op, div, A, 2**32 - 1, n)
    finally:
        lib.efl_fxp_tune(30, prev_half)
        lib.efl_fxp_tune(25, -2)
