"""GPU: the Philox draw of the Paillier blinding exponent a (draw_a in csrc/paillier.hip and
csrc/paillier_sliced.hip) over the whole 64-bit key and counter domain, in every kernel that calls it.

Element i of a fresh-randomness call draws a from Philox(key = the keypair's seed, counter =
counter_base + i). In production the seed is a BLAKE2b-64 hash (high word non-zero) and the counter
passes 2^32 after about 43 k steps of the MNIST activation; a kernel that drops or mis-carries the
counter's high word repeats a from there on, which gives two ciphertexts the same hs^a factor. The
other GPU tests use small seeds and counter bases up to 1000. Here: the seeds A = 0xDEADBEEFCAFEF00D,
B = 0xFFFFFFFF00000000 (low word zero) and C = 2^64 - 1, and for N = 130 elements the counter bases
2^32 - 40 (the carry inside the first wave), 2^32 - N + 3 (among the last elements),
0x0123456789ABCDEF (a high word non-zero from the start) and 2^63 - N (the top of the int64_t
counter_base). The oracle is oracle/paillier.py over oracle/philox.draw_a."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import paillier as P
from oracle import philox
from test_paillier_gpu import SLICINGS, family

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "paillier_kat.json")) as f:
    KAT = json.load(f)
KEYS = [k for k in KAT["keys"] if k["n_bytes"] in (64, 128, 256)]     # 512-, 1024-, 2048-bit n
K512 = KEYS[0]
K1024 = KEYS[1]

A = 0xDEADBEEFCAFEF00D
B = 0xFFFFFFFF00000000
C = 2**64 - 1
N = 130
BASES = [2**32 - 40, 2**32 - N + 3, 0x0123456789ABCDEF, 2**63 - N]
# (seed, counter_base): every base with A, one case each with B and C
CASES = [(A, c) for c in BASES] + [(B, BASES[0]), (C, BASES[0])]
W = 5       # the tables' window: results never depend on it, and small tables build at once


@pytest.fixture(scope="module")
def efl():
    import efl as _efl
    _efl.lib.require_gpu()
    return _efl


@contextlib.contextmanager
def tune(efl, ln, kind, v):
    lib = efl.lib.raw()
    prev = lib.efl_pl_tune(ln, kind, v)
    assert prev >= 0
    try:
        yield
    finally:
        lib.efl_pl_tune(ln, kind, prev)


def make(efl, k, g, owner, window=W):
    kp = efl.paillier.Keypair(seed=A)
    kp.set_keys_ints(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, g,
                     int(k["p"], 16) if owner else None, int(k["q"], 16) if owner else None, table_window=window)
    return kp


def plaintexts(n, seed):
    m = torch.from_numpy(np.random.default_rng(seed).integers(-2**63, 2**63 - 1, n, dtype=np.int64))
    m[:4] = torch.tensor([0, -1, 2**63 - 1, -2**63])
    return m


def checked_elements(n, base):
    """The first and the last element and the ones at the counters 2^32 - 1, 2^32 and 2^32 + 1."""
    return sorted({0, n - 1} | {c - base for c in (2**32 - 1, 2**32, 2**32 + 1) if 0 <= c - base < n})


def hex_at(efl, kp, limbs, idx):
    pc = efl.privacy.paillier_cipher
    sub = limbs[torch.tensor(idx, device=limbs.device)]
    return pc.CipherTensor(sub, (len(idx),), kp.key).to_hex().strings()


def oracle_at(k, g, seed, base, idx, m=None):
    okp = P.Keypair(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, g)
    out = []
    for i in idx:
        hsa = P.fbpowm(okp.hs, okp.n2, philox.draw_a(seed, base + i, k["a_bits"]), g)
        out.append(P.hx(hsa if m is None else P.encrypt(okp, int(m[i]), hsa)))
    return out


def run(kp, m, seed, base):
    kp.seed = seed
    return kp.fbpowm(n=m.numel(), counter_base=base).limbs, kp.encrypt(m, counter_base=base).tensor.limbs


def test_checked_elements_sit_on_the_carry():
    assert checked_elements(N, BASES[0]) == [0, 39, 40, 41, 129]
    assert checked_elements(N, BASES[1]) == [0, 126, 127, 128, 129]
    assert checked_elements(N, BASES[2]) == [0, 129] and checked_elements(N, BASES[3]) == [0, 129]
    assert BASES[3] + N - 1 == 2**63 - 1


_KEYSETS = {}


def keyset(efl, k, g):
    """The keypairs of one (key, group size), made once and shared by the cases: a public key whose
    context was built under family 0 (no radix-2^28 table), one built under each sliced family C (its
    radix-2^28 table serves C), and the key owner."""
    ln = k["n_bytes"] // 4
    if (ln, g) not in _KEYSETS:
        with family(ln, False, 0):
            plain = make(efl, k, g, False)
        assert plain.key.ensure_table().desc.off_table28 < 0
        with28 = {}
        for c in [c for c in SLICINGS[ln][0] if c]:
            with family(ln, False, c):
                with28[c] = make(efl, k, g, False)
            d = with28[c].key.ensure_table().desc
            assert d.off_table28 >= 0 and (1 << d.table28_log2g) == 2 * ln // c
        owner = make(efl, k, g, True)
        assert owner.key.crt_capable() == (ln >= 32)
        if ln >= 32:
            assert owner.key.crt_keys() is not None
            info = owner.key.info()
            assert info.crt_table_window[0] == info.crt_table_window[1] == W   # what the paired lanes need
        _KEYSETS[(ln, g)] = (plain, with28, owner)
    return _KEYSETS[(ln, g)]


@pytest.mark.parametrize("seed,base", CASES, ids=lambda v: hex(v))
@pytest.mark.parametrize("g", [1, 10])
@pytest.mark.parametrize("k", KEYS, ids=lambda k: f"n{8 * k['n_bytes']}")
def test_every_family_draws_the_oracles_a(efl, k, g, seed, base):
    """fbpowm(n = 130) and encrypt of 130 plaintexts at one seed and counter base of the module, in
    every family of the key that draws a; all families equal each other on the raw limbs of every
    element and the oracle at the first and last element and around the 32-bit carry.

    * dense: a public key under family 0, k_fbpowm<LN> / k_encrypt<LN> (paillier.hip draw_a);
    * sliced C (8, 16, 32 limbs per lane): the same key, whose context was built under family 0 and so
      has no radix-2^28 table, under family C: k_fbpowm<C, G> / k_encrypt<C, G> (paillier_sliced.hip
      draw_a<G>, G = 2 ln / C lanes an element);
    * sliced28 C: a public key built under family C (table28_for): k_fbpowm28<C, G> /
      k_encrypt28<C, G> with efl_pl_tune(ln, 4, 1), and k_walk28_part<C, G, .> + k_walk28_join at
      walk parts P = 2, 3, 5 (130 elements are far below 4 waves a SIMD, so a fixed P always splits);
    * the key owner (p, q given), by CRT through the sub-keys of ln / 2 limbs at their default family
      32: 1024-bit n: k_crt_pair_mixed / k_crt_pair_tree at efl_pl_tune(16, 5, 0 and 2) and
      k_gstart28 + k_fbpowm28<32, 1> per key at (16, 5, 1); 2048-bit n: k_fbpowm28<32, 2> per key with
      efl_pl_crt_join; 512-bit n has no CRT sub-key class and takes the n^2 sliced28 path."""
    ln = k["n_bytes"] // 4
    plain, with28, owner = keyset(efl, k, g)
    m = plaintexts(N, ln + g)
    idx = checked_elements(N, base)
    with family(ln, False, 0):
        ref = run(plain, m, seed, base)
    assert hex_at(efl, plain, ref[0], idx) == oracle_at(k, g, seed, base, idx), "dense fbpowm"
    assert hex_at(efl, plain, ref[1], idx) == oracle_at(k, g, seed, base, idx, m), "dense encrypt"

    def same(got, what):
        for r, o, name in zip(ref, got, ("fbpowm", "encrypt")):
            bad = torch.nonzero((r != o).any(dim=1)).reshape(-1).tolist()
            assert not bad, (what, name, "elements", bad[:8])

    for c in with28:
        with family(ln, False, c):
            same(run(plain, m, seed, base), ("sliced", c))
            for parts in (1, 2, 3, 5):
                with tune(efl, ln, 4, parts):
                    same(run(with28[c], m, seed, base), ("sliced28", c, "parts", parts))
    for v in ((0, 1, 2) if ln == 32 else (0,)):
        with tune(efl, 16, 5, v):
            same(run(owner, m, seed, base), ("owner", "crt mode", v))
    owner.crt_encrypt = False                    # and the key owner on the public path
    try:
        same(run(owner, m, seed, base), ("owner", "public path"))
    finally:
        owner.crt_encrypt = True


@pytest.fixture(scope="module")
def pair_owner(efl):
    kp = efl.paillier.Keypair(seed=A)
    kp.set_keys_ints(int(K1024["n"], 16), int(K1024["hs"], 16), 64, 10, int(K1024["p"], 16), int(K1024["q"], 16))
    return kp


NP = 32768 + 65
PAIR_BASES = [2**32 - 40, 2**32 - NP + 33]
_PAIR_REF = {}


def pair_reference(efl, kp, base):
    """The per-key walks' limbs (efl_pl_tune(16, 5, 1)) and the oracle's hex at the checked elements,
    made once a counter base and shared by the tail modes."""
    if base not in _PAIR_REF:
        m = plaintexts(NP, 7).cuda()
        with tune(efl, 16, 5, 1):
            ref = run(kp, m, A, base)
        idx = sorted({NP - 1} | {c - base for c in (2**32 - 1, 2**32, 2**32 + 1)})
        _PAIR_REF[base] = (m, ref, idx, oracle_at(K1024, 10, A, base, idx), oracle_at(K1024, 10, A, base, idx, m.cpu()))
    return _PAIR_REF[base]


@pytest.mark.parametrize("tail", [0, 1, 4])
@pytest.mark.parametrize("base", PAIR_BASES, ids=["carry-in-whole-wave", "carry-in-tail"])
def test_paired_lane_crt_kernels_carry(efl, pair_owner, base, tail):
    """The key owner's paired-lane CRT kernels (1024-bit key, group size 10, efl_pl_tune(16, 5, 2)) at
    32,768 + 65 elements: whole waves (the rounds of 1,024 SIMDs), a tail of 65 elements and a
    part-empty last wave. Tail mode efl_pl_tune(16, 6, .) 0 runs k_crt_pair_mixed (tree waves and
    whole waves in one launch), 4 k_crt_pair_whole + k_crt_pair_tree<., 4>, 1 k_crt_pair_whole +
    k_crt_pair_part + k_crt_pair_tjoin; each draws a with draw_a<1> at ctr0 + el. Counter base
    2^32 - 40 puts the carry inside a whole wave, 2^32 - N + 33 inside the tail. Bit-equal to the
    per-key walks (mode 1) on every element's limbs, and to the oracle at the three elements around
    the carry and the last one."""
    m, ref, idx, want_f, want_c = pair_reference(efl, pair_owner, base)
    assert idx[0] > 0 and idx[-1] == NP - 1 and (idx[0] < 64) == (base == PAIR_BASES[0])
    assert base != PAIR_BASES[1] or idx[0] >= 32768
    with tune(efl, 16, 5, 2), tune(efl, 16, 6, tail):
        got = run(pair_owner, m, A, base)
    for r, o, name in zip(ref, got, ("fbpowm", "encrypt")):
        bad = torch.nonzero((r != o).any(dim=1)).reshape(-1).tolist()
        assert not bad, (name, "elements", bad[:8])
    assert hex_at(efl, pair_owner, got[0], idx) == want_f
    assert hex_at(efl, pair_owner, got[1], idx) == want_c


def test_mixed_hsa_rows_draw_their_own_counter_past_2_32(efl):
    """encrypt with some hsa given and some "0" (as test_paillier_gpu.test_mixed_hsa_never_reuses_a)
    under seed A with counter_base = 2^32 - 5 over 40 rows: the rows with hsa == "0" are re-run in
    runs of consecutive rows at counter_base + row (512-bit key owner without a CRT class: the n^2
    path, k_encrypt28<32, 1>), so they equal the oracle at that counter on both sides of the carry;
    the rows with a given hsa keep it."""
    k = K512
    kp = efl.paillier.Keypair(seed=A)
    kp.set_keys_ints(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, 1, int(k["p"], 16), int(k["q"], 16),
                     table_window=W)
    assert kp.seed == A
    rows = 40
    base = 2**32 - 5
    zero_rows = [0, 1, 2, 4, 5, 6, 7, 20, 21, 39]          # runs that end before, straddle and follow the carry
    given = kp.fbpowm(a=[12345 + i for i in range(rows)]).to_hex().strings()
    hsa = ["0" if i in zero_rows else given[i] for i in range(rows)]
    got = kp.encrypt(torch.zeros(rows, dtype=torch.int64), hsa=hsa, counter_base=base).tensor.to_hex().strings()
    want = oracle_at(k, 1, A, base, zero_rows)
    for i in range(rows):
        if i in zero_rows:
            assert got[i] == want[zero_rows.index(i)], i     # m = 0: the ciphertext is hs^(a') itself
        else:
            assert got[i] == given[i], i
    assert len(set(got)) == rows
