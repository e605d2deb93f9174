"""Stage P over the whole operand domain. A ciphertext operand is hex text from a peer, parsed into
2 ln words, so the kernels see any integer below T = 2^(64 ln): non-units (0, n, multiples of p or
q), values at or above n^2 up to T - 1 — everything the reference hands to mpz_mul / mpz_mod /
mpz_powm / mpz_invert, which are total. Every op, every kernel family and every known-answer key
runs the labelled operand list of tests/operand_domain.py (tests/test_operand_domain_host.py checks
that list on the CPU) and must equal the Python-int oracle bit for bit; there is no tolerance.
The padded limb classes run the same list in tests/test_paillier_key_sizes_gpu.py."""
import glob
import os

import pytest
import torch

from operand_domain import first_mismatch, operands, rotate, tile
from oracle import paillier as P
from test_paillier_gpu import ALL, family, fams, ids, keypair
from test_paillier_scalar_gpu import okeypair

pytestmark = pytest.mark.gpu

_MEMO = {}


def memo(key, fn):
    """Oracle values do not depend on the kernel family: computed once per key and case."""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@pytest.fixture(scope="module")
def efl():
    import efl as _efl
    _efl.lib.require_gpu()
    return _efl


def domain(k):
    """(okp, operand list, batch size) of a known-answer key: 70 elements cross a wave for every
    lanes-per-element choice (24 for the 4096-bit key, as tests/test_paillier_scalar_gpu.py)."""
    def make():
        okp = okeypair(k)
        ops = operands(okp.n, okp.p, okp.q, k["n_bytes"] // 2)
        return okp, ops, (70 if k["n_bytes"] < 512 else 24)
    okp, ops, count = memo((k["n_bytes"], "domain"), make)
    assert len(ops) <= count
    return okp, ops, count


def hexes(efl, xs, shape=None):
    return efl.HexTensor.from_ints(xs, shape)


def check(got, want, ops, what):
    msg = first_mismatch(got, want, ops)
    assert not msg, f"{what}: {msg}"


@pytest.mark.parametrize("k,c", fams(ALL))
def test_add(efl, k, c):
    """x y mod n^2 with both operands from the list: rotations 1, 5 and 11 pair every class with
    others (unreduced x unreduced among them), rotation 0 squares each (T-1 x T-1), and one valid
    ciphertext broadcasts against the list."""
    okp, ops, count = domain(k)
    kp = keypair(efl, k, private=False)
    xs = [o.x for o in tile(ops, count)]
    base = [o.x for o in ops]
    ct = int(k["vectors"][3]["c"], 16)
    with family(k["n_bytes"] // 4, False, c):
        for r in (0, 1, 5, 11):
            ys = tile(rotate(base, r), count)
            got = kp.add(hexes(efl, xs), hexes(efl, ys)).to_hex().to_ints()
            want = memo((k["n_bytes"], "add", r), lambda: [P.add(okp, x, y) for x, y in zip(xs, ys)])
            check(got, want, ops, f"add, y rotated by {r}")
        got = kp.add(hexes(efl, xs), hexes(efl, [ct])).to_hex().to_ints()
        check(got, [P.add(okp, x, ct) for x in xs], ops, "add, valid ciphertext")


SCALARS = [0, 1, 2, 3, 2**40 + 1]
HEX_SCALAR = "FFFFFFFFFFFFFFFFFFFF"
NEG_SCALARS = [-1, -7, -2**63]


@pytest.mark.parametrize("k,c", fams(ALL))
def test_mul_scalar(efl, k, c):
    """x^y mod n^2: non-negative int64 scalars and a hex scalar over the whole list; negative
    scalars (the route through x^-1) over the units, reduced or not; a non-unit with a negative
    scalar, reduced or not, is the reference's error for the smallest such element."""
    okp, ops, count = domain(k)
    kp = keypair(efl, k, private=False)
    xs = [o.x for o in tile(ops, count)]
    units = [o for o in ops if o.unit]
    us = [o.x for o in tile(units, count)]
    by = {o.label: o.x for o in ops}
    with family(k["n_bytes"] // 4, False, c):
        for y in SCALARS:
            got = kp.mul_scalar(hexes(efl, xs), torch.tensor(y)).to_hex().to_ints()
            want = memo((k["n_bytes"], "scalar", y), lambda: [P.mul_scalar(okp, x, y) for x in xs])
            check(got, want, ops, f"mul_scalar {y}")
        got = kp.mul_scalar(hexes(efl, xs), HEX_SCALAR).to_hex().to_ints()
        want = memo((k["n_bytes"], "scalar", HEX_SCALAR), lambda: [P.mul_scalar_hex(okp, x, HEX_SCALAR) for x in xs])
        check(got, want, ops, "mul_scalar hex text")
        for y in NEG_SCALARS:
            got = kp.mul_scalar(hexes(efl, us), torch.tensor(y)).to_hex().to_ints()
            want = memo((k["n_bytes"], "scalar", y), lambda: [P.mul_scalar(okp, x, y) for x in us])
            check(got, want, units, f"mul_scalar {y} over the units")
        got = kp.mul_scalar(hexes(efl, us), "-7").to_hex().to_ints()
        check(got, _MEMO[(k["n_bytes"], "scalar", -7)], units, "mul_scalar hex text -7 over the units")
        for bad_x, at in ((by["M+n"], 3), (by["M"], 7), (by["n"], 0), (by["0"], 12)):
            batch = list(us)
            batch[at] = bad_x
            batch[at + 6] = by["M+n"]
            with pytest.raises(efl.errors.InvalidArgumentError, match=f"element {at} has no inverse"):
                kp.mul_scalar(hexes(efl, batch), torch.tensor(-3))
            with pytest.raises(efl.errors.InvalidArgumentError, match=f"element {at} has no inverse"):
                kp.mul_scalar(hexes(efl, batch), "-3")
            # the same batch with the scalar positive needs no inverse
            got = kp.mul_scalar(hexes(efl, batch), torch.tensor(3)).to_hex().to_ints()
            assert got == [pow(x, 3, okp.n2) for x in batch]


@pytest.mark.parametrize("k,c", fams(ALL))
def test_mul_exp2(efl, k, c):
    """x^(2^y) mod n^2; shift 0 gives x mod n^2 (include/efl_hip.h), also for x at or above n^2."""
    okp, ops, count = domain(k)
    kp = keypair(efl, k, private=False)
    xs = [o.x for o in tile(ops, count)]
    with family(k["n_bytes"] // 4, False, c):
        for y in (0, 1, 5, 33):
            got = kp.mul_exp2(hexes(efl, xs), torch.tensor(y)).to_hex().to_ints()
            want = memo((k["n_bytes"], "exp2", y), lambda: [P.mul_exp2(okp, x, y) for x in xs])
            check(got, want, ops, f"mul_exp2 {y}")
            if y == 0:
                assert want == [x % okp.n2 for x in xs]


@pytest.mark.parametrize("k,c", fams(ALL))
def test_shift_add(efl, k, c):
    """FixedPointTensor.__add__'s ciphertext half (efl_pl_fxp_add), x from the list, y rotated."""
    okp, ops, count = domain(k)
    kp = keypair(efl, k, private=False)
    xs = [o.x for o in tile(ops, count)]
    ys = tile(rotate([o.x for o in ops], 5), count)
    with family(k["n_bytes"] // 4, False, c):
        for xe, ye in ((0, 0), (5, 0), (0, 7), (70, 2)):
            z, ze = kp.shift_add(hexes(efl, xs), torch.tensor(xe), hexes(efl, ys), torch.tensor(ye))
            want = memo((k["n_bytes"], "fxp", xe, ye),
                        lambda: [P.fixedpoint_add(okp, x, xe, y, ye)[0] for x, y in zip(xs, ys)])
            check(z.to_hex().to_ints(), want, ops, f"shift_add ({xe}, {ye})")
            assert ze.cpu().tolist() == [min(xe, ye)] * count


@pytest.mark.parametrize("k", ALL, ids=ids)
def test_invert(efl, k):
    """k_invert starts Pornin's GCD from a = x as given: every unit, reduced or not, gives
    pow(x, -1, n^2); a batch with an unreduced non-unit at index 5 and a 0 at index 9 reports 5
    through the raw ABI with both rows zeroed, and the wrapper raises for it (the shape of
    test_unblind_reports_first_blind_number_without_inverse in tests/test_rsa_gpu.py)."""
    from efl.privacy import paillier_cipher as pc
    okp, ops, count = domain(k)
    kp = keypair(efl, k, private=False)
    units = [o for o in ops if o.unit]
    assert sum(not o.reduced for o in units) >= 3
    us = [o.x for o in tile(units, count)]
    got = kp.invert(hexes(efl, us)).to_hex().to_ints()
    check(got, [P.invert(okp, x) for x in us], units, "invert")
    by = {o.label: o.x for o in ops}
    batch = list(us)
    batch[5], batch[9] = by["M+n"], 0
    key = kp.key
    x = kp._cipher(hexes(efl, batch))
    out = torch.full_like(x.limbs, -1)
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert pc._lib.efl_pl_invert(*key.args(), x.limbs.data_ptr(), out.data_ptr(), len(batch), bad.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream) == 0
    assert int(bad.item()) == 5
    rows = pc.CipherTensor(out, (len(batch),), key).to_hex().to_ints()
    assert rows[5] == 0 and rows[9] == 0
    assert [r for i, r in enumerate(rows) if i not in (5, 9)] == \
        [P.invert(okp, v) for i, v in enumerate(batch) if i not in (5, 9)]
    with pytest.raises(efl.errors.InvalidArgumentError, match="element 5 has no inverse"):
        kp.invert(hexes(efl, batch))


MM_XE = [[0, 2, 1], [3, 0, 5]]
MM_YE = [[0, 1], [2, 0], [1, 3]]
MM_POS = [[2, 1], [0, 3], [4, 1]]          # every term's class reaches some output
MM_ALONE = [[2, 1], [0, 3], [0, 1]]        # output (0, 0) is x_00^2 alone
MM_MIXED = [[3, -2], [-1, 0], [5, -7]]


def _chunks6(xs):
    """2 x 3 matrices that together hold every value of xs (the last one wraps round)."""
    return [[[xs[(i + j) % len(xs)] for j in range(3)], [xs[(i + 3 + j) % len(xs)] for j in range(3)]]
            for i in range(0, len(xs), 6)]


def _matmul_cases(k):
    okp, ops, _ = domain(k)
    by = {o.label: o.x for o in ops}
    cases = [(f"list[{6 * i}:]", xm, MM_POS) for i, xm in enumerate(_chunks6([o.x for o in ops]))]
    # x = n with y = 2 alone in its output (the product is 0 mod n^2), x = 0, x = M + 1, x = T - 1
    cases.append(("n^2 alone", [[by["n"], 1, by["M+1"]], [by["T-1"], 0, by["M+1"]]], MM_ALONE))
    cases.append(("M alone", [[by["M"], by["2"], by["M+n"]], [by["n(n-1)"], by["p^2"], by["T-1"]]], MM_ALONE))
    cases += [(f"units[{6 * i}:]", xm, MM_MIXED) for i, xm in enumerate(_chunks6([o.x for o in ops if o.unit]))]
    out = []
    for name, xm, ym in cases:
        want = memo((k["n_bytes"], "matmul", name), lambda: P.matmul(okp, xm, MM_XE, ym, MM_YE))
        out.append((name, xm, ym, want))
    zero_outputs = sum(z == 0 for _, _, _, (zm, _) in out for row in zm for z in row)
    assert zero_outputs >= 4
    return out


@pytest.mark.parametrize("k,c", fams(ALL))
def test_matmul(efl, k, c):
    """PaillierMatmul, u = 2, v = 3, w = 2, over the list: every class in some term with y >= 0
    (z_pos returned as it stands: a product of 0 mod n^2 must read "0", through the single-split
    store and through k_matcomb28), units only with mixed signs (the finish inverts z_neg). Term
    splits 0 (chosen), 1 and 2 (efl_pl_tune(ln, 3, .)), and the per-term composition
    (_matmul_composed) on the same inputs."""
    lib = efl.lib.raw()
    ln = k["n_bytes"] // 4
    kp = keypair(efl, k, private=False)
    xe, ye = torch.tensor(MM_XE), torch.tensor(MM_YE)
    cases = _matmul_cases(k)
    with family(ln, False, c):
        for s in (0, 1, 2):
            prev = lib.efl_pl_tune(ln, 3, s)
            try:
                for name, xm, ym, (wm, we) in cases:
                    x = hexes(efl, [v for row in xm for v in row], (2, 3))
                    zm, ze = kp.matmul(x, xe, torch.tensor(ym), ye)
                    assert ze.cpu().tolist() == we, (name, s)
                    got, want = zm.to_hex().strings(), [P.hx(v) for row in wm for v in row]
                    assert got == want, f"matmul {name}, splits {s}: output " \
                        f"{next(i for i in range(4) if got[i] != want[i])}: got {got} want {want}"
            finally:
                lib.efl_pl_tune(ln, 3, prev)
        for name, xm, ym, (wm, we) in cases:
            x = kp._cipher(hexes(efl, [v for row in xm for v in row], (2, 3)))
            zm, ze = kp._matmul_composed(x, xe.cuda(), torch.tensor(ym).cuda(), ye.cuda())
            assert ze.cpu().tolist() == we, name
            assert zm.to_hex().strings() == [P.hx(v) for row in wm for v in row], f"composed matmul {name}"


@pytest.mark.parametrize("k,c", fams(ALL))
def test_encrypt_given_hsa(efl, k, c):
    """c = g(m) hsa mod n^2 for hsa as a peer may send it: T - 1, M + 1, n, M (text non-zero,
    product 0) and 1, against every sign and size of m."""
    okp, ops, _ = domain(k)
    by = {o.label: o.x for o in ops}
    kp = keypair(efl, k, private=False)
    pairs = [(m, by[h]) for h in ("T-1", "M+1", "n", "M", "1") for m in (0, 5, -5, 2**63 - 1, -2**63)]
    with family(k["n_bytes"] // 4, False, c):
        ct = kp.encrypt(torch.tensor([m for m, _ in pairs]), hsa=hexes(efl, [h for _, h in pairs]))
    got = ct.tensor.to_hex().strings()
    want = [P.hx(P.encrypt(okp, m, h)) for m, h in pairs]
    assert got == want, next((i, pairs[i][0]) for i in range(len(pairs)) if got[i] != want[i])
    assert want[15:20] == ["0"] * 5


@pytest.mark.parametrize("method", [1, 0])
@pytest.mark.parametrize("k,c", fams(ALL, decrypt=True))
def test_decrypt(efl, k, c, method):
    """Decryption reduces c mod p^2 and mod q^2 first, whatever c's size: unreduced units c + j M
    made from known-answer ciphertexts, the list's units (1, M + 1, M - 1, T - 1, ...) against the
    oracle, both exponentiation methods of the sliced kernels. Units only: the reference's L of a
    non-unit is not a defined result."""
    lib = efl.lib.raw()
    ln = k["n_bytes"] // 4
    okp, ops, count = domain(k)
    M, T = okp.n2, 1 << (16 * k["n_bytes"])
    kp = keypair(efl, k)
    # every known-answer ciphertext that fits once more under T (the 1024-bit key's n^2 is 0.85 T:
    # 5 of its 32 do), lifted by M and by the largest multiple that fits
    lifted = sorted({(int(v["c"], 16) + j * M, v["m"]) for v in k["vectors"]
                     for j in (1, (T - 1 - int(v["c"], 16)) // M) if j and int(v["c"], 16) + j * M < T})
    assert len(lifted) >= 5 and all(M <= x < T for x, _ in lifted)
    units = [o for o in ops if o.unit]
    assert {"1", "M+1", "M-1", "T-1"} <= {o.label for o in units}
    cs = tile([o.x for o in units] + [x for x, _ in lifted], count)
    want = memo((k["n_bytes"], "decrypt"), lambda: [P.decrypt(okp, x) for x in cs])
    assert want[len(units):len(units) + len(lifted)][:count - len(units)] == [m for _, m in lifted][:count - len(units)]
    prev = lib.efl_pl_tune(ln, 2, method)
    try:
        with family(ln, True, c):
            got = kp.decrypt(hexes(efl, cs)).strings()
    finally:
        lib.efl_pl_tune(ln, 2, prev)
    assert got == [P.hx(d) for d in want], next(i for i in range(len(cs)) if got[i] != P.hx(want[i]))


@pytest.mark.parametrize("k", [k for k in ALL if k["n_bytes"] >= 128], ids=ids)
def test_crt_join_unreduced_addends(efl, k):
    """efl_pl_crt_join's rows at and above p^2 and q^2, up to 2^(32 ln) - 1. The join is two plain
    products, a sum s = q^2 yp + p^2 yq and one conditional subtraction of n^2 (include/efl_hip.h):
    exact, s mod n^2, whenever s < 2 n^2 — which unreduced addends can meet — and s - n^2 mod
    2^(64 ln) past that, as the header states. Nothing in the efl package calls the join itself:
    the library feeds it the sub-keys' walk results, which are below p^2 and q^2."""
    from efl.privacy import paillier_cipher as pc
    from test_paillier_crt_gpu import ints, limbs
    kp = keypair(efl, k)
    key = kp.key
    p, q = key.p, key.q
    p2, q2, n2 = p * p, q * q, key.n * key.n
    W = 1 << (32 * key.ln)
    assert p2 < W and q2 < W
    yp = [p2, p2 + 1, 0, p2, p2 - 1, W - 1, W - 1, 0, W - 1, p2 + 5, 1, p2 - 1, p2 + 3, 0, 5]
    yq = [0, 0, q2, q2, q2 + 1, 0, W - 1, W - 1, q2 - 1, q2 + 7, q2 + 1, q2 - 1, 0, q2 + 9, q2]
    period = len(yp)
    yp, yq = tile(yp, 70), tile(yq, 70)
    z = torch.empty((len(yp), key.lc), dtype=torch.int32, device="cuda")
    Yp, Yq = limbs(yp, key.ln), limbs(yq, key.ln)
    assert pc._lib.efl_pl_crt_join(*key.args(), Yp.data_ptr(), Yq.data_ptr(), None, z.data_ptr(), len(yp),
                                   torch.cuda.current_stream().cuda_stream) == 0
    exact = 0
    for i, (a, b, g) in enumerate(zip(yp, yq, ints(z))):
        s = q2 * a + p2 * b
        if s < 2 * n2:
            exact += a >= p2 or b >= q2
            assert g == s % n2, i
        else:
            assert g == (s - n2) % (W * W), i
    assert exact >= 7 * (len(yp) // period)        # unreduced addends inside the exact range
    pkg = os.path.dirname(os.path.abspath(pc.__file__))
    calls = [f for f in glob.glob(os.path.join(os.path.dirname(pkg), "**", "*.py"), recursive=True)
             if "efl_pl_crt_join(" in open(f).read()]
    assert calls == []


def _get_sll(v):
    """mpz_get_sll (gmp_utils.cc:38-45): the low 64 bits of |v|, negated where v < 0, as int64."""
    r = abs(v) & (2**64 - 1)
    if v < 0:
        r = -r & (2**64 - 1)
    return r - 2**64 if r >= 2**63 else r


@pytest.mark.parametrize("k", ALL, ids=ids)
def test_decrypt_int64_beyond_int64(efl, k):
    """decrypt(..., dtype=int64) of plaintexts past 64 bits (efl_pl_to_int64): m scaled by 2^40 + 1
    and by -(2^62) under encryption, |plaintext| >= 2^64, with |m| = 0 mod 2^64 and low bits = 2^63
    among them."""
    kp = keypair(efl, k)
    ms = [2**62 + 12345, -(2**62) - 99, 2**63 - 1, -2**63, 2**24, -(2**24), 4, -4, 6, -6, 2, 3 * 2**61, 2**40 + 7, -1]
    ct = kp.encrypt(torch.tensor(ms))
    saw = set()
    for y in (2**40 + 1, -(2**62)):
        prod = [m * y for m in ms]
        got = kp.decrypt(kp.mul_scalar(ct.tensor, torch.tensor(y)), dtype=torch.int64).cpu().tolist()
        assert got == [_get_sll(v) for v in prod], y
        assert kp.decrypt(kp.mul_scalar(ct.tensor, torch.tensor(y))).strings() == [P.hx(v) for v in prod]
        assert sum(abs(v) >= 2**64 for v in prod) >= 6
        saw |= {abs(v) % 2**64 for v in prod if abs(v) >= 2**64}
    assert 0 in saw and 2**63 in saw
