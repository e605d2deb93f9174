"""The hex text kernels on their own (efl_hex_lengths, efl_hex_write, efl_hex_parse through
limbs_to_hex / hex_to_limbs): mpz_get_str(..., 16) and mpz_set_str(..., 16) restated as Python's
format(v, "x") and int(s, 16). The other tests only ever hand them near-full-width ciphertexts;
here every limb width, the text lengths around the wave's 64-character stride, numbers whose top
limbs are zero, signs, and the batch sizes around a workgroup's 4 (256 for the lengths) elements."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 8, 63, 64, 65, 512]
BATCHES = [1, 4, 5, 257]


@pytest.fixture(scope="module")
def efl():
    import efl as _efl
    _efl.lib.require_gpu()
    return _efl


def values(L):
    """0, 1, and 2^k - 1, 2^k at every multiple of 4 around 28..36, 252..260 and 508..516 (texts of
    63, 64, 65, 127, 128, 129 characters among them) and at 32 L - 1, where they fit L limbs."""
    ks = [28, 32, 36, 248, 252, 256, 260, 504, 508, 512, 516, 32 * L - 1]
    vs = [0, 1]
    for k in ks:
        for v in ((1 << k) - 1, 1 << k):
            if v < 1 << (32 * L) and v not in vs:
                vs.append(v)
    return vs


def limbs_of(vals, L):
    a = np.stack([np.frombuffer(v.to_bytes(4 * L, "little"), "<u4") for v in vals])
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def ints_of(t):
    return [int.from_bytes(r.tobytes(), "little") for r in t.cpu().numpy().view("<u4")]


def batch(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


def text(v, neg):
    return ("-" if neg and v else "") + format(v, "x")


@pytest.mark.parametrize("L", WIDTHS)
def test_write_lengths_offsets_characters_and_round_trip(efl, L):
    from efl.privacy import paillier_cipher as pc
    vals = values(L)
    if L >= 64:
        lens = {len(format(v, "x")) for v in vals}
        assert {63, 64, 65, 127, 128, 129} <= lens
    for n in BATCHES:
        vs = batch(vals, n) if n > len(vals) else vals[-n:]   # the small batches: the widest values
        x = limbs_of(vs, L)
        flags = [(i // len(vals) + i) % 3 == 0 for i in range(n)]   # a third negative, element 0 among them
        if n == 257:
            assert any(f and v == 0 for f, v in zip(flags, vs))
        neg = torch.tensor(flags, dtype=torch.int8, device="cuda")
        for ng, fl in ((None, [False] * n), (neg, flags)):
            want = [text(v, f) for v, f in zip(vs, fl)]
            lens = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            assert pc._lib.efl_hex_lengths(x.data_ptr(), L, ng.data_ptr() if ng is not None else None,
                                           lens.data_ptr(), n, torch.cuda.current_stream().cuda_stream) == 0
            assert lens.cpu().tolist() == [len(s) for s in want]
            hx = pc.limbs_to_hex(x, ng, (n,))
            assert hx.offs.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
            assert hx.strings() == want
            # and back: magnitude and sign (a negative zero was written as "0")
            mag, sg = pc.hex_to_limbs(hx, L, x.device, signed=True)
            assert ints_of(mag) == vs
            assert sg.cpu().tolist() == [int(f and v != 0) for v, f in zip(vs, fl)]
            if ng is None:
                mag, sg = pc.hex_to_limbs(hx, L, x.device)
                assert sg is None and ints_of(mag) == vs


@pytest.mark.parametrize("L", WIDTHS)
def test_parse_case_leading_zeros_and_width(efl, L):
    from efl.privacy import paillier_cipher as pc
    dev = efl.lib.require_gpu()
    vals = values(L)
    top = vals[-1]                                      # 2^(32 L - 1)
    full = (1 << (32 * L)) - 1
    strs, want = [], []
    for i, v in enumerate(vals + [full, 0xabcdef % (1 << (32 * L)), full - 0xabcdef % (1 << (32 * L))]):
        s = format(v, "x")
        for t in (s.upper(), "".join(ch.upper() if (j + i) % 2 else ch for j, ch in enumerate(s)),
                  "0" + s, "0" * (8 * L - len(s)) + s, "0" * (8 * L - len(s) + 1) + s,
                  "0" * (8 * L + 70 - len(s)) + s):
            strs.append(t)
            want.append(v)
    mag, sg = pc.hex_to_limbs(efl.HexTensor.from_strings(strs), L, dev)
    assert sg is None and ints_of(mag) == want
    mag, sg = pc.hex_to_limbs(efl.HexTensor.from_strings(["-" + s for s in strs]), L, dev, signed=True)
    assert ints_of(mag) == want and sg.cpu().tolist() == [1] * len(strs)
    # one digit too many: accepted while the extra digits are all 0, refused when one is not
    for extra in ("1" + "0" * (8 * L), "1" + format(top, "x").rjust(8 * L, "0"), "f" + "0" * 70 + format(full, "x")):
        rows = ["1", "2", extra, "3"]
        with pytest.raises(efl.errors.InvalidArgumentError, match="element 2 is not a hex integer"):
            pc.hex_to_limbs(efl.HexTensor.from_strings(rows), L, dev)
        with pytest.raises(efl.errors.InvalidArgumentError, match="element 2 is not a hex integer"):
            pc.hex_to_limbs(efl.HexTensor.from_strings(["-" + r for r in rows]), L, dev, signed=True)


@pytest.mark.parametrize("L", [1, 8, 65])
def test_parse_rejections_report_the_smallest_index(efl, L):
    from efl.privacy import paillier_cipher as pc
    dev = efl.lib.require_gpu()
    for bad in ("", "-", "g", "0x1", "12 ", "+1", "--1", "1-", "fffg", "G" + "0" * 70):
        for signed in (False, True):
            with pytest.raises(efl.errors.InvalidArgumentError, match="element 1 is not a hex integer"):
                pc.hex_to_limbs(efl.HexTensor.from_strings(["1", bad, "2"]), L, dev, signed=signed)
    rows = ["a"] * 300
    for i in (299, 200, 7, 6, 130):     # several bad rows, in several workgroups: the smallest is reported
        rows[i] = "zz"
    with pytest.raises(efl.errors.InvalidArgumentError, match="element 6 is not a hex integer"):
        pc.hex_to_limbs(efl.HexTensor.from_strings(rows), L, dev)
    rows[3] = ""
    with pytest.raises(efl.errors.InvalidArgumentError, match="element 3 is not a hex integer"):
        pc.hex_to_limbs(efl.HexTensor.from_strings(rows), L, dev, signed=True)


@pytest.mark.parametrize("L", [1, 8, 65])
def test_parse_signs(efl, L):
    """A signed parse gives magnitude and flag. An unsigned parse (a ciphertext operand) keeps no
    sign, so a negative text is refused rather than read as its magnitude; -0...0 is 0 either way."""
    from efl.privacy import paillier_cipher as pc
    dev = efl.lib.require_gpu()
    strs = ["-0", "-000", "0", "-" + "0" * (8 * L + 3), "5", "-5", "-" + "f" * (8 * L), "-00a"]
    mags = [0, 0, 0, 0, 5, 5, (1 << (32 * L)) - 1, 10]
    mag, sg = pc.hex_to_limbs(efl.HexTensor.from_strings(strs), L, dev, signed=True)
    assert ints_of(mag) == mags and sg.cpu().tolist() == [1, 1, 0, 1, 0, 1, 1, 1]
    mag, sg = pc.hex_to_limbs(efl.HexTensor.from_strings(strs[:5]), L, dev)
    assert sg is None and ints_of(mag) == mags[:5]
    for i in (5, 6, 7):
        rows = strs[:5] + ["7"] * 3
        rows[i] = strs[i]
        with pytest.raises(efl.errors.InvalidArgumentError, match=f"element {i} is not a hex integer"):
            pc.hex_to_limbs(efl.HexTensor.from_strings(rows), L, dev)


def test_negative_ciphertext_text_is_refused_by_every_op(efl):
    """The reference computes with -5 (mpz_mod brings it into range); no op of its own ever writes
    a negative ciphertext. Dropping the sign would compute with 5, silently; the build refuses the
    element instead. Signed consumers (mul_scalar's string scalars) are unchanged."""
    import json
    import os
    from conftest import GOLDEN
    from oracle import paillier as P
    with open(os.path.join(GOLDEN, "paillier_kat.json")) as f:
        k = json.load(f)["keys"][0]
    kp = efl.paillier.Keypair(seed=3)
    kp.set_keys_ints(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, 1, int(k["p"], 16), int(k["q"], 16))
    okp = P.Keypair(int(k["n"], 16), int(k["hs"], 16), k["a_bits"] // 8, 1)
    good, neg = ["7", "-0", "9"], ["7", "9", "-5"]
    err = efl.errors.InvalidArgumentError
    one = torch.tensor([1, 1, 1])
    for call in (lambda x: kp.add(x, good), lambda x: kp.add(good, x), lambda x: kp.mul_scalar(x, one),
                 lambda x: kp.mul_exp2(x, one), lambda x: kp.invert(x), lambda x: kp.decrypt(x),
                 lambda x: kp.shift_add(x, one, good, one), lambda x: kp.encrypt(one, hsa=x),
                 lambda x: kp.matmul(efl.HexTensor.from_strings(x, (1, 3)), one.reshape(1, 3), one.reshape(3, 1),
                                     one.reshape(3, 1))):
        with pytest.raises(err, match="element 2 is not a hex integer"):
            call(neg)
    assert kp.add(good, good).to_hex().to_ints() == [49, 0, 81]
    assert kp.mul_scalar(good, ["-1", "-0", "-2"]).to_hex().to_ints() == \
        [P.mul_scalar(okp, 7, -1), 1, P.mul_scalar(okp, 9, -2)]
