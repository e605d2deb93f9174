"""CPU: the host side of ECDH PSI (efl.psi.EccSigner). csrc/fe25519.h, the header k_x25519 is
compiled from, is compiled by g++ under ASan and UBSan into a stand-alone program that checks every
field vector and every X25519 vector of tests/golden/x25519_kat.json; the argument checks of
efl_x25519 / efl_x25519_hash (they run before any HIP call); EccSigner's constructor."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, PKG

with open(os.path.join(GOLDEN, "x25519_kat.json")) as _f:
    KAT = json.load(_f)


def all_vectors():
    """[(scalar hex, u hex, out hex)] of the fixture: known answers, every scalar with every u, the
    signed digests."""
    v = [(k["scalar"], k["u"], k["out"]) for k in KAT["known"]]
    for s in KAT["scalars"]:
        v += [(s["scalar"], u, o) for u, o in zip(KAT["us"], s["outs"])]
    v += [(KAT["hash"]["secret"], h["digest"], h["signed"]) for h in KAT["hash"]["vectors"]]
    return v


def test_fixture_has_the_vectors():
    assert os.path.getsize(os.path.join(GOLDEN, "x25519_kat.json")) < 64 * 1024
    names = {k["name"] for k in KAT["known"]}
    assert {"rfc7748-5.2-1", "rfc7748-5.2-2", "rfc7748-6.1-alice-shared", "reference-test"} <= names
    assert next(k for k in KAT["known"] if k["name"] == "rfc7748-5.2-1")["out"].startswith("c3da5537")
    assert KAT["iterated"]["after_1"].startswith("422c8e7a") and KAT["iterated"]["after_1000"].endswith("532c51")
    sc = {s["name"]: s for s in KAT["scalars"]}
    assert len(sc) >= 4 and sc["zeros"]["scalar"] == "00" * 32 and sc["ones"]["scalar"] == "ff" * 32
    assert sc["unclamped"]["scalar"] != sc["clamped-twin"]["scalar"]
    assert sc["unclamped"]["outs"] == sc["clamped-twin"]["outs"]
    p = 2 ** 255 - 19
    us = [int.from_bytes(bytes.fromhex(u), "little") for u in KAT["us"]]
    assert us[:8] == [0, 1, 9, p - 1, p, p + 1, 2 ** 255 - 1, 2 ** 255 + 9]
    for s in KAT["scalars"]:
        assert len(s["outs"]) == len(us) and s["outs"][7] == s["outs"][2] != "00" * 32
        assert all(s["outs"][i] == "00" * 32 for i in (0, 1, 3, 4, 8, 9))
    totals = [len(KAT["hash"]["prefix"]) + len(h["id"]) // 2 for h in KAT["hash"]["vectors"]]
    assert totals == [10, 55, 56, 63, 64, 119, 120]
    assert any(max(bytes.fromhex(h["id"]), default=0) > 127 for h in KAT["hash"]["vectors"])


HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "fe25519.h"
using namespace efl::fe;

struct X { const char *k, *u, *out; };
struct M { const char *a, *b, *sum, *diff, *prod, *sq, *loose, *a24, *inv; };
struct F { uint32_t limbs[10]; const char* out; };
static const X xs[] = {
%(xs)s
};
static const M ms[] = {
%(ms)s
};
static const F fs[] = {
%(fs)s
};

static void unhex(uint8_t b[32], const char* s) {
  for (int i = 0; i < 32; ++i) {
    unsigned v;
    sscanf(s + 2 * i, "%%2x", &v);
    b[i] = (uint8_t)v;
  }
}
static Fe load(const char* s) {
  uint8_t b[32];
  uint32_t w[8];
  Fe h;
  unhex(b, s);
  words_from_bytes(w, b);
  from_words(h, w);
  return h;
}
static int bad = 0;
static void expect(Fe h, const char* want, const char* what, int i) {
  uint8_t b[32], e[32];
  uint32_t w[8];
  freeze(h);
  to_words(w, h);
  bytes_from_words(b, w);
  unhex(e, want);
  if (memcmp(b, e, 32)) {
    printf("MISMATCH %%s %%d\n", what, i);
    ++bad;
  }
}

int main() {
  int i = 0;
  for (const M& m : ms) {
    const Fe a = load(m.a), b = load(m.b);
    Fe s, d, h, t;
    add(s, a, b);
    expect(s, m.sum, "sum", i);
    sub(d, a, b);
    expect(d, m.diff, "diff", i);
    mul(h, a, b);
    expect(h, m.prod, "prod", i);
    sqr(h, a);
    expect(h, m.sq, "sq", i);
    mul(h, s, d);                 // loose operands
    expect(h, m.loose, "loose", i);
    sqr(h, d);
    mul(t, d, d);
    freeze(h);
    freeze(t);
    if (memcmp(h.v, t.v, sizeof h.v)) {
      printf("MISMATCH sqr vs mul of a loose operand %%d\n", i);
      ++bad;
    }
    mul_a24(h, d);
    expect(h, m.a24, "a24", i);
    invert(h, a);
    expect(h, m.inv, "inv", i);
    Fe p = a, q = b;
    cswap(p, q, 0u);
    if (memcmp(p.v, a.v, sizeof a.v) || memcmp(q.v, b.v, sizeof b.v)) ++bad, printf("MISMATCH cswap 0 %%d\n", i);
    cswap(p, q, ~0u);
    if (memcmp(p.v, b.v, sizeof a.v) || memcmp(q.v, a.v, sizeof b.v)) ++bad, printf("MISMATCH cswap 1 %%d\n", i);
    ++i;
  }
  i = 0;
  for (const F& f : fs) {
    Fe h;
    memcpy(h.v, f.limbs, sizeof h.v);
    expect(h, f.out, "freeze", i++);
  }
  i = 0;
  for (const X& x : xs) {
    uint8_t k[32], u[32], e[32], out[32];
    unhex(k, x.k);
    unhex(u, x.u);
    unhex(e, x.out);
    x25519(out, k, u);
    if (memcmp(out, e, 32)) {
      printf("MISMATCH x25519 %%d\n", i);
      ++bad;
    }
    ++i;
  }
  printf("checked %%zu field, %%zu freeze, %%zu x25519 vectors, %%d mismatches\n", sizeof ms / sizeof *ms,
         sizeof fs / sizeof *fs, sizeof xs / sizeof *xs, bad);
  return bad ? 1 : 0;
}
"""


def test_fe25519_header_under_sanitizers(tmp_path):
    """The header the kernel is compiled from, as a host program of its own under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    q = lambda s: '"%s"' % s
    xs = ",\n".join("  {%s, %s, %s}" % (q(k), q(u), q(o)) for k, u, o in all_vectors())
    ms = ",\n".join("  {" + ", ".join(q(m[f]) for f in ("a", "b", "sum", "diff", "prod", "sq", "loose", "a24", "inv")) + "}"
                    for m in KAT["field"]["mul"])
    fs = ",\n".join("  {{%s}, %s}" % (", ".join("%du" % x for x in f["limbs"]), q(f["out"])) for f in KAT["field"]["freeze"])
    src = tmp_path / "fe_host.cpp"
    src.write_text(HOST_MAIN % {"xs": xs, "ms": ms, "fs": fs})
    exe = tmp_path / "fe_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len(all_vectors())
    assert f"{n} x25519 vectors, 0 mismatches" in r.stdout, r.stdout
    assert n >= len(KAT["known"]) + len(KAT["scalars"]) * len(KAT["us"]) + 7


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    P16, P20 = ctypes.c_void_p(16), ctypes.c_void_p(20)
    k = b"\x07" * 32
    # n == 0 is a no-op, before anything else is looked at
    assert lib.efl_x25519(None, None, None, 0, None) == 0
    assert lib.efl_x25519_hash(None, None, 0, None, None, None, 0, None) == 0
    # negative counts, null buffers, a null scalar
    assert lib.efl_x25519(k, P16, P16, -1, None) == -3
    assert "negative" in lib.efl_last_error().decode()
    assert lib.efl_x25519(k, None, P16, 5, None) == -3
    assert "null buffer" in lib.efl_last_error().decode()
    assert lib.efl_x25519(k, P16, None, 5, None) == -3
    assert lib.efl_x25519(None, P16, P16, 5, None) == -3
    assert "scalar" in lib.efl_last_error().decode()
    # rows are 16-byte aligned
    assert lib.efl_x25519(k, P20, P16, 5, None) == -3
    assert "aligned" in lib.efl_last_error().decode()
    assert lib.efl_x25519(k, P16, P20, 5, None) == -3
    h = lib.efl_x25519_hash
    assert h(k, b"curve25519", 10, P16, P16, P16, -1, None) == -3
    assert h(k, b"curve25519", -1, P16, P16, P16, 5, None) == -3
    assert "prefix_len" in lib.efl_last_error().decode()
    assert h(k, b"x" * 65, 65, P16, P16, P16, 5, None) == -3
    assert h(k, None, 3, P16, P16, P16, 5, None) == -3
    assert "null prefix" in lib.efl_last_error().decode()
    assert h(k, b"curve25519", 10, None, P16, P16, 5, None) == -3
    assert h(k, b"curve25519", 10, P16, None, P16, 5, None) == -3
    assert h(k, b"curve25519", 10, P16, P16, None, 5, None) == -3
    assert h(None, b"curve25519", 10, P16, P16, P16, 5, None) == -3
    assert h(k, b"curve25519", 10, P16, P16, P20, 5, None) == -3
    assert "aligned" in lib.efl_last_error().decode()


def test_ecc_signer_constructor_needs_no_gpu():
    import efl
    assert efl.psi.EccSigner is efl.psi.ecc_signer.EccSigner and "EccSigner" in efl.psi.__all__
    for bad in (b"p" * 31, b"p" * 33, "p" * 32, bytearray(b"p" * 32), 5):
        with pytest.raises(TypeError, match="secret must be 32-byte string"):
            efl.psi.EccSigner(bad)
    for hashfunc in (lambda v: None, lambda v: b"a" * 31, lambda v: "a" * 32):
        with pytest.raises(TypeError, match="the return value of hashfunc  must be 32 bytes!"):
            efl.psi.EccSigner(hashfunc=hashfunc)
    seen = []
    s = efl.psi.EccSigner(b"p" * 32, hashfunc=lambda v: seen.append(v) or b"a" * 32)
    assert seen == [b"test"]                      # the reference's probe
    assert efl.psi.EccSigner()._private != efl.psi.EccSigner()._private
    # what needs no launch needs no GPU either
    assert s.sign_list([]) == [] and s.sign_hash_list([]) == []
    with pytest.raises(ValueError, match="item 1 is not a 32-byte string"):
        s.sign_list([b"a" * 32, b"a" * 31])
    from efl.psi import ecc_cipher
    with pytest.raises(efl.errors.InvalidArgumentError, match="32 bytes"):
        ecc_cipher.x25519(b"short", ecc_cipher.rows_from_bytes([b"a" * 32]))
    assert ecc_cipher.bytes_from_rows(ecc_cipher.rows_from_bytes([b"a" * 32, b"b" * 32])) == [b"a" * 32, b"b" * 32]
