"""CPU: X25519 over its whole u, scalar, output and limb domain (tests/x25519_domain.py).

The exact-integer model of csrc/fe25519.h's limb arithmetic is checked at the class maxima (which
covers the classes: a column is a sum of products of limbs and every carry is monotone in the column
it leaves), the Python reference is tied to the OpenSSL-checked digests of
tests/golden/x25519_domain.json and to the existing known answers, and the header itself runs as a
stand-alone g++ program under ASan and UBSan with FE_AUDIT defined to a checker that aborts on a limb
outside the class its site states: mul, sqr and mul_a24 over family F limb for limb against the
model, add / sub and ladder_step at the tight extremes, freeze on arbitrary limbs, invert, and
x25519() over all of U, K and W.
"""
import hashlib
import json
import math
import os
import random
import shutil
import struct
import subprocess

import pytest

import x25519_domain as xd
from conftest import GOLDEN, PKG

P = xd.P


# ---- the model ----------------------------------------------------------------------------------
def test_model_holds_at_the_class_maxima():
    loose, tight = list(xd.LOOSE), list(xd.TIGHT)
    assert loose[0] == 3 * 2 ** 26 - 1 and loose[1] == 3 * 2 ** 25 + 2 ** 16 - 1
    assert tight[0] == 2 ** 26 - 1 and tight[1] == 2 ** 25 + 2 ** 16 - 1
    # the columns (their asserts: none reaches 2^64, no 19 f, 2 f or 4 f reaches 2^32), largest first
    mc, sc, ac = xd.mul_columns(loose, loose), xd.sqr_columns(loose), xd.a24_columns(loose)
    assert mc == sc                                    # a square of the maximum is the product's columns
    assert max(mc) == mc[0] and round(math.log2(mc[0]), 2) == 62.13 and mc[0] < 2 ** 63
    assert round(math.log2(mc[9]), 2) == 57.49         # the column whose carry is multiplied by 19
    assert max(ac) < 2 ** 45
    assert 19 * loose[0] < 2 ** 32 and 4 * loose[1] < 2 ** 32 and 19 * loose[1] < 2 ** 32
    # columns are monotone in every limb: the maximum's columns bound any vector's of the class
    rng = random.Random(1)
    fam = xd.family_f("loose")
    for f in fam[1:21] + rng.sample(fam, 40):
        g = rng.choice(fam)
        assert all(a <= b for a, b in zip(xd.mul_columns(f, g), mc))
        assert all(a <= b for a, b in zip(xd.sqr_columns(f), sc))
    # the carry's proved bounds for those columns: tight, and more than tight
    for cols in (mc, sc, ac):
        b = xd.carry_bounds(cols)
        assert all(x <= m for x, m in zip(b, xd.CARRY_MAX)), b
    assert tuple(xd.carry_bounds(mc)) == xd.CARRY_MAX
    assert xd.in_class(xd.CARRY_MAX, "tight")
    assert xd.CARRY_MAX[1] < 2 ** 25 + 2 ** 11 and xd.CARRY_MAX[5] < 2 ** 25 + 2 ** 11
    # what the comment used to promise does not hold: ten columns just below 2^63 leave limb 1
    # outside the tight class (limb 5 above the old 2^25 + 2^11 too); below 2^62 they stay inside
    worst = xd.carry([2 ** 63 - 1] * 10)
    assert worst[1] == 2 ** 25 + 77823 and worst[5] == 2 ** 25 + 4095
    assert not xd.in_class(worst, "tight")
    assert xd.in_class(xd.carry_bounds([2 ** 62] * 10), "tight")
    # add and sub: tight operands give loose limbs, and sub never wraps
    assert xd.in_class([a + b for a, b in zip(tight, tight)], "loose")
    assert xd.in_class(xd.sub_model(tight, [0] * 10), "loose")
    assert xd.in_class(xd.sub_model([0] * 10, tight), "loose")
    assert xd.limbs_value(xd.sub_model([0] * 10, [0] * 10)) == 2 * P


def test_model_computes_the_field():
    rng = random.Random(2)
    pairs = xd.field_pairs()
    for f, g in pairs[:40] + rng.sample(pairs, 200):
        h = xd.mul_model(f, g)
        assert xd.in_class(h, "tight") and xd.limbs_value(h) % P == xd.limbs_value(f) * xd.limbs_value(g) % P
        s = xd.sqr_model(f)
        assert s == xd.mul_model(f, f) and xd.limbs_value(s) % P == xd.limbs_value(f) ** 2 % P
        assert xd.limbs_value(xd.a24_model(g)) % P == xd.A24 * xd.limbs_value(g) % P
    for v in (0, 1, P - 1, P, 2 ** 255 - 1):
        assert xd.limbs_value(xd.limbs_of(v)) == v and xd.in_class(xd.limbs_of(v), "tight")


# ---- the families and the fixture ---------------------------------------------------------------
def test_families_have_their_rows():
    us = xd.family_u()
    assert 740 <= len(us) <= 760
    kinds = {k: [v for kk, _, v in us if kk == k] for k in {k for k, _, _ in us}}
    assert sorted(kinds["p+small"])[:19] == [P + j for j in range(19)]
    assert max(kinds["p+small"]) == 2 ** 256 - 1                          # p + 18 with bit 255
    assert len(kinds["bit"]) == len(kinds["all-but-bit"]) == 255 and len(kinds["limb"]) == 20
    assert kinds["even-limbs"][0] + kinds["odd-limbs"][0] == 2 ** 255 - 1
    assert all(xd.on_curve(u) for u in kinds["curve"]) and not any(xd.on_curve(u) for u in kinds["twist"])
    assert len(kinds["curve"]) == len(kinds["twist"]) == 64
    ks = xd.family_k()
    assert 516 <= len(ks) <= 524 and len({k for _, _, k in ks}) == len(ks)
    assert xd.on_curve(9) and not xd.on_curve(int.from_bytes(xd.k_points()[1], "little"))
    assert len(xd.w_candidates()) == xd.load_fixture()["candidates"]
    for cls in ("tight", "loose"):
        f = xd.family_f(cls)
        assert len(f) == 4021 and all(xd.in_class(v, cls) for v in f) and f[0] == list(xd.CLASS_MAX[cls])


def test_reference_reproduces_the_fixture():
    fx = xd.load_fixture()
    assert os.path.getsize(xd.FIXTURE) < 64 * 1024
    assert fx["seed"] == xd.SEED and fx["u_scalars"] == [k.hex() for k in xd.U_SCALARS]
    assert fx["w_scalars"] == [k.hex() for k in xd.W_SCALARS] and fx["lane_scalar"] == xd.LANE_SCALAR.hex()
    assert fx["k_points"] == [u.hex() for u in xd.k_points()]
    per_class = {cls: [w for c, w in xd.family_w() if c == cls] for cls in ("curve", "twist")}
    xd.check_w_conditions(per_class)
    assert len(per_class["curve"]) == 102 and len(per_class["twist"]) == 212
    assert set(xd.w_candidates()) >= {w for _, w in xd.family_w()}
    for cls, w in xd.family_w()[::16]:                 # the generator filtered every one
        assert xd.prime_order_class(w) == cls
    assert xd.digests() == fx["digests"]
    # the low-order rows are zero, a non-canonical u is its residue, bit 255 is ignored
    for rows in xd.expected_u():
        by = {(k, a, u >> 255): r for (k, a, u), r in zip(xd.family_u(), rows)}
        for j in range(19):
            assert by["small", j, 0] == by["small", j, 1] == by["p+small", j, 0] == by["p+small", j, 1]
            assert any(by["small", j, 0]) == (j > 1)
        assert all(not any(r) for (k, _, _), r in by.items() if k == "low-order")
    # and the existing known answers
    with open(os.path.join(GOLDEN, "x25519_kat.json")) as f:
        kat = json.load(f)
    for k in kat["known"]:
        assert xd.x25519(bytes.fromhex(k["scalar"]), bytes.fromhex(k["u"])).hex() == k["out"], k["name"]
    for s in kat["scalars"]:
        assert [xd.x25519(bytes.fromhex(s["scalar"]), bytes.fromhex(u)).hex() for u in kat["us"]] == s["outs"]


# ---- the header as a host program ---------------------------------------------------------------
HOST_MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace efl { namespace fe { struct Fe; } }
static void fe_audit(int site, const efl::fe::Fe& h, int cls);
#define FE_AUDIT(site, fe, cls) fe_audit(site, fe, cls)
#include "fe25519.h"
using namespace efl::fe;

static const uint32_t kClassMax[2][2] = {{(1u << 26) - 1, (1u << 25) + (1u << 16) - 1},
                                         {3 * (1u << 26) - 1, 3 * (1u << 25) + (1u << 16) - 1}};
static const char* const kSiteName[kAuditSites] = {"mul_f", "mul_g", "sqr_f", "a24_f", "sub_f", "sub_g", "carry_h"};
static uint32_t site_max[kAuditSites][10];
static unsigned long long site_calls[kAuditSites];

static void fe_audit(int site, const Fe& h, int cls) {
  ++site_calls[site];
  for (int i = 0; i < 10; ++i) {
    if (h.v[i] > kClassMax[cls == kLoose][i & 1]) {
      printf("AUDIT %s: limb %d = %u is outside the %s class\n", kSiteName[site], i, h.v[i],
             cls == kLoose ? "loose" : "tight");
      fflush(stdout);
      abort();
    }
    if (h.v[i] > site_max[site][i]) site_max[site][i] = h.v[i];
  }
}

static int bad = 0;
static std::vector<uint32_t> data;
static size_t at = 0;
static const uint32_t* take(size_t n) {
  if (at + n > data.size()) {
    printf("the vector file is short\n");
    exit(2);
  }
  at += n;
  return data.data() + at - n;
}
static Fe fe_of(const uint32_t* p) {
  Fe h;
  memcpy(h.v, p, sizeof h.v);
  return h;
}
static bool in_class(const Fe& h, int cls) {
  for (int i = 0; i < 10; ++i)
    if (h.v[i] > kClassMax[cls == kLoose][i & 1]) return false;
  return true;
}
static void fail(const char* what, size_t i) {
  if (++bad <= 20) printf("MISMATCH %s %zu\n", what, i);
}
static void limbs_are(const Fe& h, const uint32_t* want, const char* what, size_t i) {
  if (memcmp(h.v, want, sizeof h.v)) fail(what, i);
  if (!in_class(h, kTight)) fail("not tight", i);
}
static void value_is(Fe h, const uint32_t* want, const char* what, size_t i) {
  uint32_t w[8];
  freeze(h);
  to_words(w, h);
  if (memcmp(w, want, sizeof w)) fail(what, i);
}

int main(int argc, char** argv) {
  FILE* fp = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!fp) return 2;
  fseek(fp, 0, SEEK_END);
  data.resize((size_t)ftell(fp) / 4);
  fseek(fp, 0, SEEK_SET);
  if (fread(data.data(), 4, data.size(), fp) != data.size()) return 2;
  fclose(fp);
  const uint32_t* n = take(6);
  const size_t n_field = n[0], n_addsub = n[1], n_step = n[2], n_freeze = n[3], n_inv = n[4], n_x = n[5];

  for (size_t i = 0; i < n_field; ++i) {
    const Fe f = fe_of(take(10)), g = fe_of(take(10));
    const uint32_t *m = take(10), *s = take(10), *a = take(10), *mv = take(8), *sv = take(8), *av = take(8);
    Fe h, t;
    mul(h, f, g);
    limbs_are(h, m, "mul limbs", i);
    value_is(h, mv, "mul value", i);
    sqr(h, f);
    limbs_are(h, s, "sqr limbs", i);
    value_is(h, sv, "sqr value", i);
    mul(t, f, f);
    if (memcmp(h.v, t.v, sizeof h.v)) fail("sqr(f) is not mul(f, f)", i);
    mul_a24(h, g);
    limbs_are(h, a, "a24 limbs", i);
    value_is(h, av, "a24 value", i);
    h = f;                                      // in place, as sqr_n and the ladder call them
    mul(h, h, g);
    limbs_are(h, m, "mul in place", i);
    h = f;
    sqr(h, h);
    limbs_are(h, s, "sqr in place", i);
  }
  for (size_t i = 0; i < n_addsub; ++i) {
    const Fe f = fe_of(take(10)), g = fe_of(take(10));
    const uint32_t *sv = take(8), *dv = take(8);
    Fe h;
    add(h, f, g);
    if (!in_class(h, kLoose)) fail("add not loose", i);
    value_is(h, sv, "add value", i);
    sub(h, f, g);
    if (!in_class(h, kLoose)) fail("sub not loose", i);
    value_is(h, dv, "sub value", i);
  }
  for (size_t i = 0; i < n_step; ++i) {
    const Fe x1 = fe_of(take(10));
    Fe x2 = fe_of(take(10)), z2 = fe_of(take(10)), x3 = fe_of(take(10)), z3 = fe_of(take(10));
    const uint32_t *e0 = take(8), *e1 = take(8), *e2 = take(8), *e3 = take(8);
    ladder_step(x1, x2, z2, x3, z3);
    if (!in_class(x2, kTight) || !in_class(z2, kTight) || !in_class(x3, kTight) || !in_class(z3, kTight))
      fail("ladder_step not tight", i);
    value_is(x2, e0, "ladder_step x2", i);
    value_is(z2, e1, "ladder_step z2", i);
    value_is(x3, e2, "ladder_step x3", i);
    value_is(z3, e3, "ladder_step z3", i);
  }
  for (size_t i = 0; i < n_freeze; ++i) {
    Fe h = fe_of(take(10));
    const uint32_t* want = take(8);
    freeze(h);
    for (int l = 0; l < 10; ++l)
      if (h.v[l] > limb_mask(l)) fail("freeze limb not canonical", i);
    uint32_t w[8];
    to_words(w, h);
    if (memcmp(w, want, sizeof w)) fail("freeze", i);
  }
  for (size_t i = 0; i < n_inv; ++i) {
    const Fe z = fe_of(take(10));
    const uint32_t* want = take(8);
    Fe h;
    invert(h, z);
    if (!in_class(h, kTight)) fail("invert not tight", i);
    value_is(h, want, "invert", i);
  }
  for (size_t i = 0; i < n_x; ++i) {
    const uint8_t* k = reinterpret_cast<const uint8_t*>(take(8));
    const uint8_t* u = reinterpret_cast<const uint8_t*>(take(8));
    const uint8_t* want = reinterpret_cast<const uint8_t*>(take(8));
    uint8_t out[32];
    x25519(out, k, u);
    if (memcmp(out, want, 32)) fail("x25519", i);
  }
  if (at != data.size()) {
    printf("the vector file is long\n");
    return 2;
  }
  for (int s = 0; s < kAuditSites; ++s) {
    uint32_t e = 0, o = 0;
    for (int i = 0; i < 10; ++i) {
      uint32_t& m = (i & 1) ? o : e;
      if (site_max[s][i] > m) m = site_max[s][i];
    }
    printf("site %s calls %llu even %u odd %u limb1 %u limb5 %u\n", kSiteName[s], site_calls[s], e, o, site_max[s][1],
           site_max[s][5]);
  }
  printf("checked %zu field, %zu addsub, %zu step, %zu freeze, %zu invert, %zu x25519 vectors, %d mismatches\n", n_field,
         n_addsub, n_step, n_freeze, n_inv, n_x, bad);
  return bad ? 1 : 0;
}
"""


def words(v: int) -> list:
    return list(struct.unpack("<8I", xd.le(v % P)))


def freeze_vectors() -> list:
    """Whole-uint32 limb vectors: 1,000 random ones, and p - 1 .. p + 1 and 2p - 1 .. 2p + 1 in the
    canonical split (the excess in limb 9) and with limbs borrowed from the limb above."""
    rng = random.Random(xd.SEED + 6)
    out = [[rng.getrandbits(32) for _ in range(10)] for _ in range(1000)]
    out += [[2 ** 32 - 1] * 10, [0] * 10]
    for v in (P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1):
        base = xd.limbs_of(v)
        splits = [base]
        for i in range(9):                      # one borrow: limb i + 1 gives one unit to limb i
            if base[i + 1]:
                s = base[:]
                s[i] += 1 << xd.limb_bits(i)
                s[i + 1] -= 1
                splits.append(s)
        s = base[:]                             # every limb borrows from the one above
        for i in range(9):
            if s[i + 1]:
                s[i] += 1 << xd.limb_bits(i)
                s[i + 1] -= 1
        splits.append(s)
        s = base[:]                             # limb 0 takes as much of limb 1 as 32 bits hold
        take = min(s[1], (2 ** 32 - 1 - s[0]) >> 26)
        s[0] += take << 26
        s[1] -= take
        splits.append(s)
        assert all(xd.limbs_value(s) == v and all(0 <= x < 2 ** 32 for x in s) for s in splits)
        out += splits
    return out


def step_vectors() -> list:
    rng = random.Random(xd.SEED + 7)
    zero, top = [0] * 10, list(xd.TIGHT)
    out = [[top if c >> b & 1 else zero for b in range(5)] for c in range(32)]
    out += [[[rng.randint(0, m) for m in xd.TIGHT] for _ in range(5)] for _ in range(500)]
    return out


def x_vectors() -> list:
    """(k, u, out) over all of U x 2 scalars, K x 2 u values and W x 2 scalars."""
    v = []
    for k, rows in zip(xd.U_SCALARS, xd.expected_u()):
        v += [(k, xd.le(u), r) for (_, _, u), r in zip(xd.family_u(), rows)]
    for (_, _, k), rows in zip(xd.family_k(), xd.expected_k()):
        v += [(k, u, r) for u, r in zip(xd.k_points(), rows)]
    for k, us in zip(xd.W_SCALARS, xd.crafted_w()):
        v += [(k, u, xd.le(w)) for u, (_, w) in zip(us, xd.family_w())]
    return v


def vector_file() -> tuple:
    val = xd.limbs_value
    blob, put = [], lambda ws: blob.extend(ws)
    field, steps, frz, xs = xd.field_pairs(), step_vectors(), freeze_vectors(), x_vectors()
    zero, top = [0] * 10, list(xd.TIGHT)
    addsub = [(zero, top), (top, zero), (top, top), (zero, zero)]
    inv = [xd.limbs_of(0), xd.limbs_of(1), xd.limbs_of(P - 1), list(xd.LOOSE)]
    put([len(field), len(addsub), len(steps), len(frz), len(inv), len(xs)])
    for f, g in field:
        put(f + g + xd.mul_model(f, g) + xd.sqr_model(f) + xd.a24_model(g))
        put(words(val(f) * val(g)) + words(val(f) ** 2) + words(xd.A24 * val(g)))
    for f, g in addsub:
        put(f + g + words(val(f) + val(g)) + words(val(f) - val(g)))
    for s in steps:
        put([x for fe in s for x in fe])
        for r in xd.ladder_step_model(*(val(fe) for fe in s)):
            put(words(r))
    for f in frz:
        put(f + words(val(f)))
    for z in inv:
        put(z + words(pow(val(z), P - 2, P)))
    for k, u, r in xs:
        blob.append(k + u + r)
    head = [x for x in blob if not isinstance(x, bytes)]
    tail = b"".join(x for x in blob if isinstance(x, bytes))
    counts = {"field": len(field), "addsub": len(addsub), "step": len(steps), "freeze": len(frz), "invert": len(inv),
              "x25519": len(xs)}
    return struct.pack("<%dI" % len(head), *head) + tail, counts


def test_fe25519_header_over_the_domain_under_sanitizers(tmp_path):
    """fe25519.h with FE_AUDIT defined, as a host program of its own under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    blob, counts = vector_file()
    assert counts["field"] == 8042 and counts["step"] == 532 and counts["freeze"] >= 1050
    assert counts["x25519"] == 2 * len(xd.family_u()) + 2 * len(xd.family_k()) + 2 * len(xd.family_w())
    vec = tmp_path / "vectors.bin"
    vec.write_bytes(blob)
    src = tmp_path / "fe_domain.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "fe_domain"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    want = "checked %(field)d field, %(addsub)d addsub, %(step)d step, %(freeze)d freeze, %(invert)d invert, " \
           "%(x25519)d x25519 vectors, 0 mismatches" % counts
    assert want in r.stdout, r.stdout
    # the audit saw every site, family F reached the loose maxima at the sites that take loose limbs,
    # the add / sub extremes reached the tight maxima, and carry() stayed inside what the model proves
    site = {}
    for line in r.stdout.splitlines():
        if line.startswith("site "):
            t = line.split()
            site[t[1]] = {t[i]: int(t[i + 1]) for i in range(2, len(t), 2)}
    assert set(site) == {"mul_f", "mul_g", "sqr_f", "a24_f", "sub_f", "sub_g", "carry_h"}
    assert all(s["calls"] > 100000 for s in site.values())
    for name in ("mul_f", "mul_g", "sqr_f", "a24_f"):
        assert (site[name]["even"], site[name]["odd"]) == (xd.LOOSE[0], xd.LOOSE[1]), (name, site[name])
    for name in ("sub_f", "sub_g"):
        assert (site[name]["even"], site[name]["odd"]) == (xd.TIGHT[0], xd.TIGHT[1]), (name, site[name])
    c = site["carry_h"]
    assert c["even"] == 2 ** 26 - 1 and c["odd"] <= xd.CARRY_MAX[1]
    assert 2 ** 25 <= c["limb1"] <= xd.CARRY_MAX[1] and 2 ** 25 <= c["limb5"] <= xd.CARRY_MAX[5]


def test_the_audit_aborts_on_a_limb_outside_its_class(tmp_path):
    """The checker is not vacuous: one limb above the loose maximum at mul's entry ends the program."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    f = list(xd.LOOSE)
    f[3] += 1
    head = [1, 0, 0, 0, 0, 0] + f + list(xd.LOOSE) + [0] * 54
    vec = tmp_path / "vectors.bin"
    vec.write_bytes(struct.pack("<%dI" % len(head), *head))
    src = tmp_path / "fe_domain.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "fe_domain"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True)
    assert r.returncode == -6 and "AUDIT mul_f: limb 3" in r.stdout, (r.returncode, r.stdout)
