"""CPU: the host side of the signature tail (efl_rsa_decimal, efl_rsa_oneway). csrc/decimal.h, the
header the kernels are compiled from, is compiled by g++ under ASan and UBSan into a stand-alone
program that converts V(words) (tests/decimal_values.py) for words = 1, 2, 3, 32, 33, 64 and 128
through the same two routines the kernels call (to_chunks over arrays, text_byte for every column of
a right-aligned row) and must print exactly Python's str(v); efl_rsa_decimal_digits; the argument
checks of both entry points (they run before any HIP call); the host twin of the device hash."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

from conftest import PKG
from decimal_values import digits, values

WORDS = (1, 2, 3, 32, 33, 64, 128)

HOST_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "decimal.h"
using namespace efl::decimal;

// a line of the input: "<words> <hex>"; a line of the output: the decimal text, or a complaint
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char line[2048];
  int bad = 0;
  long rows = 0;
  while (fgets(line, sizeof line, f)) {
    int words = 0, at = 0;
    if (sscanf(line, "%d %n", &words, &at) != 1 || words < 1 || words > kMaxWords) return 3;
    std::string hex(line + at);
    while (!hex.empty() && (hex.back() == '\n' || hex.back() == ' ')) hex.pop_back();
    // exactly `words` words and exactly max_chunks(words) chunks: ASan guards both ends
    std::vector<uint32_t> x(words, 0u), chunks(max_chunks(words), 0xDEADBEEFu);
    for (size_t i = 0; i < hex.size(); ++i) {
      const char c = hex[hex.size() - 1 - i];
      const uint32_t nib = c <= '9' ? c - '0' : c - 'a' + 10;
      if (i / 8 >= (size_t)words) return 4;
      x[i / 8] |= nib << (4 * (i % 8));
    }
    int puts_seen = 0;
    uint32_t* xp = x.data();
    uint32_t* cp = chunks.data();
    const int len = to_chunks(
        words, [xp](int j) { return xp[j]; }, [xp](int j, uint32_t v) { xp[j] = v; },
        [cp, &puts_seen](int k, uint32_t c) {
          if (k != puts_seen++ || c >= kChunk) abort();
          cp[k] = c;
        });
    if (puts_seen != max_chunks(words)) { ++bad; printf("row %ld: %d chunks\n", rows, puts_seen); continue; }
    for (int j = 0; j < words; ++j) if (x[j]) { ++bad; printf("row %ld: quotient left\n", rows); }
    // the tight stride, and one that leaves padding left of the last chunk too
    std::string got[2];
    for (int t = 0; t < 2; ++t) {
      const int64_t stride = max_digits(words) + (t ? 9 * 2 + 5 : 0);
      std::string text((size_t)stride, '?');
      for (int64_t col = 0; col < stride; ++col)
        text[(size_t)col] = (char)text_byte(stride, col, max_chunks(words), [cp](int k) { return cp[k]; });
      if (len < 1 || len > max_digits(words)) { ++bad; printf("row %ld: len %d\n", rows, len); break; }
      for (int64_t col = 0; col < stride - len; ++col)
        if (text[(size_t)col] != '0') { ++bad; printf("row %ld: padding\n", rows); break; }
      got[t] = text.substr((size_t)(stride - len));
    }
    if (got[0] != got[1]) { ++bad; printf("row %ld: the strides disagree\n", rows); }
    printf("%s\n", got[0].c_str());
    ++rows;
  }
  fclose(f);
  fprintf(stderr, "decimal host check: %ld rows, %d failures\n", rows, bad);
  return bad ? 1 : 0;
}
"""


def test_decimal_header_under_sanitizers(tmp_path):
    """The header the kernels are compiled from, as a host program of its own under ASan + UBSan."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / "decimal_host.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "decimal_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    want, lines = [], []
    for w in WORDS:
        for v in values(w):
            lines.append(f"{w} {v:x}")
            want.append(str(v))
    inp = tmp_path / "values.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"decimal host check: {len(want)} rows, 0 failures" in r.stderr, r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for i, (g, x) in enumerate(zip(got, want)):
        assert g == x, (i, lines[i][:40])


def test_value_set_covers_the_edges():
    """V(words) holds what its docstring says: every length up to the width's, the SHA-256 block edges."""
    for w in WORDS:
        vs = values(w)
        lens = {len(str(v)) for v in vs}
        assert lens == set(range(1, digits(w) + 1)), w
        assert 0 in vs and 2 ** (32 * w) - 1 in vs and all(0 <= v < 2 ** (32 * w) for v in vs)
    assert {55, 56, 63, 64, 65, 119, 120} <= {len(str(v)) for v in values(32)}
    assert 2900 <= len(values(128)) <= 3200


def test_decimal_digits():
    import efl
    lib = efl.lib.raw()
    for w in range(1, 129):
        assert lib.efl_rsa_decimal_digits(w) == len(str(2 ** (32 * w) - 1)), w
    assert [lib.efl_rsa_decimal_digits(w) for w in (1, 32, 64, 128)] == [10, 309, 617, 1234]
    assert lib.efl_rsa_decimal_digits(0) == 0 and lib.efl_rsa_decimal_digits(129) == 0
    assert lib.efl_rsa_decimal_digits(-1) == 0


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    P = ctypes.c_void_p
    P16 = P(16)
    err = lambda: lib.efl_last_error().decode()

    def decimal(x=P16, words=64, n=5, text=P16, stride=617, len_=P16):
        return lib.efl_rsa_decimal(x, words, n, text, stride, len_, None)

    def oneway(x=P16, words=64, n=5, hash_=1, out=P16):
        return lib.efl_rsa_oneway(x, words, n, hash_, out, None)

    # n == 0 is a no-op, before anything else is looked at
    assert lib.efl_rsa_decimal(None, 0, 0, None, 0, None, None) == 0
    assert lib.efl_rsa_oneway(None, 0, 0, 0, None, None) == 0
    assert decimal(n=-1) == -3 and "negative" in err()
    assert oneway(n=-1) == -3 and "negative" in err()
    # null buffers
    for name in ("x", "text", "len_"):
        assert decimal(**{name: None}) == -3 and "null buffer" in err(), name
    for name in ("x", "out"):
        assert oneway(**{name: None}) == -3 and "null buffer" in err(), name
    # a row has 1 to 128 words
    for w in (0, 129, -1):
        assert decimal(words=w, stride=2000) == -3 and "1 to 128 words" in err(), w
        assert oneway(words=w) == -3 and "1 to 128 words" in err(), w
    # a stride one below the most digits of the width
    for w, d in ((1, 10), (32, 309), (64, 617), (128, 1234)):
        assert decimal(words=w, stride=d - 1) == -3 and "stride" in err(), w
    assert decimal(stride=2 ** 30 + 1) == -3 and "stride" in err()
    # the device has one hash
    for h in (0, 2, -1):
        assert oneway(hash_=h) == -3 and "EFL_ONEWAY_SHA256_64" in err(), h
    # alignment: words and lengths 4 bytes, hash rows 8
    assert decimal(x=P(18)) == -3 and "misaligned" in err()
    assert decimal(len_=P(18)) == -3 and "misaligned" in err()
    assert oneway(out=P(20)) == -3 and "misaligned" in err()
    with pytest.raises(efl.errors.InvalidArgumentError, match="stride"):
        efl.lib.check(decimal(stride=616))


def test_oneway_host_twin_and_text():
    import efl
    rc = efl.psi.rsa_cipher
    assert rc.ONEWAY_HASHES == {"sha256": 1}
    for text in ("0", "1", "12345678901234567890", "9" * 617, "abc", "6.5", ""):
        want = int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "big")
        assert rc.oneway_sha256(text) == want
    assert rc.oneway_sha256("0") == 0x5FECEB66FFC86F38          # sha256(b"0") = 5feceb66ffc86f38...
    assert rc.oneway_text(bytes([0x38, 0x6F, 0xC8, 0xFF, 0x66, 0xEB, 0xEC, 0x5F])) == b"5feceb66ffc86f38"
    # no leading zeros, as hex() writes a number: the reference's hex(v)[2:]
    assert rc.oneway_text(bytes(8)) == b"0" and rc.oneway_text(b"\x0a" + bytes(7)) == b"a"
    assert rc.oneway_text(b"\xff" * 8) == b"f" * 16
    for v in (0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1):
        assert rc.oneway_text(v.to_bytes(8, "little")) == hex(v)[2:].encode()
    with pytest.raises(efl.errors.InvalidArgumentError, match="8 bytes"):
        rc.oneway_text(b"1234567")


def test_signers_take_a_hash_name_without_gpu():
    import efl
    psi = efl.psi
    assert psi.RsaJoinServer is psi.rsa_join.RsaJoinServer and psi.RsaJoinClient is psi.rsa_join.RsaJoinClient
    assert {"RsaJoinServer", "RsaJoinClient", "rsa_join"} <= set(psi.__all__)
    s = psi.RsaSigner(oneway_hash="sha256")
    # items the device does not take go through the host twin on str(item), as a callable would
    t = psi.RsaSigner(oneway_hash=psi.rsa_cipher.oneway_sha256)
    items = ["abc", 6.5, -1, True, 2 ** 4096]
    assert s.oneway_hash_list(items) == t.oneway_hash_list(items)
    assert s.oneway_hash_list([]) == []
    with pytest.raises(efl.errors.InvalidArgumentError, match="sha256"):
        psi.RsaSigner(oneway_hash="md5")
    for bad in (0, -4, 2.5, None):
        with pytest.raises(efl.errors.InvalidArgumentError, match="batch_size"):
            psi.RsaJoinClient(batch_size=bad)
