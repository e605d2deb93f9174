#!/usr/bin/env python3
"""Writes tests/golden/mmh3_kat.json: known answers of MurmurHash3_x86_32 as the reference's
`mmh3.hash` gives it (signed), of the bucket ids built on it (xfl/data/functions.py:37-46) and of
CheckSum chains (xfl/data/check_sum.py).

The hash below is written from the public algorithm (Austin Appleby's public-domain MurmurHash3) in
plain Python integers, independent of csrc/mmh3.h. The `mmh3` module is not needed: the script refuses
to write unless it reproduces SMHasher's verification value 0xB0F57EE3 and the published vectors.

    python tests/golden/make_mmh3_golden.py
"""
import json
import os
import random

M32 = 0xFFFFFFFF


def rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def murmur3_x86_32(data: bytes, seed: int = 0) -> int:
    """Unsigned."""
    h = seed & M32
    n = len(data)
    for o in range(0, n - n % 4, 4):
        k = int.from_bytes(data[o:o + 4], "little")
        k = rotl(k * 0xCC9E2D51 & M32, 15) * 0x1B873593 & M32
        h = (rotl(h ^ k, 13) * 5 + 0xE6546B64) & M32
    tail = data[n - n % 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        h ^= rotl(k * 0xCC9E2D51 & M32, 15) * 0x1B873593 & M32
    h ^= n & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return h


def mmh3_hash(data, seed: int = 0) -> int:
    """mmh3.hash: signed."""
    if isinstance(data, str):
        data = data.encode("utf-8")
    h = murmur3_x86_32(data, seed)
    return h - (1 << 32) if h & 0x80000000 else h


def smhasher_verification() -> int:
    blob = b"".join(murmur3_x86_32(bytes(range(i)), 256 - i).to_bytes(4, "little") for i in range(256))
    return murmur3_x86_32(blob, 0)


PUBLISHED = [  # (input, seed, unsigned hash)
    (b"", 0, 0),
    (b"test", 0, 0xBA6BD213),
    (b"Hello, world!", 0, 0xC0363E43),
    (b"The quick brown fox jumps over the lazy dog", 0, 0x2E4FF723),
    (b"hello", 0, 613153351),
    (b"foo", 0, -156908512 & M32),
    (b"abc", 0, 0xB3DD93FA),
    (b"", 1, 0x514E28B7),
    (b"", 0xFFFFFFFF, 0x81F16F39),
    (b"aaaa", 0x9747B28C, 0x5A97808A),
]


def self_check():
    v = smhasher_verification()
    if v != 0xB0F57EE3:
        raise SystemExit("SMHasher verification value is 0x%08X, not 0xB0F57EE3" % v)
    for data, seed, want in PUBLISHED:
        got = murmur3_x86_32(data, seed)
        if got != want:
            raise SystemExit("%r seed 0x%X: 0x%08X, published 0x%08X" % (data, seed, got, want))
    ids = [str(i) for i in range(4096)]
    hs = [mmh3_hash(i) for i in ids]
    if sum(h < 0 for h in hs) != 2129:
        raise SystemExit("of '0'..'4095' %d hash negative, not 2129" % sum(h < 0 for h in hs))
    sizes = [0] * 64
    for h in hs:
        sizes[h % 64] += 1
    if (min(sizes), max(sizes)) != (46, 79):
        raise SystemExit("bucket sizes at 64 buckets run %d..%d, not 46..79" % (min(sizes), max(sizes)))


def check_sum_chain(values, seed=0):
    """The value after every add, CheckSum.add being cur = mmh3.hash(str(cur).encode() + value)."""
    cur, out = seed, []
    for v in values:
        cur = mmh3_hash(str(cur).encode("utf-8") + v)
        out.append(cur)
    return out


def main():
    self_check()
    rng = random.Random(0x6D6D6833)
    hashes = [{"hex": d.hex(), "seed": s, "hash": mmh3_hash(d, s)} for d, s, _ in PUBLISHED]
    # every length 0..67 (every tail length after every block count), bytes >= 0x80 included
    for n in range(68):
        d = bytes(rng.randrange(256) for _ in range(n))
        for s in (0, 1, 0xFFFFFFFF, 0x9747B28C):
            hashes.append({"hex": d.hex(), "seed": s, "hash": mmh3_hash(d, s)})
    # a byte >= 0x80 in every tail position
    for n in (1, 2, 3, 5, 6, 7):
        for pos in range(n - n % 4, n):
            d = bytearray(b"a" * n)
            d[pos] = 0x80 + pos
            hashes.append({"hex": bytes(d).hex(), "seed": 0, "hash": mmh3_hash(bytes(d))})
    utf8 = "你好, wörld"
    hashes.append({"hex": utf8.encode("utf-8").hex(), "seed": 0, "hash": mmh3_hash(utf8), "text": utf8})

    ids = [str(i) for i in range(4096)]
    decimal_hashes = [mmh3_hash(i) for i in ids]
    buckets = []
    for bucket_num in (1, 2, 3, 64, 1000, 4096):
        for c in (1, 2, 3):
            sample = [ids[i] for i in range(0, 4096, 97)]
            buckets.append({"bucket_num": bucket_num, "client2multiserver": c, "ids": sample,
                            "keys": [(mmh3_hash(i) % (bucket_num * c)) // c for i in sample],
                            "local": [mmh3_hash(i) % c for i in sample]})

    chains = []
    for name, values, seed in (
            ("decimal ids", [i.encode() for i in ids[:40]], 0),
            ("empty values", [b"", b"", b"x", b""], 0),
            ("binary rows", [bytes(rng.randrange(256) for _ in range(32)) for _ in range(24)], 0),
            ("short rows", [bytes(rng.randrange(256) for _ in range(8)) for _ in range(24)], 0),
            ("seeded", [b"a", b"bc", b"def"], 12345),
            ("negative seed", [b"a", b"bc", b"def"], -2147483648),
            ("mixed lengths", [bytes(rng.randrange(256) for _ in range(n)) for n in range(20)], 0)):
        chain = check_sum_chain(values, seed)
        chains.append({"name": name, "seed": seed, "values": [v.hex() for v in values], "chain": chain})
    if not any(c < 0 for ch in chains for c in ch["chain"][:-1]):
        raise SystemExit("no chain's running value goes negative")

    out = {"source": "tests/golden/make_mmh3_golden.py (pure Python, from the public algorithm)",
           "smhasher_verification": "0x%08X" % smhasher_verification(),
           "hashes": hashes,
           "decimal_ids": {"count": 4096, "negative": sum(h < 0 for h in decimal_hashes), "hashes": decimal_hashes},
           "buckets": buckets, "check_sums": chains}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mmh3_kat.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, len(hashes), "hashes,", len(buckets), "bucket cases,", len(chains), "chains")


if __name__ == "__main__":
    main()
