"""What the sort join's tests share (test_strsort_host.py, test_strsort_gpu.py, test_sort_join_gpu.py):
the pool of byte strings at which a string order goes wrong, and the expectation, stated with Python's
own bytes order and sorted() and nothing of the product."""
import numpy as np

POOL = [
    b"", b"a", b"a\x00", b"a\x00\x00", b"ab", b"abc", b"b",                    # the empty string, prefixes, NULs
    b"abcdefgh", b"abcdefghX", b"abcdefghY", b"abcdefgh\x00",                  # 8 leading bytes shared
    b"abcdefghiJ", b"abcdefghiK",                                              # 9
    b"0123456789abcdefP", b"0123456789abcdefQ", b"0123456789abcdef",           # 16
    b"\x7f", b"\x80", b"\xff", b"\xff\x00", b"a\xffb", b"a\x7fb", b"\x00", b"\x00\x00",   # bytes >= 0x80 compare unsigned
    b"a", b"abc", b"abcdefghX", b"", b"\x80",                                  # duplicates
    b"#", b"##", b"#5", b"id#", b"id#5", b"id#5#x", b"id#5#y#z", b"#5#", b"#a#b",   # empty fields, two and three '#'
    b"x#9", b"x#10", b"x#100", b"y#9", b"y#10", b"w#100", b"x#9",              # the order is lexicographic, not numeric
    b"a#", b"a#\x00", b"a\x00#1", b"a#1", b"\x80#\x80", b"\x7f#\x80", b"\x80#\x7f",
    b"id1#20240101", b"id2#20240101", b"id1#20240102", b"id0#20240102",
    b"k1#12345678", b"k2#12345678", b"k1#123456789", b"k0#1234567890", b"k3#12345678\x00",   # field 1 shares 8, 9 bytes
    b"abcdefgh#12345678", b"abcdefgi#12345678", b"abcdefgh#1234567", b"no hash at all",
]


def fields(key):
    """(field 0, field 1) as split(b'#') gives them; field 1 of a key without '#' is empty."""
    t = key.split(b"#")
    return t[0], (t[1] if len(t) > 1 else b"")


def expected_order(keys, segment=None, mode="record"):
    """The one correct output of the sort: ascending in (segment, key order, row index)."""
    seg = [0] * len(keys) if segment is None else [int(s) for s in segment]
    if mode == "bytes":
        return sorted(range(len(keys)), key=lambda i: (seg[i], keys[i], i))
    return sorted(range(len(keys)), key=lambda i: (seg[i], fields(keys[i])[1], fields(keys[i])[0], i))


def pack(keys, lead=0):
    """(chars uint8, offsets int64 [n + 1]) numpy arrays; `lead` bytes of filler come first, so the
    strings start at odd offsets."""
    offsets = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in keys], out=offsets[1:])
    chars = np.frombuffer(b"\xee" * lead + b"".join(keys) + b"\xee", dtype=np.uint8).copy()
    return chars, offsets + lead


def random_keys(rng, n, record=False):
    """n strings of length 0..40 over a small alphabet (so that prefixes and duplicates happen), with
    '#' among the letters; record=True: every key has a '#'."""
    alphabet = np.frombuffer(b"ab#\x00\xff1", dtype=np.uint8)
    out = []
    for length in rng.integers(0, 41, size=n).tolist():
        k = alphabet[rng.integers(0, len(alphabet), size=length)].tobytes()
        if record and b"#" not in k:
            k = k[:length // 2] + b"#" + k[length // 2:]
        out.append(k)
    return out


def draw(rng, n, record=False):
    """n keys: half drawn from POOL, half random."""
    pool = [k for k in POOL if not record or b"#" in k]
    picks = rng.integers(0, len(pool), size=n).tolist()
    rand = random_keys(rng, n, record)
    return [pool[p] if i % 2 else rand[i] for i, p in enumerate(picks)]
