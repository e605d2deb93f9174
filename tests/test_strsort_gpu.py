"""GPU: the sort join's order on the device (efl.psi.strsort). efl_strings_sort's `order` exactly equal
to sorted(range(n), key=(segment, field 1, field 0, row)), stated with Python's own bytes order
(strsort_pool.py), at the sizes around the wave, the tile of 2,048 rows, a run count that is no power
of two and several tiles, in both modes, without segments, with one, with 64 (some empty, negative
numbers) and with one per row, over strings from the pool of traps and random strings that start at
odd offsets; byte-identical from run to run; efl_strings_search and efl_strings_run_heads against
their definitions; sort_keys against sorted(keys, key=cmp_to_key(..))."""
import functools

import numpy as np
import pytest
import torch

from strsort_pool import POOL, draw, expected_order, pack, random_keys

pytestmark = pytest.mark.gpu

TILE = 2048                                   # csrc/strsort.h kTile
SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE, 5 * TILE + 7)


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


@functools.lru_cache(maxsize=None)
def keys_of(n):
    return tuple(draw(np.random.default_rng(1000 + n), n))


def segments_of(n):
    """(name, int32 [n] or None): no segments, one, 64 with some empty and negative numbers, one per row."""
    rng = np.random.default_rng(2000 + n)
    used = np.array([s for s in range(-32, 32) if s % 5], dtype=np.int32)          # 13 of the 64 stay empty
    return (("none", None), ("one", np.full(n, 7, dtype=np.int32)), ("64", used[rng.integers(0, len(used), size=n)]),
            ("per row", (np.arange(n, dtype=np.int32)[::-1] - n // 2).copy()))


def device_order(psi, keys, segment, mode, lead=1):
    chars, offsets = pack(keys, lead)
    order = psi.sort_rows(torch.from_numpy(chars), torch.from_numpy(offsets),
                          None if segment is None else torch.from_numpy(segment), mode)
    assert order.is_cuda and order.dtype == torch.int64 and tuple(order.shape) == (len(keys),)
    return order


@pytest.mark.parametrize("mode", ("bytes", "record"))
@pytest.mark.parametrize("n", SIZES)
def test_order_is_exactly_the_expectation(psi, n, mode):
    keys = list(keys_of(n))
    for name, segment in segments_of(n):
        got = device_order(psi, keys, segment, mode, lead=1 + n % 3).tolist()
        assert sorted(got) == list(range(n)), (n, mode, name, "not a permutation")
        assert got == expected_order(keys, segment, mode), (n, mode, name)


@pytest.mark.parametrize("mode", ("bytes", "record"))
def test_pool_sorted_reversed_and_all_equal(psi, mode):
    assert device_order(psi, POOL, None, mode).tolist() == expected_order(POOL, None, mode)
    n = 2 * TILE + 100
    keys = [b"id%06d#%010d" % (i, i) for i in range(n)]
    assert device_order(psi, keys, None, mode).tolist() == list(range(n))
    assert device_order(psi, keys[::-1], None, mode).tolist() == list(range(n))[::-1]
    assert device_order(psi, [b"same#key"] * n, None, mode).tolist() == list(range(n))
    # every key shares its first 16 bytes with every other: the prefix decides nothing
    keys = [b"0123456789abcdef%05d#0123456789abcdef%05d" % ((i * 7919) % n, (i * 104729) % n) for i in range(n)]
    assert device_order(psi, keys, None, mode).tolist() == expected_order(keys, None, mode)


def test_three_runs_give_the_same_bytes(psi):
    n = 5 * TILE + 7
    keys = list(keys_of(n))
    segment = segments_of(n)[2][1]
    for mode in ("bytes", "record"):
        runs = [device_order(psi, keys, segment, mode).cpu().numpy().tobytes() for _ in range(3)]
        assert runs[0] == runs[1] == runs[2]


def test_sort_keys_is_sorted_with_record_cmp(psi):
    rng = np.random.default_rng(3)
    keys = draw(rng, 3000, record=True)

    def cmp(left, right):
        a, b = left.split(b"#"), right.split(b"#")
        return (a[1] > b[1]) - (a[1] < b[1]) or (a[0] > b[0]) - (a[0] < b[0])
    assert psi.sort_keys(keys) == sorted(keys, key=functools.cmp_to_key(cmp))
    assert psi.sort_keys(keys, mode="bytes") == sorted(keys)
    assert psi.sort_keys([b"x#9", b"x#10", b"x#100"]) == [b"x#10", b"x#100", b"x#9"]
    assert psi.sort_keys([b"a#1"]) == [b"a#1"]


def test_empty_input(psi):
    empty = torch.zeros(1, dtype=torch.int64)
    none = torch.zeros(0, dtype=torch.uint8)
    assert tuple(psi.sort_rows(none, empty).shape) == (0,)
    assert tuple(psi.run_heads(none, empty, torch.zeros(0, dtype=torch.int64)).shape) == (0,)
    assert tuple(psi.search_rows(none, empty, torch.zeros(0, dtype=torch.int64), none, empty).shape) == (0,)


TABLE_SIZES = tuple(sorted({0, 1, 2} | {2 ** k + d for k in range(1, 13) for d in (-1, 1)}))


@pytest.mark.parametrize("with_empty", (False, True))
def test_search_rows(psi, with_empty):
    """Present keys (a table with duplicates answers with the lowest row), absent ones below and above
    every key, a proper prefix of a present key, a present key plus one byte, the empty string."""
    assert TABLE_SIZES[:6] == (0, 1, 2, 3, 5, 7) and TABLE_SIZES[-1] == 4097
    rng = np.random.default_rng(40 + with_empty)
    for m in TABLE_SIZES:
        table = [k for k in draw(rng, 2 * m + 8) if k and not k.startswith(b"\x00")][:m]
        assert len(table) == m
        if m > 2:
            table[m // 2] = table[0]                              # a duplicate: row 0 is the answer
        if with_empty and m:
            table[int(rng.integers(0, m))] = b""
            if m > 2:
                table[m - 1] = b""                                # twice
        t_chars, t_offsets = (torch.from_numpy(a) for a in pack(table, 1))
        t_order = psi.sort_rows(t_chars, t_offsets, None, "bytes")
        assert t_order.tolist() == expected_order(table, None, "bytes")
        queries = table + [b"", b"\x00", b"\xff" * 50] + [k[:-1] for k in table[:300]] + [k + b"\x00" for k in table[:300]] + \
            [k + b"a" for k in table[:100]]
        first = {}
        for r, k in enumerate(table):
            first.setdefault(k, r)
        want = [first.get(q, -1) for q in queries]
        if m > 2:
            assert len(first) < m                                 # the table has duplicates
        q_chars, q_offsets = (torch.from_numpy(a) for a in pack(queries, 3))
        got = psi.search_rows(t_chars, t_offsets, t_order, q_chars, q_offsets)
        assert got.is_cuda and got.dtype == torch.int64
        assert got.tolist() == want, m
        if not with_empty:
            assert want[m] == -1 and want[m + 1] == -1 and want[m + 2] == -1      # below all keys, above all keys


def test_run_heads(psi):
    rng = np.random.default_rng(50)
    for n in (1, 2, 65, TILE + 1, 3 * TILE):
        keys = draw(rng, n)
        chars, offsets = (torch.from_numpy(a) for a in pack(keys, 1))
        order = psi.sort_rows(chars, offsets, None, "bytes")
        heads = psi.run_heads(chars, offsets, order)
        assert heads.is_cuda and heads.dtype == torch.uint8
        o = order.tolist()
        assert heads.tolist() == [int(k == 0 or keys[o[k]] != keys[o[k - 1]]) for k in range(n)]
        assert int(heads.sum()) == len(set(keys))
        # in any order, not only a sorted one
        given = torch.from_numpy(rng.permutation(n))
        g = given.tolist()
        assert psi.run_heads(chars, offsets, given).tolist() == [int(k == 0 or keys[g[k]] != keys[g[k - 1]]) for k in range(n)]
