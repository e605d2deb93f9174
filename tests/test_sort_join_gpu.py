"""GPU: the store and the two sides of the sort join (efl.psi.sort_join). KeyStore against a dict over
3,000 puts with repeats (order, first position and last value, exists and get, growth after a lookup,
clear); SortJoinServer and SortJoinClient at 1, 4 and 64 buckets with client2multiserver 1 and 2 and
batches of 7 and 2,048 against a pure-Python restatement of the reference's flow (a dict store,
sorted() with a cmp_to_key comparator, batches, CheckSum chains through efl.psi.mmh3_hash): the same
(bucket, key) list in the same order, the same per-bucket check sums on both sides, the same
get_final_result batches; the batch join's order, and what the server refuses."""
import functools

import numpy as np
import pytest
import torch

from strsort_pool import draw, pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def efl():
    import efl
    return efl


def tb(v):
    return v if isinstance(v, bytes) else str(v).encode("utf-8")


def cmp(left, right):
    a, b = left.split(b"#"), right.split(b"#")
    return (a[1] > b[1]) - (a[1] < b[1]) or (a[0] > b[0]) - (a[0] < b[0])


# ---- KeyStore ---------------------------------------------------------------------------------------------

def test_key_store_against_a_dict(efl):
    rng = np.random.default_rng(11)
    pool = draw(rng, 1200)
    keys = [pool[i] for i in rng.integers(0, len(pool), size=3000).tolist()]
    store, model = efl.psi.KeyStore(), {}
    assert store.size() == 0 and len(store) == 0 and store.keys() == [] and store.exists([b"a", b""]) == [False, False]
    assert store.get(b"a") is None and store.exists([]) == []
    # one at a time, lists, and packed rows
    for i in range(100):
        assert store.put(keys[i], i) is True
        model[keys[i]] = i
    store.put(keys[100:1500], list(range(100, 1500)))
    model.update(zip(keys[100:1500], range(100, 1500)))
    absent = [k + b"\x01" for k in keys[:200]] + [b"\x01"]

    def check():
        assert store.size() == len(model) == len(store)
        assert store.keys() == list(model) and list(store) == list(model)          # insertion order, first position
        assert store.values() == list(model.values())                              # the last value
        asked = keys[:400] + absent
        assert store.exists(asked) == [k in model for k in asked]
        assert [store.get(k) for k in asked[::37]] == [model.get(k) for k in asked[::37]]
        chars, offsets = (torch.from_numpy(a) for a in pack(asked, 1))
        found, values = store.get((chars, offsets))
        assert found.tolist() == [k in model for k in asked]
        assert values.tolist() == [model.get(k, -1) for k in asked]
        assert store.exists((chars, offsets)).tolist() == [k in model for k in asked]

    check()
    assert len(model) < 1500                                                       # there were repeats
    # growth after a lookup: packed rows, whose offsets need not start at 0
    chars, offsets = pack(keys[1500:3000], 5)
    store.put_rows(torch.from_numpy(chars), torch.from_numpy(offsets), torch.arange(1500, 3000, dtype=torch.int64))
    model.update(zip(keys[1500:3000], range(1500, 3000)))
    check()
    store.put(b"a new key", -5)
    model[b"a new key"] = -5
    check()
    store.clear()
    model.clear()
    assert store.size() == 0 and store.keys() == [] and store.exists(keys[:3]) == [False] * 3
    store.put(keys[5], 1)
    model[keys[5]] = 1
    check()
    with pytest.raises(TypeError):
        store.put("text", 1)


# ---- the join -----------------------------------------------------------------------------------------------

def records(rng, lo, hi, repeats):
    """[(hash column, sort column)]: ids lo .. hi - 1 with a time each, some ids at several times, and
    `repeats` records given twice; hash columns as str, sort columns as int, as a job reads them."""
    recs = [("user%05d" % i, int(1_600_000_000 + (i * 7919) % 5000)) for i in range(lo, hi)]
    recs += [("user%05d" % i, int(1_600_000_000 + (i * 104729) % 97)) for i in range(lo, hi, 9)]
    recs += [recs[i] for i in rng.integers(0, len(recs), size=repeats).tolist()]
    return [recs[i] for i in rng.permutation(len(recs)).tolist()]


def model_join(efl, client, server, bucket_num, c, batch_size, need_sort=True):
    """The reference's flow in plain Python. (res, client check sums, server check sums, final results)."""
    mmh3 = efl.psi.mmh3_hash
    B = bucket_num * c
    stores = [dict() for _ in range(B)]
    for i, (h, s) in enumerate(server):
        stores[mmh3(tb(h)) % B][tb(h) + b"#" + tb(s)] = i
    mine = [dict() for _ in range(B)]
    for i, (h, s) in enumerate(client):
        subtask = (mmh3(tb(h)) % (bucket_num * c)) // c
        mine[subtask * c + mmh3(tb(h)) % c][tb(h) + b"#" + tb(s)] = i
    res, c_sums, s_sums, final = [], [0] * B, [0] * B, [[] for _ in range(B)]
    for b in range(B):
        keys = list(mine[b])
        if need_sort:
            keys = sorted(keys, key=functools.cmp_to_key(cmp))
        for cur in range(0, len(keys), batch_size):
            batch = keys[cur:cur + batch_size]
            hits = [k for k in batch if k in stores[b]]
            final[b].append(hits)
            for k in hits:
                c_sums[b] = mmh3(str(c_sums[b]).encode("utf-8") + k)
                s_sums[b] = mmh3(str(s_sums[b]).encode("utf-8") + k)
                res.append((b, k, mine[b][k]))
    return res, c_sums, s_sums, final


@pytest.fixture(scope="module")
def sets():
    rng = np.random.default_rng(21)
    return records(rng, 0, 2700, 150), records(rng, 1300, 4000, 150)


@pytest.mark.parametrize("batch_size", (7, 2048))
@pytest.mark.parametrize("c", (1, 2))
@pytest.mark.parametrize("bucket_num", (1, 4, 64))
def test_join_against_the_python_flow(efl, sets, bucket_num, c, batch_size):
    client_recs, server_recs = sets
    assert 2900 < len(client_recs) < 3300 and 2900 < len(server_recs) < 3300
    B = bucket_num * c
    want, c_sums, s_sums, final = model_join(efl, client_recs, server_recs, bucket_num, c, batch_size)
    assert len(want) > 1000
    server = efl.psi.SortJoinServer(B)
    server.put_records([h for h, _ in server_recs[:2000]], [s for _, s in server_recs[:2000]])
    server.put_records([h for h, _ in server_recs[2000:]], [s for _, s in server_recs[2000:]])
    server.set_is_ready(True)
    assert server.get_is_ready() is True
    client = efl.psi.SortJoinClient(bucket_num, c, batch_size)
    got = client.join([h for h, _ in client_recs], [s for _, s in client_recs], server)
    assert got == [(b, k) for b, k, _ in want]
    assert [client.get_check_sum(b) for b in range(B)] == c_sums
    assert [server.get_check_sum(b) for b in range(B)] == s_sums
    assert [server.get_final_result(b) for b in range(B)] == final
    assert all(server.is_finished(b) for b in range(B))
    assert all(server.finish_join(b, s_sums[b]) is False for b in range(B))         # a second FinishJoin
    # the server's record numbers count over both put_records calls
    key = tb(server_recs[2500][0]) + b"#" + tb(server_recs[2500][1])
    last = max(i for i, (h, s) in enumerate(server_recs) if tb(h) + b"#" + tb(s) == key)
    assert server.store(efl.psi.mmh3_hash(tb(server_recs[2500][0])) % B).get(key) == last


def test_join_yields_the_last_value_of_a_key(efl, sets):
    client_recs, server_recs = sets
    want, _, _, _ = model_join(efl, client_recs, server_recs, 4, 2, 100)
    server = efl.psi.SortJoinServer(8)
    server.put_records([h for h, _ in server_recs], [s for _, s in server_recs])
    server.set_is_ready(True)
    values = ["record %d" % i for i in range(len(client_recs))]
    got = efl.psi.SortJoinClient(4, 2, 100).join([h for h, _ in client_recs], [s for _, s in client_recs], server, values)
    assert got == [(b, values[i]) for b, _, i in want]


def test_batch_join_keeps_the_order_given(efl, sets):
    client_recs, server_recs = sets
    want, c_sums, _, final = model_join(efl, client_recs, server_recs, 4, 2, 64, need_sort=False)
    server = efl.psi.SortJoinServer(8)
    server.put_records([h for h, _ in server_recs], [s for _, s in server_recs])
    server.set_is_ready(True)
    client = efl.psi.SortJoinClient(4, 2, 64, need_sort=False)
    got = client.join([h for h, _ in client_recs], [s for _, s in client_recs], server)
    assert got == [(b, k) for b, k, _ in want]
    assert [client.get_check_sum(b) for b in range(8)] == c_sums
    assert [server.get_final_result(b) for b in range(8)] == final
    sorted_want, _, _, _ = model_join(efl, client_recs, server_recs, 4, 2, 64)
    assert [w[:2] for w in sorted_want] != got                                       # the order matters


def test_what_the_server_refuses(efl):
    server = efl.psi.SortJoinServer(4)
    server.put_records(["a", "b", b"c"], [1, 2, 3])
    assert server.get_is_ready() is False
    with pytest.raises(efl.errors.UnavailableError):
        server.sync_join([b"a#1"], 0)
    with pytest.raises(efl.errors.UnavailableError):
        server.sync_join([b"a#1"], 9)                                                # not ready comes first
    server.set_is_ready(True)
    for bad in (-1, 4, 9, "1", None):
        with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match, expect 0..3, got"):
            server.sync_join([b"a#1"], bad)
        with pytest.raises(efl.errors.InvalidArgumentError, match="bucket id not match"):
            server.finish_join(bad, 0)
    assert all(server.get_final_result(b) == [] and server.get_check_sum(b) == 0 for b in range(4))   # nothing was looked up
    b = efl.psi.mmh3_hash(b"a") % 4
    assert server.sync_join([b"a#1", b"a#2", b"a"], b) == [True, False, False]
    assert server.get_final_result(b) == [[b"a#1"]]
    assert server.get_check_sum(b) == efl.psi.mmh3_hash(b"0a#1")
    assert server.finish_join(b, 12345) is False                                     # a mismatch does not finish
    assert server.finish_join(b, server.get_check_sum(b)) is True
    assert server.finish_join(b, server.get_check_sum(b)) is False                   # only once


def test_an_altered_check_sum_fails_the_join(efl):
    class Altered(efl.psi.SortJoinClient):
        def _new_check_sum(self):
            return efl.psi.CheckSum(seed=1)

    server = efl.psi.SortJoinServer(2)
    server.put_records(["a", "b", "c"], [1, 2, 3])
    server.set_is_ready(True)
    with pytest.raises(ValueError, match="Join finish error"):
        Altered(2).join(["a", "b", "x"], [1, 2, 3], server)
    # the same join with an honest client finishes: the server's buckets were not closed by the attempt
    server = efl.psi.SortJoinServer(2)
    server.put_records(["a", "b", "c"], [1, 2, 3])
    server.set_is_ready(True)
    got = efl.psi.SortJoinClient(2).join(["a", "b", "x"], [1, 2, 3], server)
    assert sorted(k for _, k in got) == [b"a#1", b"b#2"]
