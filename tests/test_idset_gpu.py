"""GPU: efl.psi.IdStore (csrc/idset.hip) against a Python dict over `bytes`, the reference's store
(efls-data/xfl/data/store/sample_kv_store.py). Everything is exact equality: positions, the order of
keys(), sizes, existence, values. One row runs per lane in 256-lane blocks, so 63 / 64 / 65 sit around
a wave, 257 past a block and 2049 past eight of them; the winners' ranks cross blocks from 257 on."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (8, 32)
SIZES = (1, 63, 64, 65, 257, 2049)


@pytest.fixture(scope="module")
def psi():
    import efl
    return efl.psi


def rows_of(items, width):
    return torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).reshape(len(items), width)


def bytes_of(t):
    raw = t.detach().cpu().contiguous().numpy().tobytes()
    w = t.shape[1]
    return [raw[i:i + w] for i in range(0, len(raw), w)]


def random_keys(rng, n, width, space=None):
    """n rows; with `space` they are drawn from that many distinct rows (duplicates on purpose)."""
    if space is None:
        return [rng.getrandbits(8 * width).to_bytes(width, "little") for _ in range(n)]
    pool = [rng.getrandbits(8 * width).to_bytes(width, "little") for _ in range(space)]
    return [pool[rng.randrange(space)] for _ in range(n)]


class Dict(object):
    """The reference's DictSampleKvStore with positions: what every IdStore answer is checked against."""

    def __init__(self):
        self.d, self.pos = {}, {}

    def put(self, keys, values=None):
        out = []
        for i, k in enumerate(keys):
            if k not in self.pos:
                self.pos[k] = len(self.pos)
            self.d[k] = self.pos[k] if values is None else values[i]
            out.append(self.pos[k])
        return out

    def find(self, keys):
        return [self.pos.get(k, -1) for k in keys]


def check_against(store, ref, width, probe):
    """keys() order, values(), size(), and find / exists / get of `probe` (present and absent rows)."""
    assert store.size() == len(ref.pos)
    assert bytes_of(store.keys()) == list(ref.pos) and store.keys().is_cuda
    assert store.values().tolist() == [ref.d[k] for k in ref.pos]
    want = ref.find(probe)
    dev = rows_of(probe, width).cuda()
    assert store.find(dev).tolist() == want
    assert store.exists(dev).tolist() == [p >= 0 for p in want]
    found, vals = store.get(dev)
    assert found.tolist() == [p >= 0 for p in want]
    assert vals.tolist() == [ref.d.get(k, -1) for k in probe]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", WIDTHS)
def test_parity_with_a_dict(psi, width, n):
    rng = random.Random(1000 * width + n)
    store, ref = psi.IdStore(width=width, capacity=8, seed=rng.getrandbits(64)), Dict()
    absent = random_keys(rng, 64, width)
    # a batch with duplicates inside, then one that overlaps it, then fresh rows only
    first = random_keys(rng, n, width, space=max(1, (2 * n) // 3))
    second = [first[rng.randrange(n)] if rng.random() < 0.5 else k for k in random_keys(rng, n, width)]
    third = random_keys(rng, n, width)
    for batch, with_values in ((first, True), (second, False), (third, True)):
        values = [rng.randrange(-2 ** 63, 2 ** 63) for _ in batch] if with_values else None
        got = store.put_rows(rows_of(batch, width).cuda(), None if values is None else torch.tensor(values).cuda())
        assert got.is_cuda and got.dtype == torch.int64
        assert got.tolist() == ref.put(batch, values)
        check_against(store, ref, width, first + absent + batch)


@pytest.mark.parametrize("width", WIDTHS)
def test_duplicates(psi, width):
    rng = random.Random(width)
    # 300 identical rows: one key at position 0 with the value of row 299
    store = psi.IdStore(width=width, capacity=1024, seed=11)
    k = bytes(range(1, width + 1))
    pos = store.put_rows(rows_of([k] * 300, width).cuda(), torch.arange(5000, 5300).cuda())
    assert pos.tolist() == [0] * 300 and store.size() == 1
    assert bytes_of(store.keys()) == [k] and store.values().tolist() == [5299]
    # the same key in different waves and blocks of one batch: rows 0, 64, 256, 2048
    store, ref = psi.IdStore(width=width, capacity=8192, seed=12), Dict()
    batch = random_keys(rng, 2049, width)
    for i in (64, 256, 2048):
        batch[i] = batch[0]
    batch[2047] = batch[65]                   # and a pair that does not start at row 0
    values = list(range(9000, 9000 + 2049))
    assert store.put_rows(rows_of(batch, width).cuda(), torch.tensor(values).cuda()).tolist() == ref.put(batch, values)
    assert store.size() == 2049 - 4 and ref.d[batch[0]] == 9000 + 2048
    check_against(store, ref, width, batch)
    # a key present from an earlier batch keeps its position and takes the new value
    again = [batch[300], batch[0], batch[300]] + random_keys(rng, 5, width)
    v2 = [-1, -2, -3, 1, 2, 3, 4, 5]
    got = store.put_rows(rows_of(again, width).cuda(), torch.tensor(v2).cuda()).tolist()
    assert got == ref.put(again, v2) and got[:3] == [ref.pos[batch[300]], 0, ref.pos[batch[300]]]
    assert ref.d[batch[300]] == -3 and ref.d[batch[0]] == -2
    check_against(store, ref, width, batch + again)


@pytest.mark.parametrize("width", WIDTHS)
def test_edge_keys(psi, width):
    zero, ones = bytes(width), b"\xff" * width       # EccSigner gives the zero row for low-order points
    base = bytes(range(0x40, 0x40 + width))
    first = bytes([base[0] ^ 1]) + base[1:]
    last = base[:-1] + bytes([base[-1] ^ 0x80])
    batch = [zero, ones, base, first, last, zero, ones, last]
    for seed in (0, 1, 2 ** 64 - 1):
        store, ref = psi.IdStore(width=width, capacity=16, seed=seed), Dict()
        assert store.put_rows(rows_of(batch, width).cuda()).tolist() == ref.put(batch) == [0, 1, 2, 3, 4, 0, 1, 4]
        probes = batch + [bytes([1]) + zero[1:], zero[:-1] + bytes([1]), ones[:-1] + b"\xfe", b"\xfe" + ones[1:],
                          bytes([base[0] ^ 2]) + base[1:], base[:-1] + bytes([base[-1] ^ 1])]
        check_against(store, ref, width, probes)
        assert store.find(rows_of(probes[8:], width).cuda()).tolist() == [-1] * 6


def home_rows(lib, seed, width, capacity, home, count, rng):
    out = []
    while len(out) < count:
        k = rng.getrandbits(8 * width).to_bytes(width, "little")
        if lib.efl_idset_hash(seed, k, width) & (capacity - 1) == home:
            out.append(k)
    return out


@pytest.mark.parametrize("width", WIDTHS)
def test_chains_wrap_around_the_end_of_the_table(psi, width):
    """20 rows whose home is the last slot and 10 whose home is the one before: the chains run over
    the table's end into its first slots."""
    import efl
    lib = efl.lib.raw()
    rng, seed = random.Random(63 + width), 0x5EED
    store, ref = psi.IdStore(width=width, capacity=64, seed=seed), Dict()
    at63 = home_rows(lib, seed, width, 64, 63, 40, rng)
    at62 = home_rows(lib, seed, width, 64, 62, 20, rng)
    batch = at63[:7] + at62[:10] + at63[7:20]
    assert store.put_rows(rows_of(batch[:12], width).cuda()).tolist() == ref.put(batch[:12])
    assert store.put_rows(rows_of(batch[12:], width).cuda()).tolist() == ref.put(batch[12:])
    assert store.capacity == 64 and store.size() == 30
    slots = (store._slots.cpu().to(torch.int64) & 0xFFFFFFFF).tolist()
    used = [i for i, s in enumerate(slots) if s != 0xFFFFFFFF]
    assert used == list(range(0, 28)) + [62, 63]           # one chain from 62 over the end to 27
    assert sorted(slots[i] for i in used) == list(range(30))
    check_against(store, ref, width, batch + at63[20:] + at62[10:])
    assert store.find(rows_of(at63[20:] + at62[10:], width).cuda()).tolist() == [-1] * 30


@pytest.mark.parametrize("width", WIDTHS)
def test_growth(psi, width):
    rng = random.Random(5000 + width)
    store, ref = psi.IdStore(width=width, capacity=8, seed=99), Dict()
    keys = random_keys(rng, 5000, width)
    absent = rows_of(random_keys(rng, 1000, width), width).cuda()
    done = []
    for o in range(0, 5000, 257):
        batch = keys[o:o + 257]
        assert store.put_rows(rows_of(batch, width).cuda()).tolist() == ref.put(batch)
        done += batch
        assert store.find(rows_of(done, width).cuda()).tolist() == ref.find(done)
        assert not bool(store.exists(absent).any())
    assert store.size() == 5000 and store.capacity == 16384 and bytes_of(store.keys()) == keys
    assert store.values().tolist() == list(range(5000))
    # batches of known keys do not make the table grow: the size is read back instead
    for _ in range(4):
        store.put_rows(rows_of(keys[:3000], width).cuda())
    assert store.capacity == 16384 and store.size() == 5000


@pytest.mark.parametrize("width", WIDTHS)
def test_determinism_and_independence_of_the_seed(psi, width):
    rng = random.Random(77 + width)
    batches = [random_keys(rng, n, width, space=400) for n in (300, 2049, 65)]
    values = [torch.tensor([rng.randrange(-2 ** 40, 2 ** 40) for _ in b]) for b in batches]
    results = []
    for seed in (5, 5, 6, 2 ** 63 + 1):
        store = psi.IdStore(width=width, capacity=8, seed=seed)
        pos = [store.put_rows(rows_of(b, width).cuda(), v.cuda()).cpu() for b, v in zip(batches, values)]
        results.append((store.keys().cpu(), store.values().cpu(), torch.cat(pos)))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)


def test_forms(psi):
    rng = random.Random(3)
    keys = random_keys(rng, 5000, 32)
    store, ref = psi.IdStore(seed=1), Dict()
    # host rows in, host positions out; the rows are not written
    host = rows_of(keys[:100], 32)
    before = host.clone()
    pos = store.put_rows(host, torch.arange(100))
    assert not pos.is_cuda and pos.tolist() == ref.put(keys[:100], list(range(100))) and torch.equal(host, before)
    assert not store.find(host).is_cuda and not store.exists(host).is_cuda
    found, vals = store.get(host)
    assert not found.is_cuda and not vals.is_cuda and vals.tolist() == list(range(100))
    # a misaligned view (rows 1 byte into a buffer) and a strided one (every second row)
    flat = torch.zeros(32 * 50 + 1, dtype=torch.uint8)
    flat[1:] = rows_of(keys[100:150], 32).reshape(-1)
    shifted = flat.cuda()[1:].view(50, 32)
    assert shifted.data_ptr() % 16 == 1
    assert store.put_rows(shifted).tolist() == ref.put(keys[100:150])
    strided = rows_of(keys[90:190], 32).cuda()[::2]
    assert not strided.is_contiguous()
    assert store.put_rows(strided).tolist() == ref.put(keys[90:190:2])
    assert store.find(strided).tolist() == ref.find(keys[90:190:2])
    wide = torch.zeros((40, 48), dtype=torch.uint8)
    wide[:, 8:40] = rows_of(keys[200:240], 32)
    assert store.put_rows(wide.cuda()[:, 8:40]).tolist() == ref.put(keys[200:240])
    check_against(store, ref, 32, keys[:260])
    # the list-of-bytes forms of the reference
    assert store.put(keys[300], 41) is True and store.put(keys[300:303], [1, 2, 3]) is True
    ref.put([keys[300]], [41])
    ref.put(keys[300:303], [1, 2, 3])
    assert store.exists(keys[298:304]) == [False, False, True, True, True, False]
    assert store.get(keys[301]) == 2 and store.get(keys[299]) is None
    check_against(store, ref, 32, keys[:310])
    # clear, then reuse
    store.clear()
    assert store.size() == 0 and tuple(store.keys().shape) == (0, 32)
    assert not bool(store.exists(rows_of(keys[:310], 32).cuda()).any())
    ref = Dict()
    assert store.put_rows(rows_of(keys, 32).cuda()).tolist() == ref.put(keys)
    check_against(store, ref, 32, keys[:64])
    # iter_batches yields keys() in order
    batches = list(store.iter_batches(2048))
    assert [b.shape[0] for b in batches] == [2048, 2048, 904]
    assert torch.equal(torch.cat(batches), store.keys()) and bytes_of(torch.cat(batches)) == keys
    # width 8 through the list forms
    small = psi.IdStore(width=8, capacity=8)
    assert small.put([b"abcdefgh", b"ABCDEFGH", b"abcdefgh"], [1, 2, 3])
    assert small.exists([b"abcdefgh", b"abcdefgH"]) == [True, False] and small.get(b"abcdefgh") == 3
    assert small.size() == 2


@pytest.mark.parametrize("width", WIDTHS)
def test_through_the_c_abi(width):
    """insert, find and rehash on caller-owned buffers, a torch device scalar as the size counter."""
    import efl
    lib = efl.lib.raw()
    rng = random.Random(width)
    keys = random_keys(rng, 600, width)
    batch = keys[:300] + keys[:100]
    rows = rows_of(batch, width).cuda()
    cap, seed = 1024, 0xABCDEF
    table = torch.empty((512, width), dtype=torch.uint8, device="cuda")
    slots = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    size = torch.zeros((), dtype=torch.int64, device="cuda")
    pos = torch.full((400,), -7, dtype=torch.int64, device="cuda")
    nbytes = lib.efl_idset_scratch_bytes(400)
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    assert rows.data_ptr() % 16 == 0 and table.data_ptr() % 16 == 0
    args = (table.data_ptr(), 512, size.data_ptr())
    assert lib.efl_idset_insert(rows.data_ptr(), 400, width, *args, 0, slots.data_ptr(), cap, seed, pos.data_ptr(),
                                scratch.data_ptr(), nbytes, None) == 0, lib.efl_last_error()
    torch.cuda.synchronize()
    assert int(size) == 300 and pos.tolist() == list(range(300)) + list(range(100))
    assert bytes_of(table[:300]) == keys[:300]
    # a second batch against a size_bound above the true size
    rows2 = rows_of(keys[250:350], width).cuda()
    pos2 = torch.empty(100, dtype=torch.int64, device="cuda")
    assert lib.efl_idset_insert(rows2.data_ptr(), 100, width, *args, 400, slots.data_ptr(), cap, seed,
                                pos2.data_ptr(), scratch.data_ptr(), nbytes, None) == 0, lib.efl_last_error()
    torch.cuda.synchronize()
    assert int(size) == 350 and pos2.tolist() == list(range(250, 350))
    # too small a table for the bound is refused and nothing is written
    assert lib.efl_idset_insert(rows2.data_ptr(), 100, width, *args, 450, slots.data_ptr(), cap, seed,
                                pos2.data_ptr(), scratch.data_ptr(), nbytes, None) == -3
    assert "below twice" in lib.efl_last_error().decode()
    # find: present, absent
    probe = rows_of(keys[340:360], width).cuda()
    out = torch.empty(20, dtype=torch.int64, device="cuda")
    assert lib.efl_idset_find(probe.data_ptr(), 20, width, table.data_ptr(), slots.data_ptr(), cap, seed,
                              out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == list(range(340, 350)) + [-1] * 10
    # rehash into a larger slot array under another seed; the old slots stay as they were
    old = slots.clone()
    slots2 = torch.zeros(4096, dtype=torch.int32, device="cuda")
    assert lib.efl_idset_rehash(table.data_ptr(), width, size.data_ptr(), 400, slots2.data_ptr(), 4096, seed + 1,
                                None) == 0
    allp = rows_of(keys, width).cuda()
    out = torch.empty(600, dtype=torch.int64, device="cuda")
    assert lib.efl_idset_find(allp.data_ptr(), 600, width, table.data_ptr(), slots2.data_ptr(), 4096, seed + 1,
                              out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == list(range(350)) + [-1] * 250 and torch.equal(slots, old)
    assert int((slots2 != -1).sum()) == 350
    table2 = slots2.tolist()
    for i in range(350):                    # a key sits in the chain that starts at its home slot
        at = lib.efl_idset_hash(seed + 1, keys[i], width) & 4095
        while table2[at] not in (i, -1):
            at = (at + 1) & 4095
        assert table2[at] == i
    # misaligned rows are refused
    assert lib.efl_idset_find(probe.data_ptr() + 4, 1, width, table.data_ptr(), slots.data_ptr(), cap, seed,
                              out.data_ptr(), None) == -3
    assert "aligned" in lib.efl_last_error().decode()
