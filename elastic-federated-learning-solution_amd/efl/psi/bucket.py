"""The bucket hash of the reference's data-join, on the device, with the reference's names.

In efls-data both parties first key every record by `mmh3.hash(id) % bucket_num`
(xfl/data/functions.py:37-46: DefaultKeySelector and get_local_bucket_id; pipelines.py key_by), one
join server runs per bucket, and a client subtask that talks to `client2multiserver` servers splits
its records once more with get_local_bucket_id. Two parties that split their IDs differently find
wrong intersections, so the hash is the reference's: MurmurHash3_x86_32 with mmh3's signed result and
Python's `%` (csrc/mmh3.h).

`mmh3_hash`, `get_local_bucket_id` and `DefaultKeySelector.get_key` are the per-record forms, on the
host. The batched forms keep the IDs on the device, packed as the signers take them
(rsa_cipher.pack_strings): `mmh3_hash_rows`, `bucket_ids`, `DefaultKeySelector.get_keys`,
`partition_rows` (a stable counting sort: the order in which a Flink key_by hands a subtask its
records), `gather_strings`, and `partition`, which packs a list once and does all of it.
"""
from __future__ import annotations

import collections

import torch

from efl import errors
from efl import lib as _efl_lib
from efl.psi.rsa_cipher import pack_strings

_lib = _efl_lib.raw()

MAX_BUCKETS = 4096
MAX_MODULUS = 2 ** 31 - 1


def _key_bytes(key) -> bytes:
    if isinstance(key, str):
        return key.encode("utf-8")
    if isinstance(key, (bytes, bytearray, memoryview)):
        return bytes(key)
    raise TypeError(f"mmh3_hash: key must be str or bytes, not {type(key).__name__}")


def mmh3_hash(key, seed=0) -> int:
    """Drop-in for mmh3.hash(key, seed): the signed 32-bit MurmurHash3_x86_32 of a byte string (a str
    is encoded as UTF-8). A host call."""
    b = _key_bytes(key)
    return int(_lib.efl_mmh3_hash_host(b, len(b), int(seed) & 0xFFFFFFFF))


def get_local_bucket_id(key, local_bucket_num) -> int:
    """xfl/data/functions.py get_local_bucket_id."""
    return mmh3_hash(key) % local_bucket_num


def _packed(chars, offsets, what):
    """(chars, offsets, n) on the device; chars is never a null buffer."""
    chars, offsets = _efl_lib.as_tensor(chars), _efl_lib.as_tensor(offsets)
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise errors.InvalidArgumentError(f"{what}: offsets must be int64 [n + 1]")
    if chars.dtype not in (torch.uint8, torch.int8) or chars.dim() != 1:
        raise errors.InvalidArgumentError(f"{what}: chars must be a vector of bytes")
    home = chars.device if chars.is_cuda else offsets.device
    dev = home if home.type == "cuda" else _efl_lib.require_gpu()
    c = chars.contiguous().to(dev)
    if c.numel() == 0:
        c = torch.zeros(1, dtype=torch.uint8, device=dev)
    return c, offsets.contiguous().to(dev), offsets.numel() - 1


def mmh3_hash_rows(chars, offsets, seed=0) -> torch.Tensor:
    """mmh3.hash(string i, seed) as element i of an int32 device tensor (efl_mmh3_hash), for n byte
    strings packed back to back (chars uint8 / int8, offsets int64 [n + 1]; pack_strings makes them)."""
    c, o, n = _packed(chars, offsets, "mmh3_hash_rows")
    out = torch.empty(n, dtype=torch.int32, device=c.device)
    _efl_lib.check(_lib.efl_mmh3_hash(c.data_ptr(), o.data_ptr(), n, int(seed) & 0xFFFFFFFF, out.data_ptr(),
                                      _efl_lib.stream_handle(c.device)))
    return out


def _int32_rows(t, what):
    t = _efl_lib.as_tensor(t)
    if t.dtype != torch.int32 or t.dim() != 1:
        raise errors.InvalidArgumentError(f"{what}: expected an int32 vector, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous().to(t.device if t.is_cuda else _efl_lib.require_gpu())


def bucket_ids(hashes, modulus, divisor=1) -> torch.Tensor:
    """(hashes[i] % modulus) // divisor with Python's %, an int32 device tensor (efl_bucket_ids)."""
    if not (isinstance(modulus, int) and isinstance(divisor, int) and 1 <= divisor <= modulus <= MAX_MODULUS):
        raise errors.InvalidArgumentError(
            f"bucket_ids: modulus {modulus!r}, divisor {divisor!r}: 1 <= divisor <= modulus <= 2^31 - 1")
    h = _int32_rows(hashes, "bucket_ids")
    out = torch.empty_like(h)
    _efl_lib.check(_lib.efl_bucket_ids(h.data_ptr(), h.numel(), modulus, divisor, out.data_ptr(),
                                       _efl_lib.stream_handle(h.device)))
    return out


class DefaultKeySelector(object):
    """xfl/data/functions.py DefaultKeySelector: a record's key is the join bucket of its first field."""

    def __init__(self, bucket_num: int = 64, client2multiserver: int = 1):
        if not (isinstance(bucket_num, int) and isinstance(client2multiserver, int) and bucket_num >= 1
                and client2multiserver >= 1 and bucket_num * client2multiserver <= MAX_MODULUS):
            raise errors.InvalidArgumentError(
                f"DefaultKeySelector: bucket_num {bucket_num!r}, client2multiserver {client2multiserver!r}")
        self._bucket_num = bucket_num * client2multiserver
        self._client2multiserver = client2multiserver

    def get_key(self, value):
        return (mmh3_hash(value[0]) % self._bucket_num) // self._client2multiserver

    def get_keys(self, ids=None, hashes=None) -> torch.Tensor:
        """get_key of every ID of a list (packed and hashed here), or of their `hashes`
        (mmh3_hash_rows): an int32 device tensor."""
        if hashes is None:
            hashes = mmh3_hash_rows(*pack_strings(ids))
        return bucket_ids(hashes, self._bucket_num, self._client2multiserver)


def partition_rows(bucket, buckets):
    """(order int64 [n], starts int64 [buckets + 1]) of a stable counting sort of the rows by bucket[i]
    (int32 [n]), on the device (efl_bucket_partition): bucket b is order[starts[b]:starts[b + 1]], its
    row indices ascending. Rows whose bucket is outside [0, buckets) follow the last bucket."""
    if not isinstance(buckets, int) or not 1 <= buckets <= MAX_BUCKETS:
        raise errors.InvalidArgumentError(f"partition_rows: {buckets!r} buckets: 1 <= buckets <= {MAX_BUCKETS}")
    b = _int32_rows(bucket, "partition_rows")
    n, dev = b.numel(), b.device
    order = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return order, torch.zeros(buckets + 1, dtype=torch.int64, device=dev)
    starts = torch.empty(buckets + 1, dtype=torch.int64, device=dev)
    nbytes = int(_lib.efl_bucket_scratch_bytes(n, buckets))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    _efl_lib.check(_lib.efl_bucket_partition(b.data_ptr(), n, buckets, order.data_ptr(), starts.data_ptr(),
                                             scratch.data_ptr(), scratch.numel() * 8, _efl_lib.stream_handle(dev)))
    return order, starts


def gather_strings(chars, offsets, order, permutation=False):
    """(chars, offsets) of the packed strings taken in `order` (int64 [n]), on the device
    (efl_strings_gather). permutation=True: the caller knows that `order` lists every string once
    (partition_rows' does), so the result is as long as the input and nothing is read back to size it."""
    c, o, n = _packed(chars, offsets, "gather_strings")
    order = _efl_lib.as_tensor(order)
    if order.dtype != torch.int64 or order.dim() != 1 or order.numel() != n:
        raise errors.InvalidArgumentError(f"gather_strings: order must be int64 [{n}]")
    dev = c.device
    out_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n == 0:
        return torch.zeros(1, dtype=torch.uint8, device=dev), out_offsets
    order = order.contiguous().to(dev)
    total = c.numel()
    if not permutation:
        inside = (order >= 0) & (order < n)
        rows = order.clamp(0, n - 1)
        total = int(torch.where(inside, (o[rows + 1] - o[rows]).clamp(min=0), torch.zeros_like(rows)).sum())
    out_chars = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    nbytes = int(_lib.efl_strings_gather_scratch_bytes(n))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    _efl_lib.check(_lib.efl_strings_gather(c.data_ptr(), o.data_ptr(), order.data_ptr(), n,
                                           out_chars.data_ptr(), out_offsets.data_ptr(), scratch.data_ptr(),
                                           scratch.numel() * 8, _efl_lib.stream_handle(dev)))
    return out_chars, out_offsets


class Partition(collections.namedtuple("Partition", "chars offsets order starts hashes")):
    """partition()'s result, device tensors: the strings regrouped by bucket (chars uint8, offsets int64
    [n + 1]), `order` (the index in the list given of each regrouped string), `starts` ([buckets + 1])
    and the IDs' hashes in the order given. Bucket b's strings are offsets[starts[b] .. starts[b + 1]]
    over `chars`: the slice the signers' kernels take as it is (`bucket(b)`)."""
    __slots__ = ()

    def bucket(self, b, starts=None):
        """(chars, offsets) of bucket b. `starts`: a host copy of self.starts, to spare the read-back."""
        s = self.starts.tolist() if starts is None else starts
        return self.chars, self.offsets[s[b]:s[b + 1] + 1]


def partition(ids, bucket_num, client2multiserver=1) -> Partition:
    """The IDs of a list grouped by DefaultKeySelector(bucket_num, client2multiserver).get_key: packed
    once, then hashed, partitioned and gathered on the device."""
    selector = DefaultKeySelector(bucket_num, client2multiserver)
    dev = _efl_lib.require_gpu()
    chars, offsets = (t.to(dev) for t in pack_strings(ids))
    hashes = mmh3_hash_rows(chars, offsets)
    order, starts = partition_rows(selector.get_keys(hashes=hashes), bucket_num)
    out_chars, out_offsets = gather_strings(chars, offsets, order, permutation=True)
    return Partition(out_chars, out_offsets, order, starts, hashes)
