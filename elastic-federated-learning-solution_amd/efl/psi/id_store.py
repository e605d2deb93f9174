"""IdStore: the reference's signed-ID store (efls-data/xfl/data/store/sample_kv_store.py,
DictSampleKvStore: a Python dict from signed ID to value) as a hash table in device memory, built and
probed by the efl_idset_* kernels of libefl_hip.so (include/efl_hip.h, csrc/idset.h).

Keys are rows of a `uint8` [n, width] tensor, width 32 (an X25519 output) or 8 (a 64-bit one-way hash
of an RSA signature); values are `int64`. The semantics are the dict's: a key keeps the position of
its first insertion (`keys()` is in insertion order, as `dict.keys()` is), a repeated key takes the
last value given. Tensors may be on the host or on the device and results come back where the rows
were, as in efl.psi.ecc_cipher; the list-of-bytes forms `put(key, value)` / `exists(list)` keep the
reference's signatures.

`put_rows` does not synchronise: the store tracks a host upper bound of its size (every row counted
as new) and reads the true size back only when that bound would force the table to grow. The table
doubles and is rehashed from the dense key array when the bound passes half its capacity.
"""
from __future__ import annotations

import os

import torch

from efl import errors
from efl import lib as _efl_lib

_lib = _efl_lib.raw()

WIDTHS = (8, 32)
MAX_ENTRIES = 2 ** 31 - 2
MAX_CAPACITY = 2 ** 32
DEFAULT_CAPACITY = 1024
_I64_MIN = -2 ** 63


def hash_row(seed: int, row: bytes) -> int:
    """efl_idset_hash: the 64-bit hash of one row under `seed` (host only). A store of capacity C
    starts the row's probe chain at slot hash & (C - 1)."""
    if not isinstance(row, (bytes, bytearray)) or len(row) not in WIDTHS:
        raise errors.InvalidArgumentError("hash_row: a row is 8 or 32 bytes")
    return int(_lib.efl_idset_hash(int(seed) & (2 ** 64 - 1), bytes(row), len(row)))


def rows_from_bytes(items, width: int, what="IdStore") -> torch.Tensor:
    """Host uint8 [n, width] tensor of `width`-byte strings; ValueError naming the first item that is not one."""
    items = list(items)
    for i, v in enumerate(items):
        if not isinstance(v, (bytes, bytearray)) or len(v) != width:
            raise ValueError(f"{what}: item {i} is not a {width}-byte string")
    return torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).reshape(len(items), width)


class IdStore(object):
    def __init__(self, width=32, capacity=None, seed=None, device=None):
        """width: bytes per key, 8 or 32. capacity: slots of the hash table, a power of two (it holds
        capacity / 2 keys before it grows); 1024 when None. seed: 64 bits of the hash's seed,
        os.urandom when None: rows come from the peer, so the seed stays private. device: the ROCm
        device (the current one at first use when None). Needs no GPU."""
        if width not in WIDTHS:
            raise errors.InvalidArgumentError(f"IdStore: width {width!r}: keys are 8 or 32 bytes")
        capacity = DEFAULT_CAPACITY if capacity is None else capacity
        if not isinstance(capacity, int) or capacity < 2 or capacity > MAX_CAPACITY or capacity & (capacity - 1):
            raise errors.InvalidArgumentError(f"IdStore: capacity {capacity!r} is not a power of two in 2 .. 2^32")
        self.width = width
        self.seed = (int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)) & (2 ** 64 - 1)
        self._capacity = capacity
        self._device = None if device is None else torch.device(device)
        self._bound = 0              # host upper bound of the size
        self._exact = True           # _bound is the size itself
        self._keys = self._values = self._slots = self._size = self._last = None

    # ---- buffers -------------------------------------------------------------------------------

    @property
    def capacity(self) -> int:
        return self._capacity

    @property
    def device(self):
        return self._device

    def _allocate(self, capacity):
        dev = self._device
        self._keys = torch.empty((capacity // 2, self.width), dtype=torch.uint8, device=dev)
        self._values = torch.empty(capacity // 2, dtype=torch.int64, device=dev)
        self._last = torch.empty(capacity // 2, dtype=torch.int64, device=dev)   # scratch of _assign
        self._slots = torch.full((capacity,), -1, dtype=torch.int32, device=dev)  # 0xFFFFFFFF: empty
        self._capacity = capacity

    def _ensure(self):
        if self._keys is None:
            if self._device is None:
                self._device = _efl_lib.require_gpu()
            elif self._device.type != "cuda":
                raise errors.InvalidArgumentError(f"IdStore: {self._device} is not a ROCm device")
            self._size = torch.zeros(1, dtype=torch.int64, device=self._device)
            self._allocate(self._capacity)

    def _stream(self):
        return _efl_lib.stream_handle(self._device)

    def _reserve(self, n):
        """Room for n more keys at a load factor of at most 1/2."""
        if 2 * (self._bound + n) > self._capacity and not self._exact:
            self.size()                                   # the one place put_rows may synchronise
        need = self._bound + n
        if n > MAX_ENTRIES or need > MAX_ENTRIES:
            raise errors.ResourceExhaustedError(f"IdStore: {need} keys: a store holds at most 2^31 - 2")
        if 2 * need <= self._capacity:
            return
        capacity = self._capacity
        while capacity < 2 * need:
            capacity *= 2
        keys, values, kept = self._keys, self._values, self._bound
        self._allocate(capacity)
        self._keys[:kept] = keys[:kept]
        self._values[:kept] = values[:kept]
        _efl_lib.check(_lib.efl_idset_rehash(self._keys.data_ptr(), self.width, self._size.data_ptr(), kept,
                                             self._slots.data_ptr(), capacity, self.seed, self._stream()))

    def _rows(self, rows, what):
        t = _efl_lib.as_tensor(rows)
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != self.width:
            raise errors.InvalidArgumentError(
                f"IdStore.{what}: rows must be uint8 [n, {self.width}], got {t.dtype} {tuple(t.shape)}")
        return t

    def _staged(self, t):
        """Contiguous, aligned rows on the store's device, and where the result goes."""
        self._ensure()
        home = t.device
        d = t.contiguous().to(self._device)
        if d.data_ptr() % (16 if self.width == 32 else 8):
            d = d.clone()
        return d, home

    # ---- tensors -------------------------------------------------------------------------------

    def put_rows(self, rows, values=None) -> torch.Tensor:
        """Inserts the rows that are not keys yet, in row order, and gives every row's value to its
        key (values: int64 [n]; among equal rows the last one's stays, the dict's d[k] = v; None: the
        key's position). Returns the int64 [n] positions of the rows' keys. No host synchronisation
        unless the table has to grow."""
        t = self._rows(rows, "put_rows")
        n = t.shape[0]
        v = None
        if values is not None:
            v = _efl_lib.as_tensor(values)
            if v.dtype != torch.int64 or v.dim() != 1 or v.shape[0] != n:
                raise errors.InvalidArgumentError(f"IdStore.put_rows: values must be int64 [{n}]")
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=t.device)
        d, home = self._staged(t)
        self._reserve(n)
        pos = torch.empty(n, dtype=torch.int64, device=self._device)
        nbytes = int(_lib.efl_idset_scratch_bytes(n))
        scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=self._device)
        _efl_lib.check(_lib.efl_idset_insert(d.data_ptr(), n, self.width, self._keys.data_ptr(), self._keys.shape[0],
                                             self._size.data_ptr(), self._bound, self._slots.data_ptr(),
                                             self._capacity, self.seed, pos.data_ptr(), scratch.data_ptr(), nbytes,
                                             self._stream()))
        self._bound += n
        self._exact = False
        self._assign(pos, pos if v is None else v.to(self._device))
        return _efl_lib.back(pos, home)

    def _assign(self, pos, v):
        """values[pos[i]] = v[i], the highest i winning among equal positions: two amax reductions
        (the last row index per position, then the value of exactly that row), which no order of the
        lanes changes; no indexed store over duplicate positions."""
        idx = torch.arange(pos.shape[0], dtype=torch.int64, device=pos.device)
        self._last.scatter_reduce_(0, pos, idx, "amax", include_self=False)
        mine = torch.where(self._last.gather(0, pos) == idx, v, torch.full_like(v, _I64_MIN))
        self._values.scatter_reduce_(0, pos, mine, "amax", include_self=False)

    def find(self, rows) -> torch.Tensor:
        """int64 [n]: the position of each row among keys(), -1 for a row that is not a key."""
        t = self._rows(rows, "find")
        n = t.shape[0]
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=t.device)
        d, home = self._staged(t)
        pos = torch.empty(n, dtype=torch.int64, device=self._device)
        _efl_lib.check(_lib.efl_idset_find(d.data_ptr(), n, self.width, self._keys.data_ptr(), self._slots.data_ptr(),
                                           self._capacity, self.seed, pos.data_ptr(), self._stream()))
        return _efl_lib.back(pos, home)

    def exists(self, rows):
        """bool [n] for a tensor of rows; for a list of byte strings a list of bools
        (SampleKvStore.exists)."""
        if isinstance(rows, (list, tuple)):
            if not rows:
                return []
            return (self.find(rows_from_bytes(rows, self.width, "IdStore.exists")) >= 0).tolist()
        return self.find(rows) >= 0

    def get(self, rows):
        """(found bool [n], values int64 [n]) for a tensor of rows, -1 where a row is not a key; for
        one byte string its value, or None (SampleKvStore.get)."""
        if isinstance(rows, (bytes, bytearray)):
            found, vals = self.get(rows_from_bytes([rows], self.width, "IdStore.get"))
            return int(vals[0]) if bool(found[0]) else None
        pos = self.find(rows)
        if pos.shape[0] == 0:
            return pos >= 0, pos
        found = pos >= 0
        vals = self._values.gather(0, pos.to(self._device).clamp(min=0)).to(pos.device)
        return found, torch.where(found, vals, torch.full_like(vals, -1))

    def size(self) -> int:
        """The number of keys (synchronises)."""
        if self._keys is not None and not self._exact:
            self._bound = int(self._size.item())
            self._exact = True
        return self._bound

    def keys(self) -> torch.Tensor:
        """uint8 [size, width] on the device, in insertion order: a view of the store's key array,
        valid until the next put_rows or clear."""
        if self._keys is None:
            return torch.empty((0, self.width), dtype=torch.uint8)
        return self._keys[:self.size()]

    def values(self) -> torch.Tensor:
        """int64 [size], the value of each key of keys() (a view, as keys() is)."""
        if self._keys is None:
            return torch.empty(0, dtype=torch.int64)
        return self._values[:self.size()]

    def iter_batches(self, batch_size=2048):
        """keys() in order, batch_size rows at a time (EcdhDataJoinServer._fetch_a_batch)."""
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise errors.InvalidArgumentError("IdStore.iter_batches: batch_size must be a positive int")
        keys = self.keys()
        for o in range(0, keys.shape[0], batch_size):
            yield keys[o:o + batch_size]

    def clear(self):
        if self._keys is not None:
            self._slots.fill_(-1)
            self._size.zero_()
        self._bound = 0
        self._exact = True

    # ---- the reference's list-of-bytes forms ---------------------------------------------------

    def put(self, key, value) -> bool:
        """SampleKvStore.put for one byte string and one int, or for a list of each."""
        if isinstance(key, (bytes, bytearray)):
            key, value = [key], [value]
        key, value = list(key), list(value)
        if len(key) != len(value):
            raise errors.InvalidArgumentError(f"IdStore.put: {len(key)} keys, {len(value)} values")
        if key:
            self.put_rows(rows_from_bytes(key, self.width, "IdStore.put"), torch.tensor(value, dtype=torch.int64))
        return True
