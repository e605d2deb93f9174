"""The reference's default data-join (use_psi=False) without its transport: ServerSortJoinFunc with the
plain DataJoinServer on one side, ClientSortJoinFunc / ClientBatchJoinFunc on the other.

In efls-data both parties key every record by DefaultKeySelector over the hash column
(xfl/data/functions.py:37-46) and per bucket

  server  keeps the record keys hash_col + b'#' + sort_col in a SampleKvStore, answers
          exists(request.ids), appends the ids that hit to its final result and adds them to its
          CheckSum (xfl/service/data_join_server.py:86-102); FinishJoin compares the client's
          CheckSum with its own and answers only once (:74-84)
  client  puts its keys into a dict store per now_bucket_id = subtask c + get_local_bucket_id, sorts
          each store's keys with sorted(keys, key=cmp_to_key(record_cmp)) (functions.py:261; the
          batch join keeps the order given), sends them in batches of batch_size, keeps a CheckSum
          over the keys that hit and raises ValueError("Join finish error") when FinishJoin refuses

Here the keys are packed byte strings on the device: KeyStore is the dict store as a sorted index
(efl.psi.strsort: one sort, the run heads, one binary search per lookup), and the client orders the
keys of every bucket with one segmented sort. The server side runs bucket_num * client2multiserver
buckets of the client's bucket_num, as in efl.psi.bucketed_join."""
from __future__ import annotations

import itertools

import torch

from efl import errors
from efl import lib as _efl_lib
from efl.psi import bucket as _bucket
from efl.psi import strsort as _strsort
from efl.psi.bucketed_join import _check_bucket_num
from efl.psi.check_sum import CheckSum
from efl.psi.rsa_cipher import pack_strings
from efl.psi.strsort import gather_res, get_sample_store_key, to_bytes

_NO_SEGMENT = 2 ** 31 - 1          # above every bucket id: the rows a dict would not keep


def dedup_rows(chars, offsets, values, segment=None):
    """A dict's view of n packed strings put in row order (device tensors; values int64 [n]; segment
    int32 [n] or None: strings are equal only inside one segment). (first, last, order): `first`
    int64 [u] ascending, the row at which each distinct string first appears (dict order); `last`
    int64 [u], the value of the last row with that string; `order`, the bytes-mode sort of the rows
    by (segment, string, row)."""
    order = _strsort.sort_rows(chars, offsets, segment, "bytes")
    heads = _strsort.run_heads(chars, offsets, order).bool()
    if segment is not None:
        s = segment[order]
        heads[1:] |= s[1:] != s[:-1]
    tails = torch.ones_like(heads)
    tails[:-1] = heads[1:]
    # inside a run the row index ascends: its head is the first row, its tail the last
    first, perm = torch.sort(order[heads])
    return first, values[order[tails]][perm], order


class KeyStore(object):
    """The reference's DictSampleKvStore over byte strings of any length with int64 values (the
    caller's record numbers, as in IdStore). Dict semantics: keys() is in insertion order, a repeated
    key keeps its first position and takes its last value. put / put_rows append to a packed buffer
    on the device; the sorted index is built on the first lookup after a change."""

    def __init__(self, device=None):
        self._device = None if device is None else torch.device(device)
        self.clear()

    def clear(self):
        self._chars = self._offsets = self._values = None
        self._rows = 0
        self._pend_keys, self._pend_values = [], []
        self._index = None

    # ---- the packed buffer ---------------------------------------------------------------------

    def _dev(self):
        if self._device is None:
            self._device = _efl_lib.require_gpu()
        return self._device

    def _append(self, chars, offsets, values, nbytes):
        dev = self._dev()
        c, o, v = chars[:nbytes].to(dev), offsets.to(dev), values.to(dev)
        if self._rows == 0:
            self._chars, self._offsets, self._values = c.contiguous(), o.contiguous(), v.contiguous()
        else:
            self._offsets = torch.cat([self._offsets, o[1:] + self._chars.numel()])
            self._chars = torch.cat([self._chars, c])
            self._values = torch.cat([self._values, v])
        self._rows = self._values.numel()
        self._index = None

    def _flush(self):
        if self._pend_keys:
            chars, offsets = pack_strings(self._pend_keys)
            self._append(chars, offsets, torch.tensor(self._pend_values, dtype=torch.int64), int(offsets[-1]))
            self._pend_keys, self._pend_values = [], []

    def put(self, key, value) -> bool:
        """SampleKvStore.put for one byte string and one int, or for a list of each."""
        if isinstance(key, (bytes, bytearray)):
            key, value = [key], [value]
        key, value = list(key), list(value)
        if len(key) != len(value):
            raise errors.InvalidArgumentError(f"KeyStore.put: {len(key)} keys, {len(value)} values")
        for i, k in enumerate(key):
            if not isinstance(k, (bytes, bytearray)):
                raise TypeError(f"KeyStore.put: key {i} is {type(k).__name__}, not bytes")
        self._pend_keys += [bytes(k) for k in key]
        self._pend_values += [int(v) for v in value]
        self._index = None
        return True

    def put_rows(self, chars, offsets, values):
        """put for n packed strings (chars uint8, offsets int64 [n + 1] from 0) and int64 [n] values,
        host or device tensors."""
        chars, offsets, values = (_efl_lib.as_tensor(t) for t in (chars, offsets, values))
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
            raise errors.InvalidArgumentError("KeyStore.put_rows: offsets must be int64 [n + 1]")
        if chars.dtype not in (torch.uint8, torch.int8) or chars.dim() != 1:
            raise errors.InvalidArgumentError("KeyStore.put_rows: chars must be a vector of bytes")
        n = offsets.numel() - 1
        if values.dtype != torch.int64 or values.dim() != 1 or values.numel() != n:
            raise errors.InvalidArgumentError(f"KeyStore.put_rows: values must be int64 [{n}]")
        if n == 0:
            return
        self._flush()
        first, nbytes = int(offsets[0]), int(offsets[-1])
        self._append(chars.view(torch.uint8)[first:], offsets - first, values, nbytes - first)

    # ---- the index -----------------------------------------------------------------------------

    def _built(self):
        """(order, first, value_of_row): the bytes-mode order of all rows put, the first row of every
        key in insertion order, and per first row the key's value."""
        self._flush()
        if self._index is None and self._rows:
            first, last, order = dedup_rows(self._chars, self._offsets, self._values)
            value_of_row = torch.zeros(self._rows, dtype=torch.int64, device=self._device)
            value_of_row[first] = last                   # the first rows are distinct
            self._index = (order, first, value_of_row)
        return self._index

    def _queries(self, keys):
        if isinstance(keys, (list, tuple)) and not (len(keys) == 2 and isinstance(keys[0], torch.Tensor)):
            for i, k in enumerate(keys):
                if not isinstance(k, (bytes, bytearray)):
                    raise TypeError(f"KeyStore: key {i} is {type(k).__name__}, not bytes")
            return pack_strings(keys), True
        return keys, False

    def find(self, q_chars, q_offsets) -> torch.Tensor:
        """int64 [nq] on the device: the row at which each packed query string was first put, or -1."""
        index = self._built()
        dev = self._dev()
        if index is None:
            empty = torch.zeros(1, dtype=torch.int64, device=dev)
            return _strsort.search_rows(torch.zeros(1, dtype=torch.uint8, device=dev), empty, empty[:0],
                                        _efl_lib.as_tensor(q_chars).to(dev), _efl_lib.as_tensor(q_offsets).to(dev))
        return _strsort.search_rows(self._chars, self._offsets, index[0], _efl_lib.as_tensor(q_chars).to(dev),
                                    _efl_lib.as_tensor(q_offsets).to(dev))

    def exists(self, keys):
        """SampleKvStore.exists: a list of bools for a list of byte strings; a bool tensor for packed
        strings (chars, offsets)."""
        (chars, offsets), as_list = self._queries(keys)
        if as_list and not keys:
            return []
        found = self.find(chars, offsets) >= 0
        return found.tolist() if as_list else found

    def get(self, keys):
        """SampleKvStore.get: the value of one byte string, or None; for packed strings (chars,
        offsets) (found bool [n], values int64 [n], -1 where a string is not a key)."""
        if isinstance(keys, (bytes, bytearray)):
            found, values = self.get(pack_strings([bytes(keys)]))
            return int(values[0]) if bool(found[0]) else None
        (chars, offsets), _ = self._queries(keys)
        rows = self.find(chars, offsets)
        found = rows >= 0
        if self._index is None:
            return found, rows
        return found, torch.where(found, self._index[2][rows.clamp(min=0)], torch.full_like(rows, -1))

    def size(self) -> int:
        index = self._built()
        return 0 if index is None else index[1].numel()

    def keys(self) -> list:
        """The keys in insertion order, as dict.keys()."""
        index = self._built()
        if index is None:
            return []
        raw, o = self._chars.cpu().numpy().tobytes(), self._offsets.tolist()
        return [raw[o[r]:o[r + 1]] for r in index[1].tolist()]

    def values(self) -> list:
        index = self._built()
        return [] if index is None else index[2][index[1]].tolist()

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return self.size()


def _bucket_error(bucket_num, bucket_id):
    return errors.InvalidArgumentError('bucket id not match, expect 0..{}, got {}'.format(bucket_num - 1, bucket_id))


class SortJoinServer(object):
    """ServerSortJoinFunc and the DataJoinServer it starts, for every bucket of the job."""

    def __init__(self, bucket_num=64):
        _check_bucket_num(bucket_num, "SortJoinServer")
        self._bucket_num = bucket_num
        self._key_selector = _bucket.DefaultKeySelector(bucket_num)
        self._stores = [KeyStore() for _ in range(bucket_num)]
        self._joined_res = [[] for _ in range(bucket_num)]
        self._check_sums = [CheckSum() for _ in range(bucket_num)]
        self._finished = [False] * bucket_num
        self._ready = False
        self._records = 0

    @property
    def bucket_num(self):
        return self._bucket_num

    def store(self, bucket_id) -> KeyStore:
        self._expect(bucket_id)
        return self._stores[bucket_id]

    def put_records(self, hash_cols, sort_cols, values=None):
        """The server job's key_by and process_element: record i is stored as
        get_sample_store_key(hash_cols[i], sort_cols[i]) in the bucket of its hash column alone, with
        values[i] (None: its record number, counted over all calls)."""
        hash_cols, sort_cols = list(hash_cols), list(sort_cols)
        n = len(hash_cols)
        if len(sort_cols) != n or (values is not None and len(values) != n):
            raise errors.InvalidArgumentError("SortJoinServer.put_records: as many sort columns and values as hash columns")
        values = list(range(self._records, self._records + n)) if values is None else list(values)
        self._records += n
        if n == 0:
            return
        keys = [get_sample_store_key(h, s) for h, s in zip(hash_cols, sort_cols)]
        buckets = self._key_selector.get_keys([to_bytes(h) for h in hash_cols])
        order, starts = (t.tolist() for t in _bucket.partition_rows(buckets, self._bucket_num))
        for b in range(self._bucket_num):
            rows = order[starts[b]:starts[b + 1]]
            if rows:
                self._stores[b].put([keys[i] for i in rows], [values[i] for i in rows])

    def set_is_ready(self, value: bool):
        self._ready = value

    def get_is_ready(self):
        return self._ready

    def _expect(self, bucket_id):
        if not isinstance(bucket_id, int) or isinstance(bucket_id, bool) or not 0 <= bucket_id < self._bucket_num:
            raise _bucket_error(self._bucket_num, bucket_id)

    def sync_join(self, request_ids, bucket_id) -> list:
        """SyncJoin: exists(request_ids) of that bucket's store; the ids that hit are appended to the
        bucket's final result and added to its CheckSum."""
        if not self._ready:
            raise errors.UnavailableError('not_ready')
        self._expect(bucket_id)
        request_ids = list(request_ids)
        res = self._stores[bucket_id].exists(request_ids)
        tmp_res = gather_res(request_ids, res)
        self._joined_res[bucket_id].append(tmp_res)
        self._check_sums[bucket_id].add_list(tmp_res)
        return res

    def finish_join(self, bucket_id, check_sum) -> bool:
        """FinishJoin: True when the client's CheckSum is this bucket's, once; False on a mismatch and
        after the bucket has finished."""
        self._expect(bucket_id)
        if self._finished[bucket_id] or self._check_sums[bucket_id].get_check_sum() != check_sum:
            return False
        self._finished[bucket_id] = True
        return True

    def is_finished(self, bucket_id):
        self._expect(bucket_id)
        return self._finished[bucket_id]

    def get_final_result(self, bucket_id) -> list:
        self._expect(bucket_id)
        return self._joined_res[bucket_id]

    def get_check_sum(self, bucket_id):
        self._expect(bucket_id)
        return self._check_sums[bucket_id].get_check_sum()


class SortJoinClient(object):
    """ClientSortJoinFunc; with need_sort=False the order of ClientBatchJoinFunc."""

    def __init__(self, bucket_num=64, client2multiserver=1, batch_size=2048, need_sort=True):
        _check_bucket_num(bucket_num, "SortJoinClient")
        if not isinstance(client2multiserver, int) or client2multiserver < 1:
            raise errors.InvalidArgumentError(f"SortJoinClient: client2multiserver {client2multiserver!r}")
        _check_bucket_num(bucket_num * client2multiserver, "SortJoinClient")
        if not isinstance(batch_size, int) or batch_size < 1:
            raise errors.InvalidArgumentError(f"SortJoinClient: batch_size {batch_size!r}")
        self._bucket_num = bucket_num
        self._client2multiserver = client2multiserver
        self._batch_size = batch_size
        self._need_sort = bool(need_sort)
        self._key_selector = _bucket.DefaultKeySelector(bucket_num, client2multiserver)
        self._check_sums = [self._new_check_sum() for _ in range(bucket_num * client2multiserver)]

    def _new_check_sum(self):
        return CheckSum()

    def get_check_sum(self, bucket_id):
        return self._check_sums[bucket_id].get_check_sum()

    def _ordered(self, keys, hash_cols):
        """[(now_bucket_id, row of the key, last row with that key)] of the keys a dict per bucket
        keeps, by bucket and inside a bucket in the join's order: computed on the device, read back
        once."""
        c, n = self._client2multiserver, len(keys)
        buckets = self._bucket_num * c
        dev = _efl_lib.require_gpu()
        chars, offsets = (t.to(dev) for t in pack_strings(keys))
        hashes = _bucket.mmh3_hash_rows(*pack_strings(hash_cols))
        now = self._key_selector.get_keys(hashes=hashes) * c + _bucket.bucket_ids(hashes, c)
        first, last, _ = dedup_rows(chars, offsets, torch.arange(n, dtype=torch.int64, device=dev), now)
        # a repeated key's later rows leave every bucket: they sort after the last one
        segment = torch.full_like(now, _NO_SEGMENT)
        segment[first] = now[first]
        last_of = torch.zeros(n, dtype=torch.int64, device=dev)
        last_of[first] = last
        if self._need_sort:
            order = _strsort.sort_rows(chars, offsets, segment, "record")
        else:
            order, _ = _bucket.partition_rows(segment, buckets)
        order = order[:first.numel()]
        return torch.stack([now[order].to(torch.int64), order, last_of[order]], dim=1).tolist()

    def join(self, hash_cols, sort_cols, server, values=None) -> list:
        """The client job against `server` (a SortJoinServer of bucket_num * client2multiserver
        buckets): (now_bucket_id, key) for every key the server has too, or (now_bucket_id, value of
        the key) when `values` is given; in bucket order and inside a bucket in record_cmp's order
        (need_sort) or the order given."""
        hash_cols, sort_cols = list(hash_cols), list(sort_cols)
        n = len(hash_cols)
        if len(sort_cols) != n or (values is not None and len(values) != n):
            raise errors.InvalidArgumentError("SortJoinClient.join: as many sort columns and values as hash columns")
        buckets = self._bucket_num * self._client2multiserver
        self._check_sums = [self._new_check_sum() for _ in range(buckets)]
        keys = [get_sample_store_key(h, s) for h, s in zip(hash_cols, sort_cols)]
        rows = self._ordered(keys, [to_bytes(h) for h in hash_cols]) if n else []
        res = []
        for b, group in itertools.groupby(rows, key=lambda r: r[0]):
            group = list(group)
            for cur in range(0, len(group), self._batch_size):
                batch = group[cur:cur + self._batch_size]
                request_ids = [keys[r[1]] for r in batch]
                existence = server.sync_join(request_ids, b)
                self._check_sums[b].add_list(gather_res(request_ids, existence))
                for r in gather_res(batch, existence):
                    res.append((b, keys[r[1]] if values is None else values[r[2]]))
        finished = True
        for b in range(buckets):
            finished = server.finish_join(b, self._check_sums[b].get_check_sum()) and finished
        if not finished:
            raise ValueError("Join finish error")
        return res
