"""The order of the reference's default data-join, on the device, with the reference's names.

With use_psi=False efls-data joins on record keys `hash_col + b'#' + sort_col`
(xfl/data/utils.py:63-69: get_sample_store_key over to_bytes). The client sorts each bucket's keys
with sorted(keys, key=cmp_to_key(record_cmp)) (xfl/data/functions.py:49-60,261): by the sort column's
bytes, then the hash column's, both in Python's `bytes` order, ties in the order given (the sort is
stable). Batches, output records and both CheckSum chains follow that order, so a client that sorts
differently fails FinishJoin.

`get_sample_store_key`, `split_sample_store_key`, `gather_res` and `record_cmp` are the per-record
forms, on the host. The batched forms work on byte strings packed as efl.psi.bucket packs them (chars
uint8, offsets int64 [n + 1]; pack_strings makes them) and stay on the device: `sort_rows` (the order
of (segment, key, row index): one call sorts every bucket at once), `search_rows` (one binary search
per query in a sorted table), `run_heads` (where a run of equal strings starts), and `sort_keys`,
which packs a list and sorts it.
"""
from __future__ import annotations

import numpy as np
import torch

from efl import errors
from efl import lib as _efl_lib
from efl.psi.bucket import _packed
from efl.psi.rsa_cipher import pack_strings

_lib = _efl_lib.raw()

SORT_BYTES, SORT_RECORD = 0, 1
_MODES = {"bytes": SORT_BYTES, "record": SORT_RECORD}


def gather_res(ids, existence):
    """xfl/data/utils.py gather_res: the ids whose existence is true."""
    assert len(ids) == len(existence), \
        'ids size {}, existence size {}'.format(len(ids), len(existence))
    res = []
    for i in range(0, len(existence)):
        if existence[i]:
            res.append(ids[i])
    return res


def to_bytes(v):
    if isinstance(v, bytes):
        return v
    return str(v).encode('utf-8')


def get_sample_store_key(hash_col_value, sort_col_value):
    return to_bytes(hash_col_value) + b'#' + to_bytes(sort_col_value)


def split_sample_store_key(sample_store_key: bytes):
    t = sample_store_key.split(b'#')
    return t


def record_cmp(left, right):
    """xfl/data/functions.py record_cmp: the sort column, then the hash column, as bytes."""
    a = split_sample_store_key(left)
    b = split_sample_store_key(right)
    if a[1] < b[1]:
        return -1
    if a[1] > b[1]:
        return 1
    if a[0] < b[0]:
        return -1
    if a[0] > b[0]:
        return 1
    return 0


def _mode(mode, what):
    try:
        return _MODES[mode]
    except (KeyError, TypeError):
        raise errors.InvalidArgumentError(f'{what}: mode {mode!r}: "bytes" or "record"') from None


def _int64_rows(t, n, dev, what):
    t = _efl_lib.as_tensor(t)
    if t.dtype != torch.int64 or t.dim() != 1 or t.numel() != n:
        raise errors.InvalidArgumentError(f"{what} must be int64 [{n}]")
    return t.contiguous().to(dev)


def sort_rows(chars, offsets, segment=None, mode="record") -> torch.Tensor:
    """order (int64 [n], on the device): the rows of the packed strings ascending in (segment[i], key
    order, i) (efl_strings_sort). segment: int32 [n] or None (one segment). mode "record": the bytes
    between the first and the second '#' (or to the end), then the bytes before the first '#', as
    record_cmp compares them; a key without '#' has an empty second field here (sort_keys refuses it).
    mode "bytes": the whole string in Python's bytes order."""
    m = _mode(mode, "sort_rows")
    c, o, n = _packed(chars, offsets, "sort_rows")
    dev = c.device
    seg = None
    if segment is not None:
        seg = _efl_lib.as_tensor(segment)
        if seg.dtype != torch.int32 or seg.dim() != 1 or seg.numel() != n:
            raise errors.InvalidArgumentError(f"sort_rows: segment must be int32 [{n}]")
        seg = seg.contiguous().to(dev)
    order = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return order
    nbytes = int(_lib.efl_strings_sort_scratch_bytes(n))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    _efl_lib.check(_lib.efl_strings_sort(c.data_ptr(), o.data_ptr(), None if seg is None else seg.data_ptr(), n, m,
                                         order.data_ptr(), scratch.data_ptr(), scratch.numel() * 8,
                                         _efl_lib.stream_handle(dev)))
    return order


def search_rows(t_chars, t_offsets, t_order, q_chars, q_offsets) -> torch.Tensor:
    """int64 [nq] on the device: for every query string the row of the table string equal to it, the
    lowest such row, or -1 (efl_strings_search). t_order is sort_rows(t_chars, t_offsets, None,
    "bytes")."""
    qc, qo, nq = _packed(q_chars, q_offsets, "search_rows")
    dev = qc.device
    tc, to, m = _packed(_efl_lib.as_tensor(t_chars).to(dev), _efl_lib.as_tensor(t_offsets).to(dev), "search_rows")
    order = _int64_rows(t_order, m, dev, "search_rows: t_order")
    out = torch.empty(nq, dtype=torch.int64, device=dev)
    if nq == 0:
        return out
    _efl_lib.check(_lib.efl_strings_search(tc.data_ptr(), to.data_ptr(), order.data_ptr() if m else None, m, qc.data_ptr(),
                                           qo.data_ptr(), nq, out.data_ptr(), _efl_lib.stream_handle(dev)))
    return out


def run_heads(chars, offsets, order) -> torch.Tensor:
    """uint8 [n] on the device: 1 at place k when k == 0 or the strings of rows order[k] and order[k - 1]
    differ (efl_strings_run_heads)."""
    c, o, n = _packed(chars, offsets, "run_heads")
    dev = c.device
    order = _int64_rows(order, n, dev, "run_heads: order")
    heads = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return heads
    _efl_lib.check(_lib.efl_strings_run_heads(c.data_ptr(), o.data_ptr(), order.data_ptr(), n, heads.data_ptr(),
                                              _efl_lib.stream_handle(dev)))
    return heads


def check_record_keys(chars, offsets):
    """What record_cmp's a[1] raises for a key without '#', looked for in the packed bytes (host
    tensors) before anything is sorted."""
    c, o = chars.numpy(), offsets.numpy()
    n = o.shape[0] - 1
    if n == 0:
        return
    marks = np.concatenate([[0], np.cumsum(c == ord("#"), dtype=np.int64)])     # '#'s before each byte
    if np.any(marks[o[1:]] == marks[o[:-1]]):
        raise IndexError('list index out of range')


def sort_keys(keys, mode="record") -> list:
    """The list of byte strings sorted on the device. mode "record": sorted(keys,
    key=cmp_to_key(record_cmp)), with its IndexError for a key without '#'; mode "bytes": sorted(keys)."""
    m = _mode(mode, "sort_keys")
    keys = list(keys)
    for i, k in enumerate(keys):
        if not isinstance(k, bytes):
            raise TypeError(f"sort_keys: key {i} is {type(k).__name__}, not bytes")
    if not keys:
        return []
    chars, offsets = pack_strings(keys)
    if m == SORT_RECORD:
        check_record_keys(chars, offsets)
    return [keys[i] for i in sort_rows(chars, offsets, None, mode).tolist()]
