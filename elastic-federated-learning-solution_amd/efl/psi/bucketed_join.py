"""The reference's bucketed data-join without its transport: one join per bucket, each closed by a
CheckSum, on top of the EcdhJoin* and RsaJoin* halves.

In efls-data both parties key every record by DefaultKeySelector (mmh3.hash(id) % bucket_num,
xfl/data/functions.py:37-46), Flink hands each subtask the records of one key, and per bucket

  server  one DataJoinServer with its own stores; SyncJoin refuses a request for another bucket
          ('bucket id not match, expect .., got ..') and adds the request IDs that hit to its CheckSum
          (xfl/service/data_join_server.py:86-102,203-222)
  client  subtask k talks to the `client2multiserver` servers k c .. k c + c - 1: a record goes to
          now_bucket_id = k c + get_local_bucket_id(id, c), in batches of batch_size, with a CheckSum
          per server over the request IDs that hit (xfl/service/data_join_client.py:144-157)
  finish  FinishJoin(bucket_id, check_sum): the server compares, and answers only once
          (data_join_server.py:74-84); the client raises ValueError("Join finish error") otherwise

Here the IDs are hashed and partitioned on the device (efl.psi.bucket), every bucket gets a server
and a client of its own from a factory (each with its own IdStores, as each reference subtask has),
and a request ID is a row of the tensor sync_join is given: the CheckSum chains run over the rows'
bytes. The server side runs bucket_num * client2multiserver buckets of the client's bucket_num."""
from __future__ import annotations

import torch

from efl import errors
from efl.psi import bucket as _bucket
from efl.psi.check_sum import CheckSum


def row_bytes(rows) -> list:
    """The rows of a 2-D uint8 tensor as byte strings: the request IDs a CheckSum runs over."""
    t = torch.as_tensor(rows).detach().cpu().contiguous()
    raw, w = t.numpy().tobytes(), t.shape[1]
    return [raw[i:i + w] for i in range(0, len(raw), w)]


def _check_bucket_num(bucket_num, what):
    if not isinstance(bucket_num, int) or not 1 <= bucket_num <= _bucket.MAX_BUCKETS:
        raise errors.InvalidArgumentError(f"{what}: bucket_num {bucket_num!r}: 1 <= bucket_num <= {_bucket.MAX_BUCKETS}")


def _groups(ids, keys, buckets):
    """[(ids of bucket b in the order given)] from the device partition of `keys`: one read-back."""
    order, starts = _bucket.partition_rows(keys, buckets)
    order, starts = order.tolist(), starts.tolist()
    return [[ids[i] for i in order[starts[b]:starts[b + 1]]] for b in range(buckets)]


class BucketJoinServer(object):
    """One bucket's DataJoinServer: a join server (EcdhJoinServer / RsaJoinServer; every other
    attribute is that server's), the bucket id it answers for and its CheckSum."""

    def __init__(self, server, bucket_id):
        self._server = server
        self._bucket_id = bucket_id
        self._check_sum = CheckSum()
        self._finished = False

    def __getattr__(self, name):
        return getattr(self._server, name)

    @property
    def bucket_id(self):
        return self._bucket_id

    def _expect(self, bucket_id):
        if self._bucket_id != bucket_id:
            raise errors.InvalidArgumentError(
                'bucket id not match, expect {}, got {}'.format(self._bucket_id, bucket_id))

    def sync_join(self, rows, bucket_id) -> torch.Tensor:
        """SyncJoin: the join server's answer; the request rows that hit go into the CheckSum."""
        self._expect(bucket_id)
        rows = torch.as_tensor(rows)
        res = self._server.sync_join(rows)
        if rows.shape[0]:
            self._check_sum.add_list(row_bytes(rows[res.to(rows.device)]))
        return res

    def get_check_sum(self):
        return self._check_sum.get_check_sum()

    def finish_join(self, bucket_id, check_sum) -> bool:
        """FinishJoin: True when the client's CheckSum is this bucket's, once; False on a mismatch and
        after it has finished."""
        self._expect(bucket_id)
        if self._finished or self._check_sum.get_check_sum() != check_sum:
            return False
        self._finished = True
        return True

    def is_finished(self):
        return self._finished


class BucketedJoinServer(object):
    def __init__(self, server_factory, bucket_num=64):
        """server_factory(bucket_id): that bucket's join server, e.g.
        lambda b: EcdhJoinServer(signer, batch_size)."""
        _check_bucket_num(bucket_num, "BucketedJoinServer")
        self._bucket_num = bucket_num
        self._key_selector = _bucket.DefaultKeySelector(bucket_num)
        self._buckets = [BucketJoinServer(server_factory(b), b) for b in range(bucket_num)]

    @property
    def bucket_num(self):
        return self._bucket_num

    def bucket(self, bucket_id) -> BucketJoinServer:
        if not isinstance(bucket_id, int) or not 0 <= bucket_id < self._bucket_num:
            raise errors.InvalidArgumentError(
                'bucket id not match, expect 0..{}, got {}'.format(self._bucket_num - 1, bucket_id))
        return self._buckets[bucket_id]

    def add_ids(self, ids):
        """The server job's key_by: every ID goes to the join server of its bucket, in the order given."""
        ids = list(ids)
        if not ids:
            return
        for b, group in enumerate(_groups(ids, self._key_selector.get_keys(ids), self._bucket_num)):
            if group:
                self._buckets[b].add_ids(group)

    def sync_join(self, rows_or_ids, bucket_id) -> torch.Tensor:
        return self.bucket(bucket_id).sync_join(rows_or_ids, bucket_id)

    def finish_join(self, bucket_id, check_sum) -> bool:
        return self.bucket(bucket_id).finish_join(bucket_id, check_sum)

    def get_check_sum(self, bucket_id):
        return self.bucket(bucket_id).get_check_sum()

    def get_final_ids(self) -> list:
        """Per bucket: the server's IDs behind that bucket's hits."""
        return [b.get_final_ids() for b in self._buckets]


class _BucketPort(object):
    """What a bucket's join client sees of the server: that bucket's join server, with sync_join sent
    under the bucket id and the client's CheckSum kept (DataJoinClient.sync_join)."""

    def __init__(self, server, bucket_id, check_sum):
        self._server = server
        self._bucket_id = bucket_id
        self._check_sum = check_sum

    def __getattr__(self, name):
        return getattr(self._server.bucket(self._bucket_id), name)

    def sync_join(self, rows) -> torch.Tensor:
        rows = torch.as_tensor(rows)
        res = self._server.sync_join(rows, self._bucket_id)
        if rows.shape[0]:
            self._check_sum.add_list(row_bytes(rows[res.to(rows.device)]))
        return res


class BucketedJoinClient(object):
    def __init__(self, client_factory, bucket_num=64, client2multiserver=1):
        """client_factory(bucket_id): the join client of that server bucket, e.g.
        lambda b: EcdhJoinClient(signer, batch_size); its batch_size is the join's. The server runs
        bucket_num * client2multiserver buckets."""
        _check_bucket_num(bucket_num, "BucketedJoinClient")
        if not isinstance(client2multiserver, int) or client2multiserver < 1:
            raise errors.InvalidArgumentError(f"BucketedJoinClient: client2multiserver {client2multiserver!r}")
        _check_bucket_num(bucket_num * client2multiserver, "BucketedJoinClient")
        self._bucket_num = bucket_num
        self._client2multiserver = client2multiserver
        self._client_factory = client_factory
        self._key_selector = _bucket.DefaultKeySelector(bucket_num, client2multiserver)
        self._check_sums = [CheckSum() for _ in range(bucket_num * client2multiserver)]

    def get_check_sum(self, bucket_id):
        return self._check_sums[bucket_id].get_check_sum()

    def _now_bucket_ids(self, ids) -> torch.Tensor:
        """subtask (get_key) * c + get_local_bucket_id of every ID, on the device."""
        c = self._client2multiserver
        hashes = _bucket.mmh3_hash_rows(*_bucket.pack_strings(ids))
        return self._key_selector.get_keys(hashes=hashes) * c + _bucket.bucket_ids(hashes, c)

    def join(self, ids, server) -> list:
        """The client job against `server`: the IDs keyed by subtask and local bucket, every
        now_bucket_id joined through its own client, then FinishJoin with that bucket's CheckSum.
        (bucket_id, id) for every ID the server has too, in bucket order and inside a bucket in the
        order given: what the reference yields as (str(now_bucket_id), value)."""
        ids = list(ids)
        buckets = self._bucket_num * self._client2multiserver
        self._check_sums = [CheckSum() for _ in range(buckets)]
        groups = _groups(ids, self._now_bucket_ids(ids), buckets) if ids else [[] for _ in range(buckets)]
        res = []
        for b, group in enumerate(groups):
            if group:
                port = _BucketPort(server, b, self._check_sums[b])
                res += [(b, i) for i in self._client_factory(b).join(group, port)]
        finished = True
        for b in range(buckets):
            finished = server.finish_join(b, self._check_sums[b].get_check_sum()) and finished
        if not finished:
            raise ValueError("Join finish error")
        return res
