"""The reference's RSA PSI flow without its transport, over tensors, with the reference's names.

In efls-data the flow runs over gRPC between two Flink jobs (xfl/data/psi/rsa_signer.py,
xfl/service/data_join_server.py: PsiDataJoinServer on DataJoinServer). With (n, e, d) the server's
key, h(x) = sha256(str(x)) and H the one-way hash of a signature's decimal text:

  server  process_element        every local ID x goes into the sample store under H(h(x)^d)
  client  GetRsaPublicKey        (n, e)
          PsiSign                the client blinds its hashes (r^e h(y)), the server signs them
                                 (r h(y)^d) and the client unblinds and hashes: H(h(y)^d)
          SyncJoin               the server answers which of them are keys of its store
          gather_res             the client keeps the IDs that exist
  server  get_final_result       the hits

Here the store is an efl.psi.IdStore(8) on the device, a signed ID is a row of a `uint8` [n, 8] tensor
(rsa_cipher.oneway_rows; rsa_cipher.oneway_text gives the reference's byte string), blinded hashes
and signatures are `int32` [n, words] rows, and nothing leaves the device between the steps except
the existence flags. This is one bucket's join: the bucket hash, the join run bucket by bucket,
CheckSum and FinishJoin are efl.psi.bucket, efl.psi.bucketed_join and efl.psi.check_sum (DESIGN.md
§5h). Left to the service around it: IsReady, gRPC, Flink, LevelDB.
"""
from __future__ import annotations

import torch

from efl import errors
from efl.psi.ecdh_join import gather_res
from efl.psi.id_store import IdStore
from efl.psi.rsa_signer import ClientRsaSigner


class RsaJoinServer(object):
    def __init__(self, signer, batch_size=2048):
        assert signer is not None, "rsa signer should not be None!"
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise errors.InvalidArgumentError("RsaJoinServer: batch_size must be a positive int")
        self._rsa_signer = signer
        self._batch_size = batch_size
        self._ids = []                               # local IDs; the sample store's values index it
        self._sample_kv_store = IdStore(8)           # H(h(x)^d) -> index of x
        self._joined_res = []
        self._request_cnt = self._hit_cnt = self._all_cnt = 0

    def add_ids(self, ids):
        """ServerPsiJoinFunc.process_element for a list of IDs: each goes into the sample store under
        its signed form (ServerRsaSigner.sign_rows), batch_size at a time. A repeated ID is one key."""
        ids = list(ids)
        for o in range(0, len(ids), self._batch_size):
            batch = ids[o:o + self._batch_size]
            first = len(self._ids)
            self._ids.extend(batch)
            self._sample_kv_store.put_rows(self._rsa_signer.sign_rows(batch),
                                           torch.arange(first, first + len(batch), dtype=torch.int64))

    def get_rsa_public_key(self):
        """GetRsaPublicKey: the PEM bytes."""
        return self._rsa_signer.get_public_key_bytes()

    def psi_sign(self, rows) -> torch.Tensor:
        """PsiSign: the signatures of `int32` [n, words] rows of blinded hashes."""
        return self._rsa_signer.sign_blinded_rows(rows)

    def sync_join(self, rows) -> torch.Tensor:
        """SyncJoin: bool [n], which of the client's signed rows (uint8 [n, 8]) are the server's; the
        hits are kept for get_final_result."""
        rows = torch.as_tensor(rows)
        if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != 8:
            raise errors.InvalidArgumentError(
                f"sync_join: rows must be uint8 [n, 8], got {rows.dtype} {tuple(rows.shape)}")
        self._request_cnt += 1
        if rows.shape[0] == 0:
            return torch.zeros(0, dtype=torch.bool, device=rows.device)
        res = self._sample_kv_store.exists(rows)
        self._all_cnt += rows.shape[0]
        hits = rows[res]
        self._hit_cnt += hits.shape[0]
        self._joined_res.append(hits)
        return res

    def get_final_result(self) -> torch.Tensor:
        """The signed rows (uint8 [hits, 8], on the store's device) of every hit so far, in the order the
        client asked."""
        if not self._joined_res:
            return torch.empty((0, 8), dtype=torch.uint8)
        return torch.cat([h.to(self._sample_kv_store.device) for h in self._joined_res])

    def get_final_ids(self) -> list:
        """The server's IDs behind get_final_result (the reference's `_sample_store.get(key)`)."""
        rows = self.get_final_result()
        if rows.shape[0] == 0:
            return []
        found, values = self._sample_kv_store.get(rows)
        return [self._ids[i] for i in values[found].tolist()]


class RsaJoinClient(object):
    def __init__(self, batch_size=2048, oneway_hash="sha256"):
        """oneway_hash: the server signer's, a name of rsa_cipher.ONEWAY_HASHES, a callable or None."""
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise errors.InvalidArgumentError("RsaJoinClient: batch_size must be a positive int")
        self._batch_size = batch_size
        self._oneway_hash = oneway_hash

    def join(self, ids, server) -> list:
        """ClientPsiJoinFunc against `server`: a ClientRsaSigner from the server's key, then the IDs in
        batches (each ID once, as the request buffer's keys are) through blind_rows, the server's
        psi_sign, deblind_rows, sync_join and gather_res. The IDs the server has too, in the order given."""
        request_ids = list(dict.fromkeys(ids))
        signer = ClientRsaSigner(server.get_rsa_public_key(), oneway_hash=self._oneway_hash)
        res_ids = []
        for o in range(0, len(request_ids), self._batch_size):
            batch = request_ids[o:o + self._batch_size]
            blinded, r = signer.blind_rows(batch)
            signed = signer.deblind_rows(server.psi_sign(blinded), r)
            existence = server.sync_join(signed)
            res_ids += gather_res(batch, existence.tolist())
        return res_ids
