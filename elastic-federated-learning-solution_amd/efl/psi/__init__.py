"""efl.psi - sample alignment by private set intersection on the GPU, both protocols of the
reference's efls-data/xfl/data/psi: RSA blind signatures (rsa_signer.py: the signers with the
reference's names, the key context over device tensors (RsaKey), the decimal text and one-way hash of
a signature (rsa_cipher) and the PKCS#1 key reader / writer) and ECDH over curve25519 (ecc_signer.py:
EccSigner, and batched X25519 over uint8 rows in ecc_cipher); and what the signed IDs go into: IdStore
(id_store.py), the reference's SampleKvStore as a hash table in device memory, and the transport-free
joins on top of it (ecdh_join.py: EcdhJoinServer, EcdhJoinClient; rsa_join.py: RsaJoinServer,
RsaJoinClient); and what the reference's jobs put around a join: the bucket hash that keys every record
to one join per bucket (bucket.py: mmh3_hash, DefaultKeySelector, get_local_bucket_id, partition),
the CheckSum that closes a bucket's join (check_sum.py) and the joins run bucket by bucket
(bucketed_join.py: BucketedJoinServer, BucketedJoinClient); and the join the reference runs by default,
on raw record keys: record_cmp's order as a segmented string sort with a search in the sorted result
(strsort.py: sort_rows, search_rows, run_heads, sort_keys), the dict store over keys of any length and
the two sides of the sort join (sort_join.py: KeyStore, SortJoinServer, SortJoinClient)."""
from efl.psi import pkcs1
from efl.psi import rsa_cipher
from efl.psi import rsa_signer
from efl.psi import ecc_cipher
from efl.psi import ecc_signer
from efl.psi import id_store
from efl.psi import ecdh_join
from efl.psi import rsa_join
from efl.psi.rsa_cipher import RsaKey
from efl.psi.rsa_signer import RsaSigner, ServerRsaSigner, ClientRsaSigner
from efl.psi.ecc_signer import EccSigner
from efl.psi.id_store import IdStore
from efl.psi.ecdh_join import EcdhJoinServer, EcdhJoinClient
from efl.psi.rsa_join import RsaJoinServer, RsaJoinClient
from efl.psi import bucket
from efl.psi import bucketed_join
from efl.psi.bucket import mmh3_hash, mmh3_hash_rows, get_local_bucket_id, DefaultKeySelector, partition
from efl.psi.check_sum import CheckSum, check_sum
from efl.psi.bucketed_join import BucketedJoinServer, BucketedJoinClient
from efl.psi import strsort
from efl.psi import sort_join
from efl.psi.strsort import (get_sample_store_key, split_sample_store_key, gather_res, record_cmp, sort_rows,
                             search_rows, run_heads, sort_keys)
from efl.psi.sort_join import KeyStore, SortJoinServer, SortJoinClient

__all__ = ["RsaSigner", "ServerRsaSigner", "ClientRsaSigner", "RsaKey", "EccSigner", "IdStore", "EcdhJoinServer",
           "EcdhJoinClient", "RsaJoinServer", "RsaJoinClient", "pkcs1", "rsa_cipher", "rsa_signer", "ecc_cipher",
           "ecc_signer", "id_store", "ecdh_join", "rsa_join", "bucket", "bucketed_join", "mmh3_hash",
           "mmh3_hash_rows", "get_local_bucket_id", "DefaultKeySelector", "partition", "CheckSum", "check_sum",
           "BucketedJoinServer", "BucketedJoinClient", "strsort", "sort_join", "get_sample_store_key",
           "split_sample_store_key", "gather_res", "record_cmp", "sort_rows", "search_rows", "run_heads", "sort_keys",
           "KeyStore", "SortJoinServer", "SortJoinClient"]
