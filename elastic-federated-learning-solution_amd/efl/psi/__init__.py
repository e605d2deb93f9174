"""efl.psi - sample alignment by private set intersection on the GPU, both protocols of the
reference's efls-data/xfl/data/psi: RSA blind signatures (rsa_signer.py: the signers with the
reference's names, the key context over device tensors (RsaKey) and the PKCS#1 key reader / writer)
and ECDH over curve25519 (ecc_signer.py: EccSigner, and batched X25519 over uint8 rows in
ecc_cipher)."""
from efl.psi import pkcs1
from efl.psi import rsa_cipher
from efl.psi import rsa_signer
from efl.psi import ecc_cipher
from efl.psi import ecc_signer
from efl.psi.rsa_cipher import RsaKey
from efl.psi.rsa_signer import RsaSigner, ServerRsaSigner, ClientRsaSigner
from efl.psi.ecc_signer import EccSigner

__all__ = ["RsaSigner", "ServerRsaSigner", "ClientRsaSigner", "RsaKey", "EccSigner", "pkcs1", "rsa_cipher",
           "rsa_signer", "ecc_cipher", "ecc_signer"]
