"""efl.psi - sample alignment by RSA blind-signature PSI on the GPU (the reference's
efls-data/xfl/data/psi/rsa_signer.py): the signers with the reference's names, the key context over
device tensors (RsaKey) and the PKCS#1 key reader / writer."""
from efl.psi import pkcs1
from efl.psi import rsa_cipher
from efl.psi import rsa_signer
from efl.psi.rsa_cipher import RsaKey
from efl.psi.rsa_signer import RsaSigner, ServerRsaSigner, ClientRsaSigner

__all__ = ["RsaSigner", "ServerRsaSigner", "ClientRsaSigner", "RsaKey", "pkcs1", "rsa_cipher", "rsa_signer"]
