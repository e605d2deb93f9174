"""xfl/data/check_sum.py with the reference's names: the running hash by which the two sides of a
bucket's join agree on what was joined (DataJoinServer.FinishJoin compares the client's value with
its own). `add` is the definition, cur = mmh3.hash(str(cur).encode('utf-8') + value); `add_list` runs
the same chain over a whole list in one host call (efl_mmh3_checksum_host). The chain is serial by
definition and stays on the host."""
from __future__ import annotations

import ctypes

import numpy as np

from efl import lib as _efl_lib
from efl.psi.bucket import mmh3_hash

_lib = _efl_lib.raw()


def check_sum(values: list):
    _check_sum = CheckSum()
    for i in values:
        if isinstance(i, bytes):
            _check_sum.add(i)
        elif isinstance(i, list):
            _check_sum.add_list(i)
        else:
            raise TypeError(type(values))
    return _check_sum.get_check_sum()


class CheckSum(object):
    def __init__(self, seed=0):
        self._cur = seed

    def add(self, value: bytes):
        self._cur = mmh3_hash(str(self._cur).encode('utf-8') + value)

    def add_list(self, value: list):
        value = list(value)
        # the batched chain starts from a signed 32-bit value (every value after the first add is one)
        if len(value) < 2 or not isinstance(self._cur, int) or not -2 ** 31 <= self._cur < 2 ** 31 \
                or not all(isinstance(i, bytes) for i in value):
            for i in value:
                self.add(i)
            return
        offsets = np.zeros(len(value) + 1, dtype=np.int64)
        np.cumsum([len(i) for i in value], out=offsets[1:])
        chars = b"".join(value) or b"\0"
        self._cur = int(_lib.efl_mmh3_checksum_host(self._cur, ctypes.c_char_p(chars), offsets.ctypes.data, len(value)))

    def get_check_sum(self):
        return self._cur
