"""V(words): the numbers below 2^(32 words) that the decimal conversion (csrc/decimal.h) is tested on,
shared by tests/test_decimal_host.py (the header as a host program) and tests/test_rsa_oneway_gpu.py
(the kernels). Python's own str(int) is the oracle, so the set is made here and never stored.

  - 0, 1, 9, 10 and the neighbours of 10^9, 2^32 and 10^18: one chunk, two chunks, one word, two words
  - 10^k - 1 and 10^k for every k below the width's digit count: every length, all nines, a one
    followed by zero chunks, and the lengths 55, 56, 63, 64, 65, 119, 120 at which SHA-256 blocks end
  - 2^k for k = 0 or 31 mod 32, and 2^(32 words) - 1
  - each single word 0xFFFFFFFF with the others zero
  - 64 seeded random values of full width, and 64 whose top words are zero from a random position
"""
import random


def digits(words: int) -> int:
    return len(str(2 ** (32 * words) - 1))


def values(words: int) -> list:
    top = 2 ** (32 * words)
    v = [0, 1, 9, 10, 10 ** 9 - 1, 10 ** 9, 10 ** 9 + 1, 2 ** 32 - 1, 2 ** 32, 10 ** 18, 10 ** 18 + 10 ** 9]
    for k in range(digits(words)):
        v += [10 ** k - 1, 10 ** k]
    v += [2 ** k for k in range(32 * words) if k % 32 in (0, 31)]
    v.append(top - 1)
    v += [0xFFFFFFFF << (32 * j) for j in range(words)]
    rng = random.Random(1000 + words)
    v += [rng.getrandbits(32 * words) | 1 << (32 * words - 1) for _ in range(64)]
    v += [rng.getrandbits(32 * rng.randint(1, words)) for _ in range(64)]
    v = [x for x in v if x < top]
    assert all(0 <= x < top for x in v)
    return v
