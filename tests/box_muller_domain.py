"""The domain of the DP noise kernel's Box-Muller (csrc/mask.hip, csrc/box_muller_math.h,
csrc/sincos_angle.h), for tests (a plain helper, no fixtures).

Uint32ToFloat keeps 23 bits of a Philox word, so Box-Muller sees 2^23 radius uniforms and 2^23 angle
uniforms, u = k 2^-23. Here are the word sets that walk both marginals completely (every radius at
one angle, every angle at one radius, and two pairings k -> (k m) mod 2^23 with m odd, which are
bijections), the ordered-ulp distance, the float64 references, and the host build of
csrc/sincos_angle.h: a C program (gcc -O2 -ffp-contract=off, as tests/test_sincos_angle.py compiles
the header) that writes the angle v = efl_box_muller_angle(u) and efl_sincos_angle(v) for every k.
tests/golden/box_muller_domain.json (made by tests/golden/make_box_muller_golden.py) holds one
SHA-256 per 65,536 consecutive k of the little-endian float32 bytes of v, sn and cs, so a GPU test
compares the device with the host header bit for bit over every angle without a compiler and without
a 96 MiB fixture. Shared by tests/test_box_muller_domain_host.py and
tests/test_box_muller_domain_gpu.py; the references are computed once per process.
"""
from __future__ import annotations

import functools
import hashlib
import json
import os
import subprocess

import numpy as np

from oracle import mask
from test_dp_gpu import ULP_TOL, ulps          # noqa: F401  (the project's stated tolerance and distance)

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(TESTS, "golden")
FIXTURE = os.path.join(GOLDEN, "box_muller_domain.json")
CSRC = os.path.join(os.path.dirname(TESTS), "elastic-federated-learning-solution_amd", "csrc")

BITS = 23
N = 1 << BITS                       # uniforms Uint32ToFloat can produce
MASK = N - 1
CHUNK = 1 << 16
CHUNKS = N // CHUNK                 # 128
HIGH = 0xFF800000                   # the nine bits of a word that Uint32ToFloat drops
QUARTER = 0x200000                  # u = 0.25: the angle float(pi / 2), where the header's sin is 1.0
HALF = 0x400000                     # u = 0.5: the radius of the every-angle sweep
MULTIPLIERS = (0x9E3779B1, 0x85EBCA6B)
R_CLAMP_BITS = 0x40B5AFA8           # the radius at the clamp u1 = 1e-7 (box_muller_math.h kRClampBits)


# ---- the word sets ------------------------------------------------------------------------------
def all_k() -> np.ndarray:
    return np.arange(N, dtype=np.uint32)


def radius_words():
    """Every radius at the angle of u = 0.25: (x0, x1)."""
    return all_k(), np.full(N, QUARTER, np.uint32)


def angle_words():
    """Every angle at the radius of u = 0.5: (x0, x1)."""
    return np.full(N, HALF, np.uint32), all_k()


def paired_words(multiplier: int):
    """Both marginals completely: x0 = k, x1 = (k multiplier) mod 2^23 (a bijection: odd multiplier)."""
    k = all_k()
    return k, ((k.astype(np.uint64) * np.uint64(multiplier)) & np.uint64(MASK)).astype(np.uint32)


def is_bijection(x: np.ndarray) -> bool:
    return x.size == N and int(x.max()) == MASK and bool((np.bincount(x, minlength=N) == 1).all())


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the references -----------------------------------------------------------------------------
def radius_f64(x0) -> np.ndarray:
    """sqrt(-2 ln max(U(x0), 1e-7)) in float64 from the float32 uniform, rounded once to float32."""
    u1 = np.maximum(mask.word_uniform(x0), np.float32(1.0e-7)).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)).astype(np.float32)


@functools.lru_cache(None)
def oracle_radius() -> np.ndarray:
    """The oracle's float chain radius for every k (it does not depend on the angle's word)."""
    r = mask.normal_from_words(*radius_words())[0]
    r.setflags(write=False)
    return r


@functools.lru_cache(None)
def oracle_paired(multiplier: int):
    """The oracle's (z0, z1) of paired_words(multiplier)."""
    out = mask.normal_from_words(*paired_words(multiplier))[3:]
    for a in out:
        a.setflags(write=False)
    return out


# ---- the host build of csrc/sincos_angle.h ------------------------------------------------------
PROG = r"""
#include <stdint.h>
#include <stdio.h>
#include "sincos_angle.h"
#define CHUNK 65536u
static float v[CHUNK], s[CHUNK], c[CHUNK];
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* fv = fopen(argv[1], "wb");
  FILE* fs = fopen(argv[2], "wb");
  FILE* fc = fopen(argv[3], "wb");
  if (!fv || !fs || !fc) return 3;
  for (uint32_t k0 = 0; k0 < (1u << 23); k0 += CHUNK) {
    for (uint32_t j = 0; j < CHUNK; ++j) {
      const float u = (float)(k0 + j) * (1.0f / 8388608.0f);   /* Uint32ToFloat of the word k0 + j */
      v[j] = efl_box_muller_angle(u);
      efl_sincos_angle(v[j], &s[j], &c[j]);
    }
    if (fwrite(v, 4, CHUNK, fv) != CHUNK || fwrite(s, 4, CHUNK, fs) != CHUNK || fwrite(c, 4, CHUNK, fc) != CHUNK)
      return 4;
  }
  return fclose(fv) | fclose(fs) | fclose(fc) ? 5 : 0;
}
"""


def host_header_tables(workdir) -> dict:
    """{"v", "sn", "cs"}: float32 [2^23] arrays of the header compiled for the host, indexed by k."""
    workdir = str(workdir)
    src, exe = os.path.join(workdir, "bm_tables.c"), os.path.join(workdir, "bm_tables")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, src, "-lm"])
    paths = {name: os.path.join(workdir, name + ".f32") for name in ("v", "sn", "cs")}
    subprocess.check_call([exe, paths["v"], paths["sn"], paths["cs"]], timeout=300)
    out = {}
    for name, p in paths.items():
        out[name] = np.fromfile(p, dtype="<f4")
        assert out[name].size == N
        os.remove(p)
    return out


def chunk_digests(a: np.ndarray) -> list:
    """SHA-256 of the little-endian float32 bytes of each of the 128 chunks of 65,536 values."""
    b = np.ascontiguousarray(a, dtype="<f4")
    assert b.size == N
    return [hashlib.sha256(b[i:i + CHUNK].tobytes()).hexdigest() for i in range(0, N, CHUNK)]


def fixture_doc(tables: dict) -> dict:
    """What tests/golden/box_muller_domain.json holds, from host_header_tables()."""
    q = {name: "%08x" % int(bits(tables[name][QUARTER:QUARTER + 1])[0]) for name in ("v", "sn", "cs")}
    return {"about": "csrc/sincos_angle.h compiled for the host (gcc -O2 -ffp-contract=off) over all 2^23 "
                     "u = k 2^-23: SHA-256 of the little-endian float32 bytes of the angle v, sin v and cos v "
                     "per chunk of 65,536 consecutive k; made by make_box_muller_golden.py. `quarter` holds "
                     "the float32 bits at k = 0x200000 (u = 0.25).",
            "chunk": CHUNK, "chunks": CHUNKS, "quarter": q,
            "digests": {name: chunk_digests(tables[name]) for name in ("v", "sn", "cs")}}


@functools.lru_cache(None)
def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)
