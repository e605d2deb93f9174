#!/usr/bin/env python3
"""Writes tests/golden/box_muller_domain.json: the chunk digests of csrc/sincos_angle.h on the host.

The header is compiled with gcc -O2 -ffp-contract=off (as tests/test_sincos_angle.py compiles it,
which proves it within 1 ulp of the rounded sin / cos) and run over all 2^23 u = k 2^-23. For each of
the 128 chunks of 65,536 consecutive k the file holds the SHA-256 of the little-endian float32 bytes
of the angle v, of sn and of cs (tests/box_muller_domain.py has the program and the digests).
tests/test_box_muller_domain_host.py regenerates them; tests/test_box_muller_domain_gpu.py compares
the device's sn and cs with them, bit for bit over every angle.

    python tests/golden/make_box_muller_golden.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import box_muller_domain as bm      # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as d:
        doc = bm.fixture_doc(bm.host_header_tables(d))
    assert doc["quarter"]["sn"] == "3f800000", doc["quarter"]      # sin(float(pi / 2)) is 1.0 exactly
    with open(bm.FIXTURE, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    assert os.path.getsize(bm.FIXTURE) < 64 * 1024
    print(bm.FIXTURE, os.path.getsize(bm.FIXTURE), "bytes;", sum(len(v) for v in doc["digests"].values()), "digests")


if __name__ == "__main__":
    main()
