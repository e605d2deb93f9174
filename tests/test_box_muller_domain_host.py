"""CPU: the Box-Muller domain's fixture and references (tests/box_muller_domain.py).

* tests/golden/box_muller_domain.json is csrc/sincos_angle.h's: the digests are regenerated with gcc
  and compared with the committed ones.
* The reference alone stays inside the gates tests/test_box_muller_domain_gpu.py applies to the
  device. The kernel's normals are held to ULP_TOL = 4 of the oracle's (tests/test_dp_gpu.py). Over
  all 2^23 radii, each paired with an angle by a bijection:
  - the oracle's radius (float32 log, product and sqrt in a chain) is at most 1 ulp from the float64
    radius rounded once;
  - the header's sin / cos times the oracle's own radius is at most 2 ulp from the oracle's normal;
  so a device radius within 1 ulp of the oracle's leaves the normal within 3 ulp (measured: a radius
  2 ulp off reaches 5), which is why the GPU test gates the radius at 1 ulp.
* The clamp u1 < 1e-7 takes exactly one k, k = 0, and its radius is kRClampBits.
* efl_dp_box_muller checks its arguments before any HIP call.
"""
import ctypes
import json

import numpy as np
import pytest

import box_muller_domain as bm
from oracle import mask


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    return bm.host_header_tables(tmp_path_factory.mktemp("box_muller"))


def test_fixture_is_the_headers(tables):
    with open(bm.FIXTURE) as f:
        committed = json.load(f)
    assert bm.fixture_doc(tables) == committed
    assert committed["chunks"] == 128 and all(len(committed["digests"][k]) == 128 for k in ("v", "sn", "cs"))
    assert committed["quarter"]["sn"] == "3f800000"         # the every-radius sweep reads z0 = r there


def test_angle_table_is_the_oracles_angle(tables):
    v = (2.0 * np.pi * mask.word_uniform(bm.all_k()).astype(np.float64)).astype(np.float32)
    assert np.array_equal(bm.bits(tables["v"]), bm.bits(v))


def test_pairings_are_bijections():
    for m in bm.MULTIPLIERS:
        x0, x1 = bm.paired_words(m)
        assert bm.is_bijection(x0) and bm.is_bijection(x1)
        assert not np.array_equal(x0, x1)
    assert not bm.is_bijection(bm.radius_words()[1])


def test_clamp_has_one_k_and_its_radius():
    u = mask.word_uniform(bm.all_k())
    assert np.nonzero(u < np.float32(1.0e-7))[0].tolist() == [0]
    r = bm.oracle_radius()
    assert int(bm.bits(r[:1])[0]) == bm.R_CLAMP_BITS
    assert int(bm.bits(r[1:2])[0]) != bm.R_CLAMP_BITS
    # the words' high nine bits do not reach the uniform
    k = np.array([0, 1, bm.HALF, bm.MASK], np.uint32)
    assert np.array_equal(mask.word_uniform(k | np.uint32(bm.HIGH)), mask.word_uniform(k))


def test_oracle_radius_within_1ulp_of_float64():
    r = bm.oracle_radius()
    d = bm.ulps(r, bm.radius_f64(bm.all_k()))
    assert d.max() <= 1, np.bincount(d)
    assert (np.diff(r.astype(np.float64)) <= 0).all()       # non-increasing in k, as the device's must be


@pytest.mark.parametrize("multiplier", bm.MULTIPLIERS)
def test_header_sincos_with_oracle_radius_within_2ulp(tables, multiplier):
    x0, x1 = bm.paired_words(multiplier)
    r = bm.oracle_radius()[x0]
    z0, z1 = bm.oracle_paired(multiplier)
    d0 = bm.ulps((tables["sn"][x1] * r).astype(np.float32), z0)
    d1 = bm.ulps((tables["cs"][x1] * r).astype(np.float32), z1)
    assert d0.max() <= 2 and d1.max() <= 2, (np.bincount(d0), np.bincount(d1))
    assert 2 < bm.ULP_TOL


def test_normal_is_philox_plus_normal_from_words():
    w = mask.philox_blocks(99, 17, 3)
    want = np.empty((3, 4), np.float32)
    for a, b in ((0, 1), (2, 3)):
        r, sn, cs, z0, z1 = mask.normal_from_words(w[:, a], w[:, b])
        want[:, a], want[:, b] = z0, z1
        assert np.array_equal(bm.bits(z0), bm.bits(sn * r)) and np.array_equal(bm.bits(z1), bm.bits(cs * r))
    assert np.array_equal(bm.bits(mask.normal(99, 17, 11)), bm.bits(want.reshape(-1)[:11]))


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    p = ctypes.c_void_p(64)
    assert lib.efl_dp_box_muller(p, p, -1, 0, None, None, None, p, p, None) == -3
    assert "negative" in lib.efl_last_error().decode()
    for nb in (-1, 3, 5, 8):
        assert lib.efl_dp_box_muller(p, p, 4, nb, None, None, None, p, p, None) == -3
        assert "nb must be" in lib.efl_last_error().decode()
    assert lib.efl_dp_box_muller(None, None, 0, 4, None, None, None, None, None, None) == 0      # empty: no-op
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.efl_dp_box_muller(args[0], args[1], 4, 2, p, p, p, args[2], args[3], None) == -3
        assert "null buffer" in lib.efl_last_error().decode()
    odd = ctypes.c_void_p(66)
    assert lib.efl_dp_box_muller(p, p, 4, 1, odd, None, None, p, p, None) == -3
    assert "4-byte aligned" in lib.efl_last_error().decode()
