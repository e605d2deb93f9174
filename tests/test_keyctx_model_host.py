"""CPU: the key context's model and enumeration (tests/keyctx_model.py) cover what they claim to, by
property: every reachable (state, operation) pair is taken, the orders that matter are in the set,
the two budgets do what their names say for both keys, and the model refuses an order that would
pass its budget. The orders that need no device are also run against the library itself."""
import ctypes
import itertools
import os

import pytest

import keyctx_model as km

CAP = km.CONTEXT_CAP
DV, BUDGETS, DEPTH3, WALKS = km.plan(CAP)

# what the alphabet must hold at the least; an operation taken out of ALPHABET fails here
REQUIRED = {
    ("set_public", "A"), ("set_public", "B"), ("set_keypair", "A"), ("set_keypair", "B"),
    ("set_private", "pq"), ("set_private", "qp"), ("set_private", "other"), ("rekey_refused",),
    ("prepare", "table"), ("prepare", "crt"), ("encrypt", "owner"), ("encrypt", "public"), ("encrypt", "hsa"),
    ("fbpowm", "owner"), ("fbpowm", "public"), ("decrypt",), ("window", 0), ("window", km.WINDOW_SMALL),
    ("crt_encrypt", 0), ("crt_encrypt", 1), ("budget", "binding"), ("budget", "roomy"),
    ("fail_build", 1), ("fail_build", 0),
}


def steps_of(seq):
    """(state before, operation, expectation, state after) of every step of `seq`."""
    m = km.Model(DV, BUDGETS, CAP)
    out = []
    for op in seq:
        s = m.state()
        e = m.apply(op)
        out.append((s, op, e, m.state()))
    return out


@pytest.fixture(scope="module")
def taken():
    return [steps_of(seq) for seq in itertools.chain(DEPTH3, WALKS)]


def test_alphabet_and_keys():
    assert REQUIRED <= set(km.ALPHABET) and len(set(km.ALPHABET)) == len(km.ALPHABET)
    a, b = DV.keys["A"], DV.keys["B"]
    assert (a.n_bytes, a.ln, b.n_bytes, b.ln) == (64, 16, 128, 32)          # the two smallest, two limb classes
    assert all(v["g"] == 1 for k in (a, b) for v in k.vectors) and min(len(a.vectors), len(b.vectors)) >= 11
    # the 1024-bit key's primes sit in the half-length class: its owner encrypts by CRT; the 512-bit
    # key's 256-bit primes need the class of n itself, so it never does (and the model says so)
    assert b.crt_class and not a.crt_class
    # other-key primes take both ways of efl_pl_set_private: a new block (a wider class) and in place
    assert km.limb_class(2 * b.p.bit_length()) != a.ln and km.limb_class(2 * a.p.bit_length()) <= b.ln


def test_mirrors_match_the_package():
    import efl  # noqa: F401
    from efl.privacy import paillier_cipher as pc
    for mine, theirs in ((km.PlKey, pc.PlKey), (km.PlCtxInfo, pc.PlCtxInfo)):
        assert ctypes.sizeof(mine) == ctypes.sizeof(theirs)
        assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_]
    named = set(km.TABLE_FIELDS + km.SUBKEY_FIELDS + km.PRIVATE_FIELDS)
    assert named <= {n for n, _ in km.PlKey._fields_}


def test_budgets_bind_and_do_not():
    """Binding: for both keys, releasing the n^2 table gives the sub-tables a strictly wider window
    than keeping it (ensure_crt's w_drop > w_keep). Roomy: it does not. Both a few MiB, and every
    window small. A change to the window rule cannot turn the release path off silently."""
    for name in ("A", "B"):
        keep, drop = km.release_windows(DV, name, BUDGETS["binding"], CAP)
        assert drop > keep >= 1, (name, keep, drop)
        keep, drop = km.release_windows(DV, name, BUDGETS["roomy"], CAP)
        assert drop == keep >= 1, (name, keep, drop)
        assert drop <= 10
    assert (1 << 20) <= BUDGETS["binding"] < BUDGETS["roomy"] <= (8 << 20)
    # and the model takes the release in the order ADVICE r6 names, and does not under the roomy budget
    s = steps_of(km.RELEASE_ORDER)
    assert s[1][3].has_table and s[2][3].has_table and s[2][3].private
    assert not s[3][3].has_table and s[3][3].crt == 1 and s[3][3].private
    s = steps_of(km.RELEASE_ORDER[1:])
    assert s[2][3].has_table and s[2][3].crt == 1


def test_every_reachable_state_and_operation_is_taken(taken):
    trans, dist = km.reachable_pairs(DV, BUDGETS, CAP)
    got = {(s, op) for steps in taken for s, op, _, _ in steps}
    missing = set(trans) - got
    assert not missing, (len(missing), sorted(missing, key=repr)[:5])
    assert max(dist.values()) < km.WALK_LENGTH
    assert all(len(w) <= km.WALK_LENGTH for w in WALKS) and all(len(s) == 3 for s in DEPTH3)
    assert len(DEPTH3) == len(set(DEPTH3)) and set(DEPTH3) <= set(itertools.product(km.ALPHABET, repeat=3))
    # every outcome the context documents is reached
    assert {e.rc for steps in taken for _, _, e, _ in steps} == {0, 1, km.INVALID, km.EXHAUSTED, km.ABORTED}
    assert {s.crt for s in dist} == {0, 1, -1}


def test_the_orders_that_matter_are_there(taken):
    seqs = set(WALKS)
    want = km.RELEASE_ORDER + (("decrypt",),)
    assert any(w[:len(want)] == want for w in seqs)
    failed = lambda e: e.rc == km.EXHAUSTED and e.phrase == "fault injection"      # noqa: E731
    after_failed = {steps[i + 1][1] for steps in taken for i in range(len(steps) - 1) if failed(steps[i][2])}
    assert after_failed == set(km.ALPHABET)
    # ... also after a failed CRT sub-table build, which the context answers with "no CRT" (0)
    after_crt = {steps[i + 1][1] for steps in taken for i in range(len(steps) - 1)
                 if steps[i][0].fail_build and steps[i][0].crt == 0 and steps[i][3].crt == -1}
    assert after_crt == set(km.ALPHABET)
    # re-key to the other key, by both calls, while the n^2 table and while the CRT sub-tables are held
    rekeys = {(op[0], s.has_table, s.crt == 1) for steps in taken for s, op, e, t in steps
              if op[0] in ("set_public", "set_keypair") and s.key and s.key != op[1] and e.rc == 0}
    assert rekeys >= {(c, True, False) for c in ("set_public", "set_keypair")} | \
        {(c, False, True) for c in ("set_public", "set_keypair")}
    # a refused private key and a refused re-key on a live key, in every kind of state
    assert any(op == ("set_private", "other") and s.key and s.crt == 1 for steps in taken for s, op, _, _ in steps)
    assert any(op == ("rekey_refused",) and s.key and s.has_table for steps in taken for s, op, _, _ in steps)


def test_model_refuses_an_order_over_its_budget():
    seq = (("set_keypair", "B"), ("encrypt", "owner"), ("prepare", "table"), ("budget", "binding"))
    m, steps = km.run_model(DV, BUDGETS, CAP, seq[:3])
    assert BUDGETS["binding"] < m.held <= BUDGETS["roomy"]
    with pytest.raises(km.OverBudget):
        km.run_model(DV, BUDGETS, CAP, seq)
    for steps in (steps_of(s) for s in WALKS):
        m = km.Model(DV, BUDGETS, CAP)
        for _, op, _, _ in steps:
            m.apply(op)
            assert m.held <= BUDGETS[m.budget]


def test_orders_without_a_device_match_the_library(monkeypatch):
    """No key can be set without a device, so every order of three operations other than a valid
    set_public / set_keypair runs on the host alone: return codes, error phrases and the query."""
    lib = km.load_library()
    monkeypatch.delenv("EFL_PL_FAIL_TABLE_BUILD", raising=False)
    ops = [op for op in km.ALPHABET if op[0] not in ("set_public", "set_keypair")]
    used = km.i64(0)
    prev = lib.efl_pl_table_budget(-1, ctypes.byref(used))
    a = DV.keys["A"]

    def call(h, op):
        kind = op[0]
        if kind == "set_private":
            p, q = km.private_args(DV.keys, None, op[1])
            return lib.efl_pl_set_private(h, km.hx(p), km.hx(q), None)
        if kind == "rekey_refused":
            return lib.efl_pl_set_public(h, b"zz", 128, b"5", 64, 1, None)
        if kind == "prepare":
            return lib.efl_pl_ctx_prepare(h, km.PREPARE_TABLE if op[1] == "table" else km.PREPARE_CRT, None)
        if kind == "window":
            return lib.efl_pl_ctx_options(h, -2, op[1], -2)
        if kind == "crt_encrypt":
            return lib.efl_pl_ctx_options(h, -2, -1, op[1])
        if kind == "budget":
            lib.efl_pl_table_budget(used.value + BUDGETS[op[1]], None)
            return 0
        if kind == "fail_build":
            os.environ.pop("EFL_PL_FAIL_TABLE_BUILD", None)
            if op[1]:
                os.environ["EFL_PL_FAIL_TABLE_BUILD"] = "1"
            return 0
        flags = km.PUBLIC_PATH if op[-1] == "public" else 0
        if kind == "encrypt":
            return lib.efl_pl_ctx_encrypt(h, None, None, None, len(a.vectors), 0, 0, flags, None)
        if kind == "fbpowm":
            return lib.efl_pl_ctx_fbpowm(h, None, None, len(a.vectors), 0, 0, flags, None)
        return lib.efl_pl_ctx_decrypt(h, None, None, None, len(a.vectors), None)

    try:
        for seq in itertools.product(ops, repeat=3):
            h = km.vp()
            assert lib.efl_pl_ctx_create(ctypes.byref(h)) == 0
            try:
                lib.efl_pl_table_budget(used.value + BUDGETS["roomy"], None)
                os.environ.pop("EFL_PL_FAIL_TABLE_BUILD", None)
                m = km.Model(DV, BUDGETS, CAP)
                for op in seq:
                    rc, e = call(h, op), m.apply(op)
                    assert rc == e.rc and (rc >= 0 or e.phrase in lib.efl_last_error().decode()), (seq, op, rc, e)
                    info = km.PlCtxInfo()
                    assert lib.efl_pl_ctx_query(h, ctypes.byref(info)) == 0
                    assert (info.has_public, info.generation, m.key) == (0, 0, None)
            finally:
                assert lib.efl_pl_ctx_destroy(h) == 0
    finally:
        lib.efl_pl_table_budget(prev, None)
        os.environ.pop("EFL_PL_FAIL_TABLE_BUILD", None)


def test_mismatched_primes_are_refused_on_the_host():
    """The derivation refuses a prime that does not divide n (both ways round between the two keys),
    and takes each key's own primes in either order with the same result."""
    lib = km.load_library()
    for pub, prv in (("A", "B"), ("B", "A")):
        k, (p, q) = DV.keys[pub], DV.keys[prv].given
        words, d = km.i64(0), km.PlKey()
        rc = lib.efl_pl_key_derive(km.hx(k.n), km.hx(k.hs), k.a_bits // 8, 1, km.hx(p), km.hx(q), None, 1, 1 << 40,
                                   None, ctypes.byref(words), ctypes.byref(d))
        assert rc == km.INVALID and b"does not fit the public key" in lib.efl_last_error()
    for name in ("A", "B"):
        k = DV.keys[name]
        assert k.p * k.q == k.n and k.q < 2 * k.p
