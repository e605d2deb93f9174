"""GPU: the Paillier key context (csrc/keyset.hip) against its model (tests/keyctx_model.py) over
every order of up to three of its calls from the fresh context and fixed-seed walks of fourteen that
take every reachable (state, operation) pair. Raw ctypes on libefl_hip.so, torch for device buffers.

After EVERY step everything observable is compared with the model: the return code and the error
text's phrase; efl_pl_ctx_query; the device bytes of the key block and the CRT sub-blocks
(efl_pl_ctx_copy) and the descriptors of efl_pl_ctx_key, word for word against efl_pl_key_derive;
the known answers of GMP (tests/golden/paillier_kat.json) through every route the state allows,
decryption through the context and through the stateless entry point on the freshly fetched block;
the process budget's bytes in use; the generation counter. A block pointer is fetched again after
every step and never used past the step that fetched it.

A history seen before in this process (the first steps of the depth-3 orders repeat) is compared on
the return code, the query, the budget, the keys and the generation only: its device bytes and
answers were compared, after the same calls from a fresh context, the first time."""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

import keyctx_model as km

pytestmark = pytest.mark.gpu

CAP = km.CONTEXT_CAP
WALK_CHUNK = 50
KNOWN_RC = {0, 1, km.INVALID, km.EXHAUSTED, km.PRECONDITION, km.ABORTED}
FAIL_ENV = "EFL_PL_FAIL_TABLE_BUILD"

DV, BUDGETS, DEPTH3, WALKS = km.plan(CAP)
WALK_CHUNKS = km.chunks(WALKS, WALK_CHUNK)


class Broken(Exception):
    """A return code no model outcome explains (a HIP error): nothing more runs on the device."""


def words(vals, L):
    return np.stack([np.frombuffer(int(v).to_bytes(4 * L, "little"), "<u4") for v in vals])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view("<u4")


def stream():
    return torch.cuda.current_stream().cuda_stream


class Operands:
    """One key's known-answer operands on the device and the answers as words."""

    def __init__(self, k: km.Key):
        vs, ln = k.vectors, k.ln
        self.N, self.ln = len(vs), ln
        self.ms = [v["m"] for v in vs]
        self.m = torch.tensor(self.ms, dtype=torch.int64, device="cuda")
        self.hsa = dev(words([int(v["hsa"], 16) for v in vs], 2 * ln))
        self.a = dev(words([int(v["a"], 16) for v in vs], (k.a_bits + 31) // 32))
        self.c = dev(words([int(v["c"], 16) for v in vs], 2 * ln))
        self.want_c = words([int(v["c"], 16) for v in vs], 2 * ln)
        self.want_hsa = words([int(v["hsa"], 16) for v in vs], 2 * ln)
        self.want_fresh = words([k.fresh_ciphertext(m, km.SEED, km.COUNTER + i) for i, m in enumerate(self.ms)],
                                2 * ln)
        self.want_mag = words([abs(m) for m in self.ms], ln)
        self.want_neg = np.array([m < 0 for m in self.ms], dtype=np.int8)

    def out(self, L):
        return torch.empty((self.N, L), dtype=torch.int32, device="cuda")


class Harness:
    def __init__(self):
        self.lib = km.load_library()
        self.keys = DV.keys
        self.ops = {n: Operands(k) for n, k in self.keys.items()}
        self.seen = set()               # histories whose device bytes and answers were compared
        self.broken = None
        self.steps = self.full = 0
        used = km.i64(0)
        self.prev_budget = self.lib.efl_pl_table_budget(-1, ctypes.byref(used))
        self.in_use0 = used.value
        self.prev_fail = os.environ.pop(FAIL_ENV, None)
        self.prev_crt = os.environ.pop("EFL_PL_CRT_ENCRYPT", None)

    def restore(self):
        self.lib.efl_pl_table_budget(self.prev_budget, None)
        for name, v in ((FAIL_ENV, self.prev_fail), ("EFL_PL_CRT_ENCRYPT", self.prev_crt)):
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v

    def in_use(self):
        used = km.i64(0)
        self.lib.efl_pl_table_budget(-1, ctypes.byref(used))
        return used.value - self.in_use0

    def set_budget(self, mode):
        self.lib.efl_pl_table_budget(self.in_use0 + BUDGETS[mode], None)

    def err(self):
        return self.lib.efl_last_error().decode()

    # -- one operation ---------------------------------------------------------------------------
    def call(self, h, model: km.Model, op):
        """Run `op` on context h (model: the state before it); (rc, mismatch in its output or None)."""
        L, kind = self.lib, op[0]
        name = model.key or "A"
        k, o = self.keys[name], self.ops[name]
        if kind in ("set_public", "set_keypair"):
            k = self.keys[op[1]]
            if kind == "set_public":
                return L.efl_pl_set_public(h, km.hx(k.n), k.n_bytes, km.hx(k.hs), k.a_bits // 8, 1, stream()), None
            p, q = k.given
            return L.efl_pl_set_keypair(h, km.hx(k.n), k.n_bytes, km.hx(k.hs), k.a_bits // 8, 1, km.hx(p), km.hx(q),
                                        stream()), None
        if kind == "set_private":
            p, q = km.private_args(self.keys, model.key, op[1])
            return L.efl_pl_set_private(h, km.hx(p), km.hx(q), stream()), None
        if kind == "rekey_refused":
            return L.efl_pl_set_public(h, b"zz", 128, b"5", 64, 1, stream()), None
        if kind == "prepare":
            return L.efl_pl_ctx_prepare(h, km.PREPARE_TABLE if op[1] == "table" else km.PREPARE_CRT, stream()), None
        if kind == "window":
            return L.efl_pl_ctx_options(h, -2, op[1], -2), None
        if kind == "crt_encrypt":
            return L.efl_pl_ctx_options(h, -2, -1, op[1]), None
        if kind == "budget":
            self.set_budget(op[1])
            return 0, None
        if kind == "fail_build":
            os.environ.pop(FAIL_ENV, None)
            if op[1]:
                os.environ[FAIL_ENV] = "1"
            return 0, None
        flags = km.PUBLIC_PATH if len(op) > 1 and op[1] == "public" else 0
        if kind == "encrypt":
            ct = o.out(2 * o.ln)
            given = op[1] == "hsa"
            rc = L.efl_pl_ctx_encrypt(h, o.m.data_ptr(), o.hsa.data_ptr() if given else None, ct.data_ptr(), o.N,
                                      km.SEED, km.COUNTER, flags, stream())
            bad = None
            if rc == 0 and not np.array_equal(host(ct), o.want_c if given else o.want_fresh):
                bad = "ciphertexts differ from " + ("the known answers" if given else "g(m) hs^a of the Philox stream")
            return rc, bad
        if kind == "fbpowm":
            out = o.out(2 * o.ln)
            rc = L.efl_pl_ctx_fbpowm(h, o.a.data_ptr(), out.data_ptr(), o.N, 0, 0, flags, stream())
            return rc, ("hs^a differs from the known answers" if rc == 0 and not np.array_equal(host(out), o.want_hsa)
                        else None)
        if kind == "decrypt":
            mag, neg = o.out(o.ln), torch.empty(o.N, dtype=torch.int8, device="cuda")
            rc = L.efl_pl_ctx_decrypt(h, o.c.data_ptr(), mag.data_ptr(), neg.data_ptr(), o.N, stream())
            ok = rc != 0 or (np.array_equal(host(mag), o.want_mag) and np.array_equal(neg.cpu().numpy(), o.want_neg))
            return rc, None if ok else "plaintexts differ from the known answers"
        raise ValueError(op)

    # -- everything observable -------------------------------------------------------------------
    def observe(self, h, m: km.Model, prev, full):
        """Compare the context with model m; prev = (generation, keys) of the step before. Returns
        the new (generation, keys). AssertionError names the first difference."""
        L = self.lib
        info = km.PlCtxInfo()
        assert L.efl_pl_ctx_query(h, ctypes.byref(info)) == 0
        got = {f: km.field_value(info, f) for f, _ in km.PlCtxInfo._fields_}
        gen = got.pop("generation")
        assert got.pop("table_max_bytes") == CAP
        blocks = [got.pop("block_bytes")] + list(got.pop("crt_block_bytes"))
        if m.key is None:
            want = dict.fromkeys(got, 0)
            want["crt_table_window"] = want["crt_table_bytes"] = (0, 0)
        else:
            k = m.k
            want = dict(has_public=1, has_private=int(bool(m.private)), n_bytes=k.n_bytes, ln=k.ln, a_bits=k.a_bits,
                        group_size=1, table_window=m.W, has_table=int(m.has_table), crt_capable=int(m.crt_capable),
                        crt=m.crt, crt_table_window=m.sub_W, table_bytes=m.main_bytes, crt_table_bytes=m.sub_bytes)
        assert got == want, f"query: {({f: (got[f], want[f]) for f in got if got[f] != want[f]})} (got, model)"
        # the budget: what the process holds is what this context's tables take, within the budget
        used = self.in_use()
        assert used == got["table_bytes"] + sum(got["crt_table_bytes"]) == m.held, (used, m.held)
        assert used <= BUDGETS[m.budget], (used, m.budget)
        # the keys, fetched again after every step; the generation
        keys = []
        for which in range(3):
            ptr, d = km.vp(), km.PlKey()
            rc = L.efl_pl_ctx_key(h, which, ctypes.byref(ptr), ctypes.byref(d))
            want_rc = km.ABORTED if m.key is None else km.PRECONDITION if which and m.crt != 1 else 0
            assert rc == want_rc, f"efl_pl_ctx_key({which}) = {rc}, model {want_rc}: {self.err()}"
            keys.append((ptr.value, km.desc_fields(d), d) if rc == 0 else None)
        now = [(x[0], x[1]) if x else None for x in keys]
        assert gen >= prev[0], f"generation went back: {prev[0]} -> {gen}"
        assert now == prev[1] or gen > prev[0], \
            f"a pointer or descriptor of efl_pl_ctx_key changed and the generation stayed {gen}"
        if m.key is not None and full:
            self.full += 1
            self.compare_blocks(h, m, keys, blocks)
            self.answers(h, m, keys[0])
            after = km.PlCtxInfo()
            assert L.efl_pl_ctx_query(h, ctypes.byref(after)) == 0 and after.generation == gen, "the checks moved a block"
        return gen, now

    def read(self, h, which, count):
        out = np.empty(count, dtype="<u4")
        rc = self.lib.efl_pl_ctx_copy(h, which, 0, count, out.ctypes.data, stream())
        assert rc == 0, (rc, self.err())
        torch.cuda.synchronize()
        return out

    def compare_blocks(self, h, m, keys, blocks):
        k = m.k
        D = DV.main(m.key, m.private, m.W)
        hw = len(D.head)
        head = self.read(h, 0, hw)
        diff = np.flatnonzero(head != D.head)
        assert diff.size == 0, (f"key block: {diff.size} head words differ from the derivation, first at word "
                                f"{diff[0]} (private span from word {self.private_start(D)})")
        self.compare_desc("key", keys[0][2], D.desc, hw, m.has_table, k.a_bits, m.W)
        assert blocks[0] == 4 * hw + m.main_bytes, (blocks[0], hw, m.main_bytes)
        if m.crt != 1:
            assert blocks[1:] == [0, 0]
            return
        for i in range(2):
            S = DV.sub(m.key, i, m.sub_W[i], m.private)
            L28 = S.desc.n2_28_len
            want = np.concatenate([S.head, DV.sub_extra(m.key, i, L28, m.private)]) if L28 else S.head
            head = self.read(h, i + 1, len(want))
            diff = np.flatnonzero(head != want)
            assert diff.size == 0, f"CRT sub-block {i + 1}: {diff.size} head words differ, first at word {diff[0]}"
            d = keys[i + 1][2]
            assert (d.off_gn28, d.off_gstart28) == ((len(S.head), len(S.head) + L28) if L28 else (-1, -1))
            self.compare_desc(f"sub-key {i + 1}", d, S.desc, len(want), True, k.a_bits, m.sub_W[i],
                              skip=km.SUBKEY_FIELDS)
            assert blocks[i + 1] == 4 * len(want) + m.sub_bytes[i]

    @staticmethod
    def private_start(D):
        return D.desc.off_p if D.desc.has_private else -1

    @staticmethod
    def compare_desc(what, d, want, hw, has_table, a_bits, W, skip=()):
        skip = km.TABLE_FIELDS + tuple(skip)
        a, b = km.desc_fields(d, skip), km.desc_fields(want, skip)
        assert a == b, f"{what} descriptor: {({f: (a[f], b[f]) for f in a if a[f] != b[f]})} (got, derived)"
        rows, cols, lc, L28 = -(-a_bits // W), (1 << W) - 1, 2 * want.ln, want.n2_28_len
        table = (rows, hw, hw + rows * cols * lc if L28 else -1) if has_table else (0, -1, -1)
        assert (d.table_rows, d.off_table, d.off_table28) == table, (what, "table fields", table)

    def answers(self, h, m, key0):
        L, o = self.lib, self.ops[m.key]
        ct = o.out(2 * o.ln)
        rc = L.efl_pl_ctx_encrypt(h, o.m.data_ptr(), o.hsa.data_ptr(), ct.data_ptr(), o.N, 0, 0, 0, stream())
        assert rc == 0 and np.array_equal(host(ct), o.want_c), f"encryption with the known hsa ({rc})"
        for route in m.routes_ready():
            flags = km.PUBLIC_PATH if route == "public" else 0
            out = o.out(2 * o.ln)
            rc = L.efl_pl_ctx_fbpowm(h, o.a.data_ptr(), out.data_ptr(), o.N, 0, 0, flags, stream())
            assert rc == 0 and np.array_equal(host(out), o.want_hsa), f"fbpowm on the {route} route ({rc})"
            rc = L.efl_pl_ctx_encrypt(h, o.m.data_ptr(), None, out.data_ptr(), o.N, km.SEED, km.COUNTER, flags, stream())
            assert rc == 0 and np.array_equal(host(out), o.want_fresh), f"fresh encryption on the {route} route ({rc})"
        mag, neg = o.out(o.ln), torch.empty(o.N, dtype=torch.int8, device="cuda")
        rc = L.efl_pl_ctx_decrypt(h, o.c.data_ptr(), mag.data_ptr(), neg.data_ptr(), o.N, stream())
        if not m.private:
            assert rc == km.ABORTED and "No private key." in self.err(), (rc, self.err())
            return
        assert rc == 0, f"decryption: {rc} {self.err()}"
        assert np.array_equal(host(mag), o.want_mag) and np.array_equal(neg.cpu().numpy(), o.want_neg), "decryption"
        mag2, neg2 = o.out(o.ln), torch.empty(o.N, dtype=torch.int8, device="cuda")
        rc = L.efl_pl_decrypt(key0[0], ctypes.byref(key0[2]), o.c.data_ptr(), mag2.data_ptr(), neg2.data_ptr(), o.N,
                              stream())
        assert rc == 0, f"stateless decryption on the fetched block: {rc} {self.err()}"
        assert np.array_equal(host(mag2), o.want_mag) and np.array_equal(neg2.cpu().numpy(), o.want_neg), \
            "stateless decryption on the fetched block"

    # -- one sequence ------------------------------------------------------------------------------
    def run(self, seq):
        """None, or what differed first: (step, operation, message)."""
        L = self.lib
        m = km.Model(DV, BUDGETS, CAP)
        h = km.vp()
        assert L.efl_pl_ctx_create(ctypes.byref(h)) == 0
        step, op = -1, None
        try:
            self.set_budget(m.budget)
            os.environ.pop(FAIL_ENV, None)
            assert L.efl_pl_ctx_options(h, CAP, -1, -2) == 0
            prev = self.observe(h, m, (0, [None] * 3), False)
            for step, op in enumerate(seq):
                self.steps += 1
                rc, bad = self.call(h, m, op)
                if rc not in KNOWN_RC:
                    self.broken = f"{seq[:step + 1]}: return code {rc}: {self.err()}"
                    raise Broken(self.broken)
                e = m.apply(op)
                assert rc == e.rc, f"return code {rc} ({self.err() if rc < 0 else ''}), model {e.rc}"
                assert e.phrase in self.err() or rc >= 0, f"error text {self.err()!r} lacks {e.phrase!r}"
                assert bad is None, bad
                history = seq[:step + 1]
                full = history not in self.seen
                prev = self.observe(h, m, prev, full)
                self.seen.add(history)
        except AssertionError as ex:
            return step, op, str(ex)
        finally:
            os.environ.pop(FAIL_ENV, None)
            assert L.efl_pl_ctx_destroy(h) == 0
            left = self.in_use()
            self.set_budget("roomy")
        assert left == 0, f"{left} bytes still accounted after efl_pl_ctx_destroy"
        return None


@pytest.fixture(scope="module")
def harness():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hs = Harness()
    yield hs
    hs.restore()
    print(f"\nkey context model: {hs.steps} steps, {hs.full} compared in full")


def run_all(harness, seqs):
    if harness.broken:
        pytest.fail("stopped after " + harness.broken)
    t0 = time.perf_counter()
    failures = []
    for seq in seqs:
        r = harness.run(seq)
        if r is not None:
            failures.append((seq, r))
    dt = time.perf_counter() - t0
    print(f"{len(seqs)} sequences, {sum(map(len, seqs))} steps, {dt:.2f} s, {len(failures)} differ")
    lines = [f"{' '.join(km.op_id(o) for o in seq)}\n    step {st + 1} ({km.op_id(op) if op else 'fresh'}): {msg}"
             for seq, (st, op, msg) in failures[:8]]
    assert not failures, f"{len(failures)} of {len(seqs)} sequences differ from the model:\n" + "\n".join(lines)


@pytest.mark.parametrize("first", km.ALPHABET, ids=km.op_id)
def test_every_order_of_three_calls(harness, first):
    """Every order of three operations that starts with `first`, each step compared with the model."""
    run_all(harness, [s for s in DEPTH3 if s[0] == first])


@pytest.mark.parametrize("chunk", range(len(WALK_CHUNKS)))
def test_walks_over_every_state_and_operation(harness, chunk):
    """Fixed-seed walks of fourteen operations (together they take every reachable (state, operation)
    pair of the model: tests/test_keyctx_model_host.py), each step compared with the model."""
    run_all(harness, WALK_CHUNKS[chunk])
