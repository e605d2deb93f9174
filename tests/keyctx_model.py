"""A model of the Paillier key context (csrc/keyset.hip, efl_pl_ctx_*) and the orders of its calls,
for tests (a plain helper, no fixtures, no GPU, no efl import).

The context is a state machine over device memory: a main key block with or without its n^2
fixed-base table, a private span written in place, two CRT sub-blocks, a process-wide byte budget
and a generation counter. `Model` restates its transitions over plain Python values: for every
operation of `ALPHABET` it gives the return code, the key phrase of the error text and the next
state. Where an outcome depends on a table window (keep or release the n^2 table, room for the CRT
sub-tables or not) the model asks the library's own rule, efl_pl_choose_window, with the entry
sizes efl_pl_key_derive reports; it does not restate the formula. Both calls run on the CPU.

`plan()` lists every order of up to three operations from the fresh context, fixed-seed walks of
fourteen that take every reachable (state, operation) pair at least once, and a few named orders.
tests/test_keyctx_model_host.py proves those properties; tests/test_keyctx_model_gpu.py runs every
sequence on the device and compares everything observable with the model after every step.
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import json
import os
import random
from typing import NamedTuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "elastic-federated-learning-solution_amd", "efl", "libefl_hip.so")

OK, INVALID, EXHAUSTED, PRECONDITION, ABORTED = 0, -3, -8, -9, -10
PREPARE_TABLE, PREPARE_CRT, PUBLIC_PATH = 1, 2, 1
N_VECTORS = 12                      # known-answer vectors (g == 1) run after every step
WINDOW_SMALL = 3                    # the explicit window of the `window` operation
SEED, COUNTER = 0x5EED0123456789AB, (1 << 32) - 5      # the fresh-randomness stream of the checks
WALK_LENGTH, WALK_SEED = 14, 20261020   # the deepest model states lie 12 steps from the fresh context
CONTEXT_CAP = 1 << 20               # per-context table cap the tests give every context (efl_pl_ctx_options)

vp, i32, i64, u64, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_char_p


class PlKey(ctypes.Structure):
    """ctypes mirror of efl_pl_key (include/efl_hip.h); the host test holds it against the package's."""
    _fields_ = [(n, ctypes.c_int32) for n in ("ln", "a_bits", "group_size", "table_rows", "table_cols",
                                               "has_private", "pm1_bits", "qm1_bits")] + \
               [(n, ctypes.c_uint32) for n in ("n2_minv", "p2_minv", "q2_minv", "p_minv", "q_minv")] + \
               [(n, ctypes.c_int64) for n in ("off_n", "off_n2", "off_n2_r2", "off_n2_one", "off_table", "off_max",
                                               "off_p", "off_q", "off_p2", "off_q2", "off_p2_r3", "off_q2_r3",
                                               "off_pm1", "off_qm1", "off_pinv_w", "off_qinv_w", "off_hp",
                                               "off_hq", "off_qinvp")] + \
               [("p2_28_len", ctypes.c_int32), ("p2_minv28", ctypes.c_uint32), ("q2_minv28", ctypes.c_uint32),
                ("off_p2_28", ctypes.c_int64), ("off_q2_28", ctypes.c_int64),
                ("off_p2_r2_28", ctypes.c_int64 * 6), ("off_q2_r2_28", ctypes.c_int64 * 6),
                ("n2_28_len", ctypes.c_int32), ("table28_log2g", ctypes.c_int32), ("n2_minv28", ctypes.c_uint32),
                ("off_n2_28", ctypes.c_int64), ("off_n2_one28", ctypes.c_int64), ("off_table28", ctypes.c_int64),
                ("off_n2_r2_28", ctypes.c_int64), ("table_window", ctypes.c_int32),
                ("off_gn28", ctypes.c_int64), ("off_gstart28", ctypes.c_int64)]


class PlCtxInfo(ctypes.Structure):
    """ctypes mirror of efl_pl_ctx_info."""
    _fields_ = [(n, ctypes.c_int32) for n in ("has_public", "has_private", "n_bytes", "ln", "a_bits", "group_size",
                                               "table_window", "has_table", "crt_capable", "crt")] + \
               [("crt_table_window", ctypes.c_int32 * 2)] + \
               [(n, ctypes.c_int64) for n in ("block_bytes", "table_bytes", "table_max_bytes")] + \
               [("crt_block_bytes", ctypes.c_int64 * 2), ("crt_table_bytes", ctypes.c_int64 * 2),
                ("generation", ctypes.c_uint64)]


# the descriptor fields the library documents as changing with the table (efl_pl_key: off_table,
# off_table28 are -1 and table_rows 0 until a table is attached); every other field, and every head
# word, is compared with the derivation. The sub-keys' two per-element walk-start constants are
# appended by the context after the derived head; the test computes them itself.
TABLE_FIELDS = ("off_table", "off_table28", "table_rows")
SUBKEY_FIELDS = ("off_gn28", "off_gstart28")
PRIVATE_FIELDS = ("has_private", "pm1_bits", "qm1_bits", "p2_minv", "q2_minv", "p_minv", "q_minv", "off_p", "off_q",
                  "off_p2", "off_q2", "off_p2_r3", "off_q2_r3", "off_pm1", "off_qm1", "off_pinv_w", "off_qinv_w",
                  "off_hp", "off_hq", "off_qinvp", "p2_28_len", "p2_minv28", "q2_minv28", "off_p2_28", "off_q2_28",
                  "off_p2_r2_28", "off_q2_r2_28")


def field_value(d, name):
    v = getattr(d, name)
    return tuple(v) if hasattr(v, "__len__") else v


def desc_fields(d, skip=()):
    return {n: field_value(d, n) for n, _ in PlKey._fields_ if n not in skip}


def load_library(path=None):
    """libefl_hip.so through ctypes with the signatures of the key context (EFL_HIP_LIB names another
    build of the same library, as for the package)."""
    L = ctypes.CDLL(path or os.environ.get("EFL_HIP_LIB") or DEFAULT_LIB)
    PK = ctypes.POINTER(PlKey)
    sig = {
        "efl_pl_ctx_create": [ctypes.POINTER(vp)], "efl_pl_ctx_destroy": [vp],
        "efl_pl_ctx_options": [vp, i64, i32, i32],
        "efl_pl_set_public": [vp, cp, i32, cp, i32, i32, vp], "efl_pl_set_private": [vp, cp, cp, vp],
        "efl_pl_set_keypair": [vp, cp, i32, cp, i32, i32, cp, cp, vp],
        "efl_pl_ctx_key": [vp, i32, ctypes.POINTER(vp), PK], "efl_pl_ctx_prepare": [vp, i32, vp],
        "efl_pl_ctx_query": [vp, ctypes.POINTER(PlCtxInfo)], "efl_pl_ctx_copy": [vp, i32, i64, i64, vp, vp],
        "efl_pl_ctx_encrypt": [vp, vp, vp, vp, i64, u64, i64, i32, vp],
        "efl_pl_ctx_fbpowm": [vp, vp, vp, i64, u64, i64, i32, vp],
        "efl_pl_ctx_decrypt": [vp, vp, vp, vp, i64, vp],
        "efl_pl_decrypt": [vp, PK, vp, vp, vp, i64, vp],
        "efl_pl_choose_window": [i32, i64, i64],
        "efl_pl_key_derive": [cp, cp, i32, i32, cp, cp, cp, i32, i64, vp, ctypes.POINTER(i64), PK],
    }
    for name, args in sig.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = i32
    L.efl_pl_table_budget.argtypes = [i64, ctypes.POINTER(i64)]
    L.efl_pl_table_budget.restype = i64
    L.efl_last_error.restype = cp
    return L


def limb_class(bits):
    return next(c for c in (16, 32, 64, 128, 256) if 32 * c >= bits)


def hx(v):
    return format(int(v), "x").encode()


class Key:
    """One known-answer key of tests/golden/paillier_kat.json with its g == 1 vectors."""

    def __init__(self, name, k):
        self.name = name
        self.n, self.hs, p, q = (int(k[f], 16) for f in ("n", "hs", "p", "q"))
        self.given = (p, q)                                    # the fixture's order
        self.p, self.q = self.ordered("pq")
        self.n_bytes, self.a_bits = k["n_bytes"], k["a_bits"]
        self.ln = limb_class(self.n.bit_length())
        self.vectors = [v for v in k["vectors"] if v["g"] == 1][:N_VECTORS]
        # the key owner's encryption goes by CRT when the primes sit in the half-length limb class
        self.crt_class = all(2 * limb_class(x.bit_length()) == self.ln for x in (p, q)) and p * q == self.n

    def ordered(self, how):
        """(p, q) as the key block holds them when given in the fixture's order ("pq") or the other
        ("qp"): as given, unless q >= 2p (the CRT reduces mq mod p once)."""
        p, q = self.given if how == "pq" else self.given[::-1]
        return (q, p) if q >= 2 * p else (p, q)

    def fresh_ciphertext(self, m, seed, counter):
        """PaillierEncrypt with the randomness of Philox stream (seed, counter), group size 1
        (oracle/philox.py draws a as csrc/paillier.hip does): g(m) hs^a mod n^2 in Python integers."""
        from oracle import philox
        n2 = self.n * self.n
        a = philox.draw_a(seed, counter, self.a_bits)
        g = 1 + abs(m) * self.n
        if m < 0:
            g = pow(g, -1, n2)
        return g * pow(self.hs, a, n2) % n2

    def sub_key(self, i, how="pq"):
        """(x, hs mod x^2, walk start R (y^2)^-1 mod x^2) of CRT sub-key i (0: the block's p, 1: its q)."""
        x, y = self.ordered(how)[::1 if i == 0 else -1]
        R = 1 << (32 * 2 * self.ln)
        return x, self.hs % (x * x), R * pow(y * y, -1, x * x)


def load_keys():
    with open(os.path.join(GOLDEN, "paillier_kat.json")) as f:
        kat = json.load(f)
    by = {k["n_bytes"]: k for k in kat["keys"]}
    return {"A": Key("A", by[64]), "B": Key("B", by[128])}     # 512- and 1024-bit n: limb classes 16, 32


OTHER = {"A": "B", "B": "A"}


class Derived(NamedTuple):
    head: np.ndarray
    desc: PlKey

    @property
    def entry_bytes(self):
        return 4 * (2 * self.desc.ln + self.desc.n2_28_len)


class Deriver:
    """efl_pl_key_derive (host only), cached: the head words and descriptor of a key block."""

    def __init__(self, lib, keys):
        self.lib, self.keys = lib, keys
        self._cache = {}

    def _derive(self, n, hs, a_bits, p, q, walk, window):
        key = (n, hs, a_bits, p, q, walk, window)
        if key not in self._cache:
            words, d = i64(0), PlKey()
            args = (hx(n), hx(hs), a_bits // 8, 1, hx(p) if p else None, hx(q) if q else None,
                    hx(walk) if walk is not None else None, window, 1 << 62)
            rc = self.lib.efl_pl_key_derive(*args, None, ctypes.byref(words), ctypes.byref(d))
            assert rc == 0, (rc, self.lib.efl_last_error())
            head = np.zeros(words.value, dtype="<u4")
            rc = self.lib.efl_pl_key_derive(*args, head.ctypes.data, ctypes.byref(words), ctypes.byref(d))
            assert rc == 0, (rc, self.lib.efl_last_error())
            self._cache[key] = Derived(head, d)
        return self._cache[key]

    def main(self, name, private, window=1):
        """private: False, or the order the primes were given in ("pq" / "qp")."""
        k = self.keys[name]
        p, q = k.ordered(private) if private else (None, None)
        return self._derive(k.n, k.hs, k.a_bits, p, q, None, window)

    def sub(self, name, i, window=1, how="pq"):
        k = self.keys[name]
        x, hs, walk = k.sub_key(i, how)
        return self._derive(x, hs, k.a_bits, None, None, walk, window)

    def sub_extra(self, name, i, L28, how="pq"):
        """The two constants the context appends to sub-key i's head (efl_pl_key off_gn28,
        off_gstart28): (n mod x^2) 2^84 mod x^2 and (y^2)^-1 R28^2 mod x^2 as L28 28-bit limbs."""
        k = self.keys[name]
        x, y = k.ordered(how)[::1 if i == 0 else -1]
        x2 = x * x
        R28 = 1 << (28 * L28)
        vals = ((k.n % x2 << 84) % x2, pow(y * y, -1, x2) * (R28 * R28 % x2) % x2)
        return np.array([(v >> (28 * t)) & 0xFFFFFFF for v in vals for t in range(L28)], dtype="<u4")

    def window(self, a_bits, entry_bytes, max_bytes):
        return self.lib.efl_pl_choose_window(a_bits, entry_bytes, max(0, max_bytes))


def table_bytes(a_bits, W, entry_bytes):
    return -(-a_bits // W) * ((1 << W) - 1) * entry_bytes


# ---- the operations --------------------------------------------------------------------------------

ALPHABET = (
    ("set_public", "A"), ("set_public", "B"), ("set_keypair", "A"), ("set_keypair", "B"),
    ("set_private", "pq"), ("set_private", "qp"), ("set_private", "other"),
    ("rekey_refused",),
    ("prepare", "table"), ("prepare", "crt"),
    ("encrypt", "owner"), ("encrypt", "public"), ("encrypt", "hsa"),
    ("fbpowm", "owner"), ("fbpowm", "public"),
    ("decrypt",),
    ("window", 0), ("window", WINDOW_SMALL), ("crt_encrypt", 0), ("crt_encrypt", 1),
    ("budget", "binding"), ("budget", "roomy"),
    ("fail_build", 1), ("fail_build", 0),
)


def op_id(op):
    return "-".join(str(x) for x in op)


class Expect(NamedTuple):
    rc: int
    phrase: str = ""


class OverBudget(Exception):
    """The sequence would hold more table bytes than the budget it chooses: not a sequence to run."""


class State(NamedTuple):
    key: str | None
    private: object                 # False, or the order the primes were given in ("pq" / "qp")
    has_table: bool
    W: int                          # the n^2 table's window (planned, if not built)
    crt: int                        # 0 not tried, 1 sub-keys built, -1 not available
    sub_W: tuple
    window: int                     # options: explicit window (0: chosen)
    crt_mode: int                   # options: -1 default (on), 0 off, 1 on
    budget: str
    fail_build: bool


class Model:
    """The context's transitions. `budgets` maps "binding" / "roomy" to bytes above what the process
    held at the start; `cap` is the per-context table cap in force (EFL_PL_TABLE_MAX_MIB)."""

    def __init__(self, deriver: Deriver, budgets: dict, cap: int):
        self.dv, self.keys, self.budgets, self.cap = deriver, deriver.keys, budgets, cap
        self.key = None
        self.private = False
        self.has_table = False
        self.W = 0
        self.crt = 0
        self.sub_W = (0, 0)
        self.window = 0
        self.crt_mode = -1
        self.budget = "roomy"
        self.fail_build = False

    # -- sizes -----------------------------------------------------------------------------------
    @property
    def k(self) -> Key:
        return self.keys[self.key]

    def entry(self):
        return self.dv.main(self.key, False).entry_bytes

    def sub_entry(self, i):
        return self.dv.sub(self.key, i, 1, self.private or "pq").entry_bytes

    @property
    def main_bytes(self):
        return table_bytes(self.k.a_bits, self.W, self.entry()) if self.key and self.has_table else 0

    @property
    def sub_bytes(self):
        if self.crt != 1:
            return (0, 0)
        return tuple(table_bytes(self.k.a_bits, self.sub_W[i], self.sub_entry(i)) for i in range(2))

    @property
    def held(self):
        return self.main_bytes + sum(self.sub_bytes)

    def left(self, taken=0):
        return max(0, self.budgets[self.budget] - self.held - taken)

    def allowance(self):
        return max(0, min(self.cap, self.left()))

    def state(self) -> State:
        return State(self.key, self.private, self.has_table, self.W, self.crt, self.sub_W, self.window,
                     self.crt_mode, self.budget, self.fail_build)

    def copy(self):
        m = Model(self.dv, self.budgets, self.cap)
        (m.key, m.private, m.has_table, m.W, m.crt, m.sub_W, m.window, m.crt_mode, m.budget,
         m.fail_build) = self.state()
        return m

    @property
    def crt_capable(self):
        return bool(self.key and self.private and self.crt_mode != 0 and self.k.crt_class)

    # -- transitions (the names follow csrc/keyset.hip) -------------------------------------------
    def _clear(self):
        self.key, self.private, self.has_table, self.W, self.crt, self.sub_W = None, False, False, 0, 0, (0, 0)

    def _set_key(self, name, private):
        k = self.keys[name]
        eb = self.dv.main(name, False).entry_bytes
        room = max(0, self.budgets[self.budget])           # the old key's tables are released first
        if self.window:
            W = self.window
            if table_bytes(k.a_bits, W, eb) > room:
                return Expect(EXHAUSTED, "Memory usage exceeds")
        else:
            W = self.dv.window(k.a_bits, eb, min(self.cap, room))
            if not W:
                return Expect(EXHAUSTED, "Memory usage exceeds")
        self._clear()
        self.key, self.private, self.W = name, "pq" if private else False, W
        if not self.crt_capable:                           # the key owner's n^2 table is deferred
            if self.fail_build:
                self._clear()                              # no key at all rather than a dangling block
                return Expect(EXHAUSTED, "fault injection")
            self.has_table = True
        return Expect(OK)

    def _ensure_crt(self):
        if self.crt == 1:
            return True
        if self.crt == -1 or not self.crt_capable:
            return False
        a = self.k.a_bits
        each = self.allowance() // 2
        if self.has_table and not self.window:
            w_keep = self.dv.window(a, self.sub_entry(0), each)
            freed = max(0, min(self.cap, self.left() + self.main_bytes)) // 2
            w_drop = self.dv.window(a, self.sub_entry(0), freed)
            if w_drop > w_keep:                            # the n^2 table goes: the sub-tables get its room
                self.has_table = False
                each = self.allowance() // 2
        taken, Ws = 0, []
        for i in range(2):
            eb = self.sub_entry(i)
            W = self.window or self.dv.window(a, eb, each)
            if not W or (self.window and table_bytes(a, W, eb) > self.left(taken)) or self.fail_build:
                self.crt = -1                              # the public-key path serves
                return False
            taken += table_bytes(a, W, eb)
            Ws.append(W)
        self.crt, self.sub_W = 1, tuple(Ws)
        return True

    def _ensure_table(self):
        if self.has_table:
            return Expect(OK)
        k = self.k
        if not self.window:
            W = self.dv.window(k.a_bits, self.entry(), self.allowance())
            if not W:
                return Expect(EXHAUSTED, "Memory usage exceeds")
            self.W = W
        elif table_bytes(k.a_bits, self.W, self.entry()) > self.left():
            return Expect(EXHAUSTED, "Memory usage exceeds")
        if self.fail_build:
            return Expect(EXHAUSTED, "fault injection")  # the table-less block is put back
        self.has_table = True
        return Expect(OK)

    def _route(self, route):
        """What an encryption or exponentiation without given randomness builds before it runs."""
        if route == "owner" and self._ensure_crt():
            return Expect(OK)
        return self._ensure_table()

    def apply(self, op) -> Expect:
        kind = op[0]
        if kind == "rekey_refused":
            return Expect(INVALID, "not a hex integer")
        if kind == "window":
            self.window = op[1]
            return Expect(OK)
        if kind == "crt_encrypt":
            self.crt_mode = op[1]
            return Expect(OK)
        if kind == "fail_build":
            self.fail_build = bool(op[1])
            return Expect(OK)
        if kind == "budget":
            if self.held > self.budgets[op[1]]:
                raise OverBudget(f"{self.held} bytes held, {op[1]} budget {self.budgets[op[1]]}")
            self.budget = op[1]
            return Expect(OK)
        if kind == "set_public":
            return self._set_key(op[1], False)
        if kind == "set_keypair":
            return self._set_key(op[1], True)
        if kind == "set_private":
            if self.key is None:
                return Expect(OK)                          # ignored without a public key
            if op[1] == "other":
                return Expect(INVALID, "private key")      # refused: the old key stays as it was
            if not self.private or self.k.ordered(self.private) != self.k.ordered(op[1]):
                self.private = op[1]                       # written in place (the other order: written again)
                self.crt, self.sub_W = 0, (0, 0)           # drop_crt
            return Expect(OK)
        if self.key is None:
            return Expect(ABORTED, "No public key.")
        if kind == "prepare":
            if op[1] == "crt":
                return Expect(1 if self._ensure_crt() else 0)
            e = self._ensure_table()
            return Expect(1) if e.rc == OK else e
        if kind == "decrypt":
            return Expect(OK) if self.private else Expect(ABORTED, "No private key.")
        if kind in ("encrypt", "fbpowm"):
            return Expect(OK) if op[1] == "hsa" else self._route(op[1])
        raise ValueError(op)

    # -- what the state allows without another transition ------------------------------------------
    def routes_ready(self):
        """The routes an exponentiation can take now without building or releasing anything."""
        r = []
        if self.key and self.has_table:
            r.append("public")
        if self.key and (self.crt == 1 or (self.has_table and (self.crt == -1 or not self.crt_capable))):
            r.append("owner")
        return r


def private_args(keys, current, how):
    """(p, q) the set_private operation `how` passes while key `current` is set (A's without a key)."""
    k = keys[current or "A"]
    if how == "other":
        return keys[OTHER[k.name]].given
    p, q = k.given
    return (p, q) if how == "pq" else (q, p)


# ---- budgets ---------------------------------------------------------------------------------------

def release_windows(dv: Deriver, name, budget, cap):
    """(w_keep, w_drop) of ensure_crt for key `name` whose n^2 table set_public built under `budget`:
    the sub-tables' window beside the table, and with the table released."""
    k = dv.keys[name]
    eb, es = dv.main(name, False).entry_bytes, dv.sub(name, 0).entry_bytes
    W = dv.window(k.a_bits, eb, min(cap, budget))
    if not W:
        return None
    left = budget - table_bytes(k.a_bits, W, eb)
    return (dv.window(k.a_bits, es, min(cap, left) // 2), dv.window(k.a_bits, es, min(cap, budget) // 2))


def choose_budgets(dv: Deriver, cap, step=256 << 10, top=32 << 20):
    """The smallest budgets (multiples of 256 KiB from 1 MiB) at which, for both keys, releasing the n^2
    table widens the sub-tables' window ("binding") and at which it does not ("roomy")."""
    out = {}
    for b in range(1 << 20, top + 1, step):
        w = [release_windows(dv, name, b, cap) for name in ("A", "B")]
        if any(x is None or x[0] < 1 for x in w):
            continue
        if "binding" not in out and all(d > kp for kp, d in w):
            out["binding"] = b
        if "roomy" not in out and all(d == kp for kp, d in w):
            out["roomy"] = b
        if len(out) == 2:
            return out
    raise AssertionError(f"no binding / roomy budget up to {top} bytes: {out}")


# ---- enumeration -------------------------------------------------------------------------------------

def run_model(dv, budgets, cap, seq):
    """The model after `seq` with the expectation and state of every step; OverBudget if it cannot run."""
    m = Model(dv, budgets, cap)
    steps = []
    for op in seq:
        e = m.apply(op)
        steps.append((op, e, m.state()))
    return m, steps


def depth_sequences(dv, budgets, cap, depth=3):
    """Every order of up to `depth` operations the model can run, as maximal sequences (a shorter
    order is the prefix of a longer one, and every step of a sequence is checked)."""
    out = []
    for seq in itertools.product(ALPHABET, repeat=depth):
        try:
            run_model(dv, budgets, cap, seq)
        except OverBudget:
            continue
        out.append(seq)
    return out


def reachable_pairs(dv, budgets, cap):
    """The model's transition graph from the fresh context, by breadth-first search: {(state,
    operation): next state} over every pair the model can take, and each state's distance."""
    start = Model(dv, budgets, cap)
    dist, models, todo = {start.state(): 0}, {start.state(): start}, [start.state()]
    trans = {}
    while todo:
        nxt = []
        for s in todo:
            for op in ALPHABET:
                m = models[s].copy()
                try:
                    m.apply(op)
                except OverBudget:
                    continue
                t = m.state()
                trans[(s, op)] = t
                if t not in dist:
                    dist[t], models[t] = dist[s] + 1, m
                    nxt.append(t)
        todo = nxt
    return trans, dist


def random_walks(dv, budgets, cap, length=WALK_LENGTH, seed=WALK_SEED, limit=20000):
    """Fixed-seed random walks of `length` operations, drawn until every reachable (state, operation)
    pair is taken: each step picks at random among the operations not yet taken from the state it is
    in, or, when all are, the first step of a shortest way to a state that still has one."""
    trans, dist = reachable_pairs(dv, budgets, cap)
    todo = set(trans)
    left = {}                           # state -> operations not taken from it yet
    back = {}
    for (u, op), t in trans.items():
        left[u] = left.get(u, 0) + 1
        back.setdefault(t, []).append((u, op))
    rng = random.Random(seed)
    start = Model(dv, budgets, cap).state()
    walks = []
    hop = {}                            # state -> first operation of a shortest way to unfinished work
    stale = [True]

    def rehop():
        hop.clear()
        frontier = [u for u in dist if left[u]]         # breadth-first order: the same on every run
        seen = set(frontier)
        while frontier:
            nxt = []
            for t in frontier:
                for u, op in back.get(t, ()):
                    if u not in seen:
                        seen.add(u)
                        hop[u] = op
                        nxt.append(u)
            frontier = nxt
        stale[0] = False

    while todo and len(walks) < limit:
        s, walk = start, []
        for _ in range(length):
            fresh = [op for op in ALPHABET if (s, op) in todo]
            if fresh:
                onward = [op for op in fresh if left[trans[(s, op)]] > (trans[(s, op)] == s)]
                op = rng.choice(onward or fresh)          # rather one that leads to more untaken work
                todo.discard((s, op))
                left[s] -= 1
                stale[0] = stale[0] or not left[s]
            else:
                if stale[0]:
                    rehop()
                op = hop.get(s)
                if op is None:
                    break
            walk.append(op)
            s = trans[(s, op)]
        if not walk:
            break
        walks.append(tuple(walk))
    assert not todo, f"{len(todo)} reachable (state, operation) pairs lie deeper than walks of {length} reach"
    return walks


# the order ADVICE r6 found by reading: the public key first (its n^2 table is built), the private key
# in place, and the owner's first encryption under a budget that binds releases the table
RELEASE_ORDER = (("budget", "binding"), ("set_public", "B"), ("set_private", "pq"), ("encrypt", "owner"))


def named_sequences():
    """Orders the enumeration must hold whatever the walks draw: the release order followed by a
    decryption and by the public route, and every operation straight after each kind of failed table
    build (the deferred n^2 table's, the CRT sub-tables', and the release followed by a failed build)."""
    out = [RELEASE_ORDER + (("decrypt",), ("encrypt", "public"), ("decrypt",)),
           RELEASE_ORDER[:3] + (("set_private", "qp"), ("fbpowm", "owner"), ("decrypt",), ("set_public", "A"))]
    for op in ALPHABET:
        out.append((("set_keypair", "B"), ("fail_build", 1), ("encrypt", "public"), op, ("decrypt",)))
        out.append((("set_keypair", "B"), ("fail_build", 1), ("prepare", "crt"), op, ("decrypt",)))
        out.append(RELEASE_ORDER[:3] + (("fail_build", 1), ("prepare", "crt"), op, ("decrypt",)))
    return out


@functools.lru_cache(maxsize=None)
def _plan(lib_path, cap):
    lib = load_library(lib_path)
    dv = Deriver(lib, load_keys())
    budgets = choose_budgets(dv, cap)
    for seq in named_sequences():
        run_model(dv, budgets, cap, seq)                   # none of them may pass its budget
    return dv, budgets, depth_sequences(dv, budgets, cap), random_walks(dv, budgets, cap) + named_sequences()


def plan(cap=CONTEXT_CAP, lib_path=None):
    """(deriver, budgets, the depth-3 sequences, the walks: random and named) for the per-context cap."""
    return _plan(lib_path or os.environ.get("EFL_HIP_LIB") or DEFAULT_LIB, cap)


def chunks(seqs, size):
    return [seqs[i:i + size] for i in range(0, len(seqs), size)]
