#!/usr/bin/env python3
"""RSA blind-signature PSI throughput on one MI355X (efl.psi): signs/s, blinds/s,
unblinds/s and FDH/s at 1024-, 2048- and 4096-bit keys (the OpenSSL keys of
tests/golden/rsa_kat.json), kernel time between HIP events on the launch stream after a warm-up
launch. One JSON line per key into profiles/psi/bench_psi.jsonl (--out), each with

  * limb_products_issued: the v_mad_u64_u32 instructions one element's sign issues, counted from the
    kernels' own loops (csrc/powm28.h: the window walk over dp and dq as powm_window runs it; a CIOS
    product 2 L28^2, a one-lane squaring C (C + 1) / 2 + C^2, an SOS squaring over two lanes
    C (C + 1) + 2 C ceil(C / 2) + 2 C L28; the 32-bit products of the reduction of x and of the
    join), and mad_peak_frac = issued per second over the measured v_mad_u64_u32 issue rate
    (3.1722e13 lane-ops/s; bench.py MAD_U64_U32_PEAK). It cannot pass 1.
  * a CPU baseline from the same run: mpz_powm(x, d, n) of libgmp.so.10 through ctypes, one batch in
    each of 16 processes (what the reference's gmpy2.powmod list comprehension does per core), or
    CPython's pow when GMP does not load; cpu_baseline names which.

The 2048-bit line also times, in the same process, the 1024-bit-key Paillier decryption at the same
element count (the same modulus width and squaring method, exponents half as long) and reports
sign_over_decrypt; DESIGN.md §5e's bar for it is 0.45.

    python tools/bench_psi.py [--out PATH] [--keys 1024,2048,4096] [--n 1048576]
"""
import argparse
import ctypes
import ctypes.util
import json
import multiprocessing
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "elastic-federated-learning-solution_amd"))

MAD_U64_U32_PEAK = 3.1722e13
WINDOW = 5                     # csrc/powm28.h kWin
CPU_PROCS = 16


# ---- what the kernels issue ---------------------------------------------------------------------
def window_products(e, w=WINDOW):
    """(squarings, multiplies) of powm_window over e: the table's c^2 and 2^(w-1) - 1 products, then
    left to right, a squaring per bit and a multiply per window that ends in a 1 bit."""
    bit = lambda i: (e >> i) & 1
    b = e.bit_length() - 1
    j = max(b - w + 1, 0)
    while not bit(j):
        j += 1
    b = j - 1
    sq, mul = 1, (1 << (w - 1)) - 1
    while b >= 0:
        if not bit(b):
            sq += 1
            b -= 1
            continue
        j = max(b - w + 1, 0)
        while not bit(j):
            j += 1
        sq += b - j + 1
        mul += 1
        b = j - 1
    return sq, mul


def sign_family(L):
    """(C, G) of k_rsa_sign for primes of L words (csrc/rsa.hip sign())."""
    return {16: (8, 2), 32: (32, 1), 64: (32, 2)}[L]


def limbs28(L, G):
    return (((32 * L + 2 + 27) // 28) + G - 1) // G        # sliced28.h limbs_per_lane


def sign_products(k):
    """v_mad_u64_u32 instructions of one element's k_rsa_sign, all its lanes together."""
    n, d, p, q = k["n"], k["d"], k["p"], k["q"]
    W = 32 if n.bit_length() <= 1024 else 64 if n.bit_length() <= 2048 else 128
    L = next(c for c in (16, 32, 64) if 32 * c >= max(p.bit_length(), q.bit_length()))
    C, G = sign_family(L)
    C28 = limbs28(L, G)
    L28 = C28 * G
    cios = 2 * L28 * L28
    if G == 1:
        sqr = C28 * (C28 + 1) // 2 + C28 * C28                       # sqr_fips1
    elif G == 2 and C == 32:
        sqr = C28 * (C28 + 1) + 2 * C28 * ((C28 + 1) // 2) + 2 * C28 * L28   # sos_sqr, both lanes
    else:
        sqr = cios                                                   # mont_sqr through LDS
    phases = {"reduce": 0, "table": 0, "walk": 0, "join": 0}
    for x in (p, q):
        sq, mul = window_products(d % (x - 1))
        table = sqr + ((1 << (WINDOW - 1)) - 1) * cios
        walk = (sq - 1) * sqr + (mul - ((1 << (WINDOW - 1)) - 1)) * cios
        reduce_ = (3 if W == 2 * L else 2) * 2 * L * L + cios         # 32-bit products, then x R28
        phases["reduce"] += reduce_
        phases["table"] += table
        phases["walk"] += walk + cios                                 # and the conversion out
    phases["join"] = 3 * 2 * L * L + L * L
    total = sum(phases.values())
    return total, phases, (C, G)


# ---- CPU baseline ---------------------------------------------------------------------------
class Mpz(ctypes.Structure):
    _fields_ = [("alloc", ctypes.c_int), ("size", ctypes.c_int), ("d", ctypes.c_void_p)]


def load_gmp():
    for name in ("libgmp.so.10", ctypes.util.find_library("gmp")):
        if not name:
            continue
        try:
            g = ctypes.CDLL(name)
            g.__gmpz_init
            return g
        except (OSError, AttributeError):
            continue
    return None


def cpu_worker(args):
    d, n, xs, use_gmp = args
    if use_gmp:
        g = load_gmp()
        md, mn, mx, mo = Mpz(), Mpz(), Mpz(), Mpz()
        for m in (md, mn, mx, mo):
            g.__gmpz_init(ctypes.byref(m))
        g.__gmpz_set_str(ctypes.byref(md), format(d, "x").encode(), 16)
        g.__gmpz_set_str(ctypes.byref(mn), format(n, "x").encode(), 16)
        texts = [format(x, "x").encode() for x in xs]
        t0 = time.perf_counter()
        for t in texts:
            g.__gmpz_set_str(ctypes.byref(mx), t, 16)
            g.__gmpz_powm(ctypes.byref(mo), ctypes.byref(mx), ctypes.byref(md), ctypes.byref(mn))
        dt = time.perf_counter() - t0
        buf = ctypes.create_string_buffer(2 * (n.bit_length() // 8) + 8)
        g.__gmpz_get_str(buf, 16, ctypes.byref(mo))
        last = int(buf.value, 16)
    else:
        t0 = time.perf_counter()
        for x in xs:
            last = pow(x, d, n)
        dt = time.perf_counter() - t0
    assert last == pow(xs[-1], d, n)
    return dt


def cpu_baseline(k, use_gmp):
    """powm(x, d, n) per second over CPU_PROCS processes (each times its own batch)."""
    n, d = k["n"], k["d"]
    per = 2000 if n.bit_length() <= 1024 else 400 if n.bit_length() <= 2048 else 64   # ~0.5 s per process
    rng = random.Random(5)
    jobs = [(d, n, [rng.randrange(n) for _ in range(per)], use_gmp) for _ in range(CPU_PROCS)]
    with multiprocessing.get_context("fork").Pool(CPU_PROCS) as pool:
        pool.map(cpu_worker, [(d, n, j[2][:2], use_gmp) for j in jobs])   # start the workers first
        t0 = time.perf_counter()
        pool.map(cpu_worker, jobs, chunksize=1)
        wall = time.perf_counter() - t0
    return CPU_PROCS * per / wall


# ---- GPU ------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi", "bench_psi.jsonl"))
    ap.add_argument("--keys", default="1024,2048,4096")
    ap.add_argument("--n", type=int, default=1 << 20, help="elements at 1024 and 2048 bits (a quarter at 4096)")
    args = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "rsa_kat.json")) as f:
        kat = {k["name"]: k for k in json.load(f)["keys"]}
    keys = []
    for bits in (int(b) for b in args.keys.split(",")):
        k = kat[f"openssl-{bits}"]
        keys.append(dict(bits=bits, **{f: int(k[f], 16) for f in "nedpq"}))

    # the CPU column first: its processes are forked before this one touches the GPU
    use_gmp = load_gmp() is not None
    for k in keys:
        k["cpu_per_s"] = cpu_baseline(k, use_gmp)

    import torch
    import efl
    from efl.privacy import paillier_cipher as pc
    dev = efl.lib.require_gpu()
    lib = efl.lib.raw()
    stream = torch.cuda.current_stream(dev)

    def timed(fn, reps=2):
        fn()                                   # warm-up (and the code object's first load)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / 1e3 / reps

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    for k in keys:
        bits = k["bits"]
        N = args.n if bits <= 2048 else max(1, args.n // 4)
        key = efl.psi.RsaKey.private(k["n"], k["e"], k["d"], k["p"], k["q"])
        W = key.words
        g = torch.Generator(device=dev).manual_seed(bits)
        x = torch.randint(-2 ** 31, 2 ** 31, (N, W), dtype=torch.int32, device=dev, generator=g)
        r = torch.zeros((N, W), dtype=torch.int32, device=dev)
        r[:, :8] = torch.randint(-2 ** 31, 2 ** 31, (N, 8), dtype=torch.int32, device=dev, generator=g)
        r[:, 0] |= 1
        s = torch.empty_like(x)
        bad = torch.empty(1, dtype=torch.int64, device=dev)
        sh = stream.cuda_stream
        h = key._h
        t_sign = timed(lambda: efl.lib.check(lib.efl_rsa_sign(h, x.data_ptr(), s.data_ptr(), N, sh)))
        # the timed launch signs correctly: spot-check rows against Python
        xi = efl.psi.rsa_cipher.ints_from_rows(x[:4])
        assert efl.psi.rsa_cipher.ints_from_rows(s[:4]) == [pow(v, k["d"], k["n"]) for v in xi]
        t_blind = timed(lambda: efl.lib.check(lib.efl_rsa_blind(h, x.data_ptr(), r.data_ptr(), s.data_ptr(), N, sh)))
        t_unblind = timed(lambda: efl.lib.check(lib.efl_rsa_unblind(h, x.data_ptr(), r.data_ptr(), s.data_ptr(), N,
                                                                    bad.data_ptr(), sh)))
        ids = ["id_%012d" % i for i in range(N)]
        chars, offs = efl.psi.rsa_cipher.pack_strings(ids)
        chars, offs = chars.to(dev), offs.to(dev)
        fd = torch.empty((N, W), dtype=torch.int32, device=dev)
        t_fdh = timed(lambda: efl.lib.check(lib.efl_sha256_fdh(chars.data_ptr(), offs.data_ptr(), fd.data_ptr(), W, N,
                                                               sh)), reps=5)
        issued, phases, fam = sign_products(k)
        rec = {"key_bits": bits, "elements": N, "words": W, "sign_family_C_G": list(fam),
               "sign_per_s": round(N / t_sign), "blind_per_s": round(N / t_blind),
               "unblind_per_s": round(N / t_unblind), "fdh_per_s": round(N / t_fdh),
               "sign_ms": round(t_sign * 1e3, 3), "blind_ms": round(t_blind * 1e3, 3),
               "unblind_ms": round(t_unblind * 1e3, 3), "fdh_ms": round(t_fdh * 1e3, 3),
               "e": k["e"], "limb_products_issued": issued, "limb_products_by_phase": phases,
               "mad_peak_frac": round(issued * N / t_sign / MAD_U64_U32_PEAK, 3),
               "cpu_baseline": ("mpz_powm (libgmp.so.10, ctypes)" if use_gmp else "CPython pow") +
                               f", {CPU_PROCS} processes",
               "cpu_sign_per_s": round(k["cpu_per_s"], 1),
               "gpu_over_cpu": round(N / t_sign / k["cpu_per_s"], 1), "library": efl.lib.version()}
        assert rec["mad_peak_frac"] <= 1.0, rec
        del x, r, s, fd, chars, offs, key
        torch.cuda.empty_cache()
        if bits == 2048:
            # the 1024-bit-key Paillier decryption at the same element count, in this process
            n, hs, p, q = pc.generate_keypair_ints(128, 24, random.Random(128))
            kp = efl.paillier.Keypair(seed=7)
            kp.set_keys_ints(n, hs, 64, 10, p, q, 128)
            kb = kp.key.ensure_table()
            m = torch.randint(-2 ** 40, 2 ** 40, (N,), dtype=torch.int64, device=dev)
            ct = torch.empty((N, kb.lc), dtype=torch.int32, device=dev)
            mag = torch.empty((N, kb.ln), dtype=torch.int32, device=dev)
            neg = torch.empty(N, dtype=torch.int8, device=dev)
            efl.lib.check(lib.efl_pl_encrypt(*kb.args(), m.data_ptr(), None, ct.data_ptr(), N, 7, 0, sh))
            t_dec = timed(lambda: efl.lib.check(lib.efl_pl_decrypt(*kb.args(), ct.data_ptr(), mag.data_ptr(),
                                                                   neg.data_ptr(), N, sh)))
            ok = torch.equal(kp.decrypt(pc.CipherTensor(ct[:256], (256,), kb), dtype=torch.int64), m[:256])
            rec.update({"paillier_1024_decrypt_per_s": round(N / t_dec), "paillier_1024_decrypt_ms":
                        round(t_dec * 1e3, 3), "paillier_round_trip_ok": bool(ok),
                        "sign_over_decrypt": round(t_dec / t_sign, 3), "sign_over_decrypt_bar": 0.45})
            del m, ct, mag, neg, kp
            torch.cuda.empty_cache()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    out.close()


if __name__ == "__main__":
    main()
