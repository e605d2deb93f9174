#!/usr/bin/env python3
"""ECDH PSI throughput on one MI355X (efl.psi.EccSigner): X25519 per second of
efl_x25519 and efl_x25519_hash at n = 2048 (the reference's join batch), 65,536 and 2^20, kernel
time between HIP events on the launch stream after a warm-up launch. One JSON line per n into
profiles/psi/bench_ecdh.jsonl (--out), each with

  * mads_per_element: the v_mad_u64_u32 instructions one element's k_x25519 issues, counted from the
    kernel's own loops in the built library's disassembly (255 passes of the ladder loop, the
    inversion's squaring loops with their trip counts, and the straight-line rest), and
    mad_peak_frac = issued per second over the measured v_mad_u64_u32 issue rate (3.1722e13
    lane-ops/s).
  * a CPU baseline from the same run: 16 processes, one batch each, through libcrypto's X25519
    (EVP_PKEY_derive, ctypes) where the library loads, otherwise through a g++ build of
    csrc/fe25519.h; cpu_baseline names which.

The 2^20 line also times, in the same process, the 2048-bit RSA sign (tools/bench_psi.py counts its
mads) and reports half_rate_check: the X25519 rate over half of (RSA sign rate x RSA mads / X25519
mads), i.e. against half the per-mad throughput of a kernel known to issue at 0.92. At or above 1
the check holds.

    python tools/bench_ecdh.py [--out PATH] [--sizes 2048,65536,1048576]
"""
import argparse
import ctypes
import ctypes.util
import hashlib
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "elastic-federated-learning-solution_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAD_U64_U32_PEAK = 3.1722e13
CPU_PROCS = 16
INVERT_RUNS = (5, 10, 20, 10, 50, 100, 50, 5)     # fe25519.h invert(): the sqr_n loops in program order
SECRET = hashlib.sha256(b"bench_ecdh secret").digest()


# ---- what the kernel issues ---------------------------------------------------------------------
def mads_per_element():
    """v_mad_u64_u32 per element of k_x25519 from the library's disassembly, and the parts."""
    import test_isa_guard as isa
    texts = [subprocess.check_output([isa.OBJDUMP, "-d", "--mcpu=gfx950", p]).decode() for p in _code_objects(isa)]
    ins = isa.kernel_instructions(texts, "k_x25519")
    loops = sorted(isa.backward_loops(ins))
    mad = lambda lp: isa.loop_mix(ins, lp)["v_mad_u64_u32"]
    ladder = max(loops, key=mad)
    runs = [lp for lp in loops if lp != ladder]
    assert len(runs) == len(INVERT_RUNS), (len(runs), loops)
    total = sum(1 for _, op, _ in ins if op == "v_mad_u64_u32")
    straight = total - mad(ladder) - sum(mad(lp) for lp in runs)
    issued = 255 * mad(ladder) + sum(n * mad(lp) for n, lp in zip(INVERT_RUNS, runs)) + straight
    return issued, {"ladder_step_mads": mad(ladder), "ladder_step_instructions": ladder[1] - ladder[0] + 1,
                    "squaring_loop_mads": mad(runs[0]), "squaring_loop_instructions": runs[0][1] - runs[0][0] + 1,
                    "straight_line_mads": straight, "kernel_instructions": len(ins)}


def _code_objects(isa):
    d = tempfile.mkdtemp(prefix="ecdh_isa")
    paths = []
    for k, blob in enumerate(isa.code_objects(isa.LIB)):
        p = os.path.join(d, f"co{k}.o")
        with open(p, "wb") as f:
            f.write(blob)
        paths.append(p)
    return paths


# ---- CPU baseline ---------------------------------------------------------------------------
FE_HOST = r"""
#include "fe25519.h"
extern "C" void batch(const unsigned char* k, const unsigned char* u, unsigned char* out, long n) {
  for (long i = 0; i < n; ++i) efl::fe::x25519(out + 32 * i, k, u + 32 * i);
}
"""


def load_crypto():
    for name in ("libcrypto.so.3", ctypes.util.find_library("crypto")):
        if not name:
            continue
        try:
            c = ctypes.CDLL(name)
            c.EVP_PKEY_new_raw_private_key.restype = ctypes.c_void_p
            c.EVP_PKEY_new_raw_public_key.restype = ctypes.c_void_p
            c.EVP_PKEY_CTX_new.restype = ctypes.c_void_p
            c.EVP_PKEY_new_raw_private_key.argtypes = c.EVP_PKEY_new_raw_public_key.argtypes = \
                [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
            c.EVP_PKEY_CTX_new.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            c.EVP_PKEY_derive_init.argtypes = c.EVP_PKEY_CTX_free.argtypes = c.EVP_PKEY_free.argtypes = [ctypes.c_void_p]
            c.EVP_PKEY_derive_set_peer.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            c.EVP_PKEY_derive.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]
            return c
        except (OSError, AttributeError):
            continue
    return None


def build_fe_host():
    d = tempfile.mkdtemp(prefix="ecdh_host")
    src, so = os.path.join(d, "fe_host.cpp"), os.path.join(d, "libfe_host.so")
    with open(src, "w") as f:
        f.write(FE_HOST)
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"), src, "-o", so])
    return so


def cpu_worker(args):
    """Seconds one process takes for its batch of (secret, points): one X25519 per point, as the
    reference's list comprehension around make_shared does per core."""
    kind, so, points, want_last = args
    if kind == "libcrypto":
        c = load_crypto()
        X25519 = 1034                                   # EVP_PKEY_X25519 (NID_X25519)
        prv = c.EVP_PKEY_new_raw_private_key(X25519, None, SECRET, 32)
        out = ctypes.create_string_buffer(32)
        t0 = time.perf_counter()
        for u in points:
            pub = c.EVP_PKEY_new_raw_public_key(X25519, None, u, 32)
            ctx = c.EVP_PKEY_CTX_new(prv, None)
            n = ctypes.c_size_t(32)
            ok = c.EVP_PKEY_derive_init(ctx) == 1 and c.EVP_PKEY_derive_set_peer(ctx, pub) == 1 and \
                c.EVP_PKEY_derive(ctx, out, ctypes.byref(n)) == 1
            c.EVP_PKEY_CTX_free(ctx)
            c.EVP_PKEY_free(pub)
            assert ok
        dt = time.perf_counter() - t0
        last = out.raw
    else:
        lib = ctypes.CDLL(so)
        buf = b"".join(points)
        out = ctypes.create_string_buffer(len(buf))
        t0 = time.perf_counter()
        lib.batch(SECRET, buf, out, ctypes.c_long(len(points)))
        dt = time.perf_counter() - t0
        last = out.raw[-32:]
    assert want_last is None or last == want_last
    return dt, last


def cpu_baseline(per=4000):
    crypto = load_crypto()
    kind, so = ("libcrypto", None) if crypto is not None else ("fe25519.h", build_fe_host())
    # points: sha256 digests, as sign_hash makes them (none of low order)
    jobs = [(kind, so, [hashlib.sha256(b"%d/%d" % (p, i)).digest() for i in range(per)], None) for p in range(CPU_PROCS)]
    with multiprocessing.get_context("fork").Pool(CPU_PROCS) as pool:
        pool.map(cpu_worker, [(kind, so, j[2][:2], None) for j in jobs])      # start the workers first
        t0 = time.perf_counter()
        res = pool.map(cpu_worker, jobs, chunksize=1)
        wall = time.perf_counter() - t0
    label = ("libcrypto X25519 (EVP_PKEY_derive, ctypes)" if kind == "libcrypto" else "g++ -O3 build of csrc/fe25519.h") + \
        f", {CPU_PROCS} processes"
    return CPU_PROCS * per / wall, label, (jobs[0][2][-1], res[0][1])


# ---- GPU ------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi", "bench_ecdh.jsonl"))
    ap.add_argument("--sizes", default="2048,65536,1048576")
    ap.add_argument("--no-rsa", action="store_true", help="skip the RSA sign of the half-rate check")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]

    issued, parts = mads_per_element()
    # the CPU column first: its processes are forked before this one touches the GPU
    cpu_per_s, cpu_label, (cpu_u, cpu_out) = cpu_baseline()

    import torch
    import efl
    import bench_psi
    dev = efl.lib.require_gpu()
    lib = efl.lib.raw()
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream

    def timed(fn, reps):
        fn()                                   # warm-up (and the code object's first load)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / 1e3 / reps

    # the GPU and the CPU column compute the same function
    got = efl.psi.ecc_cipher.x25519(SECRET, torch.frombuffer(bytearray(cpu_u), dtype=torch.uint8).reshape(1, 32))
    assert got.numpy().tobytes() == cpu_out, "GPU and CPU baseline disagree"

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    for N in sizes:
        g = torch.Generator(device=dev).manual_seed(N)
        u = torch.randint(0, 256, (N, 32), dtype=torch.uint8, device=dev, generator=g)
        r = torch.empty_like(u)
        reps = 20 if N <= 65536 else 3
        t_x = timed(lambda: efl.lib.check(lib.efl_x25519(SECRET, u.data_ptr(), r.data_ptr(), N, sh)), reps)
        ids = [b"id_%012d" % i for i in range(N)]
        chars, offs = efl.psi.ecc_cipher.pack_strings(ids)
        chars, offs = chars.to(dev), offs.to(dev)
        t_h = timed(lambda: efl.lib.check(lib.efl_x25519_hash(SECRET, b"curve25519", 10, chars.data_ptr(),
                                                              offs.data_ptr(), r.data_ptr(), N, sh)), reps)
        # the timed launch signs correctly: spot-check rows against the single-row path
        want = efl.psi.EccSigner(SECRET).sign_list([hashlib.sha256(b"curve25519" + i).digest() for i in ids[:3]])
        assert efl.psi.ecc_cipher.bytes_from_rows(r[:3]) == want
        rec = {"elements": N, "x25519_per_s": round(N / t_x), "x25519_hash_per_s": round(N / t_h),
               "x25519_ms": round(t_x * 1e3, 4), "x25519_hash_ms": round(t_h * 1e3, 4),
               "mads_per_element": issued, **parts,
               "mad_peak_frac": round(issued * N / t_x / MAD_U64_U32_PEAK, 4),
               "cpu_baseline": cpu_label, "cpu_x25519_per_s": round(cpu_per_s, 1),
               "gpu_over_cpu": round(N / t_x / cpu_per_s, 1), "library": efl.lib.version()}
        assert rec["mad_peak_frac"] <= 1.0, rec
        del u, chars, offs
        if N == max(sizes) and not args.no_rsa:
            # the 2048-bit RSA sign at the same element count, in this process
            with open(os.path.join(ROOT, "tests", "golden", "rsa_kat.json")) as f:
                k = next(k for k in json.load(f)["keys"] if k["name"] == "openssl-2048")
            k = {f: int(k[f], 16) for f in "nedpq"}
            key = efl.psi.RsaKey.private(k["n"], k["e"], k["d"], k["p"], k["q"])
            W = key.words
            x = torch.randint(-2 ** 31, 2 ** 31, (N, W), dtype=torch.int32, device=dev, generator=g)
            s = torch.empty_like(x)
            t_rsa = timed(lambda: efl.lib.check(lib.efl_rsa_sign(key._h, x.data_ptr(), s.data_ptr(), N, sh)), 2)
            rsa_mads = bench_psi.sign_products(k)[0]
            bar = 0.5 * (N / t_rsa) * rsa_mads / issued
            rec.update({"rsa2048_sign_per_s": round(N / t_rsa), "rsa2048_sign_ms": round(t_rsa * 1e3, 3),
                        "rsa2048_mads_per_element": rsa_mads,
                        "rsa2048_mad_peak_frac": round(rsa_mads * N / t_rsa / MAD_U64_U32_PEAK, 4),
                        "half_rate_bar_per_s": round(bar), "half_rate_check": round(N / t_x / bar, 3),
                        "half_rate_check_holds": bool(N / t_x >= bar)})
            del x, s, key
        del r
        torch.cuda.empty_cache()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    out.close()


if __name__ == "__main__":
    main()
