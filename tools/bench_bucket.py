#!/usr/bin/env python3
"""Bucket hash and partition on one MI355X (efl.psi.bucket): efl_mmh3_hash,
efl_bucket_ids, efl_bucket_partition and efl_strings_gather over 2^20 decimal IDs of 16 characters and
64 buckets (the reference's default), the work both parties of a data-join do before any record is
signed. Kernel time between HIP events on the launch stream after a warm-up call, through the C ABI on
caller-owned buffers. One JSON line per step into profiles/psi/bench_bucket.jsonl (--out), each with

  * ms, rows per second, the bytes the step has to move (computed from the shapes below) and that
    rate as a fraction of the HBM peak (8.0 TB/s);
  * the same work on the host twin in the same run: the hash through efl_mmh3_hash_rows_host with 1
    and with 16 threads (the `mmh3` module is not installed, so the twin is the baseline; it is the
    same C++ the golden file pins), the bucket ids, the stable sort and the regrouping through numpy
    on one thread (numpy has no threaded form of them);
  * on the last line: the four steps together, beside the time efl_x25519_hash takes to sign the
    same IDs in the same run.

    python tools/bench_bucket.py [--out PATH] [--rows 1048576] [--buckets 64] [--reps 20]
"""
import argparse
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "elastic-federated-learning-solution_amd")
sys.path.insert(0, PKG)

HBM_PEAK = 8.0e12
ID_LEN = 16
SECRET = hashlib.sha256(b"bench_bucket secret").digest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi", "bench_bucket.jsonl"))
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--buckets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    N, B, reps = args.rows, args.buckets, args.reps

    import torch
    import efl
    dev = efl.lib.require_gpu()
    lib = efl.lib.raw()
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    check = efl.lib.check

    def timed(fn):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / 1e3 / reps

    def host_timed(fn, times=3):
        best = None
        for _ in range(times):
            t0 = time.perf_counter()
            fn()
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        return best

    # 2^20 distinct 16-digit decimal IDs from a seeded generator
    rng = np.random.default_rng(20)
    values = rng.permutation(N).astype(np.int64) * 7919 + 10 ** 15
    h_chars = np.frombuffer("".join("%016d" % v for v in values.tolist()).encode(), dtype=np.uint8).copy()
    h_offsets = np.arange(N + 1, dtype=np.int64) * ID_LEN
    chars, offsets = torch.from_numpy(h_chars).to(dev), torch.from_numpy(h_offsets).to(dev)
    hashes = torch.empty(N, dtype=torch.int32, device=dev)
    bucket = torch.empty(N, dtype=torch.int32, device=dev)
    order = torch.empty(N, dtype=torch.int64, device=dev)
    starts = torch.empty(B + 1, dtype=torch.int64, device=dev)
    out_chars, out_offsets = torch.empty_like(chars), torch.empty_like(offsets)
    p_bytes, g_bytes = int(lib.efl_bucket_scratch_bytes(N, B)), int(lib.efl_strings_gather_scratch_bytes(N))
    p_scratch = torch.empty((p_bytes + 7) // 8, dtype=torch.int64, device=dev)
    g_scratch = torch.empty((g_bytes + 7) // 8, dtype=torch.int64, device=dev)

    def do_hash():
        check(lib.efl_mmh3_hash(chars.data_ptr(), offsets.data_ptr(), N, 0, hashes.data_ptr(), sh))

    def do_ids():
        check(lib.efl_bucket_ids(hashes.data_ptr(), N, B, 1, bucket.data_ptr(), sh))

    def do_partition():
        check(lib.efl_bucket_partition(bucket.data_ptr(), N, B, order.data_ptr(), starts.data_ptr(), p_scratch.data_ptr(),
                                       p_scratch.numel() * 8, sh))

    def do_gather():
        check(lib.efl_strings_gather(chars.data_ptr(), offsets.data_ptr(), order.data_ptr(), N, out_chars.data_ptr(),
                                     out_offsets.data_ptr(), g_scratch.data_ptr(), g_scratch.numel() * 8, sh))

    def do_all():
        do_hash(), do_ids(), do_partition(), do_gather()

    # the host twin
    t_hashes = np.empty(N, dtype=np.int32)

    def host_hash(threads):
        def work(lo, hi):
            lib.efl_mmh3_hash_rows_host(h_chars.ctypes.data, h_offsets.ctypes.data + 8 * lo, hi - lo, 0,
                                        t_hashes.ctypes.data + 4 * lo)
        cuts = [N * k // threads for k in range(threads + 1)]
        ts = [threading.Thread(target=work, args=(cuts[k], cuts[k + 1])) for k in range(threads)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    twin = {}

    def host_ids():
        twin["bucket"] = (t_hashes.astype(np.int64) % B).astype(np.int32)

    def host_partition():
        twin["order"] = np.argsort(twin["bucket"], kind="stable")
        twin["starts"] = np.concatenate([[0], np.cumsum(np.bincount(twin["bucket"], minlength=B))])

    def host_gather():
        twin["chars"] = h_chars.reshape(N, ID_LEN)[twin["order"]].reshape(-1)

    t_hash_1, t_hash_16 = host_timed(lambda: host_hash(1)), host_timed(lambda: host_hash(16))
    t_ids_h, t_part_h, t_gather_h = host_timed(host_ids), host_timed(host_partition), host_timed(host_gather)

    # the device against the twin, then the timings
    do_all()
    torch.cuda.synchronize()
    assert np.array_equal(hashes.cpu().numpy(), t_hashes), "hash differs from the host twin"
    assert np.array_equal(bucket.cpu().numpy(), twin["bucket"]), "bucket ids differ"
    assert np.array_equal(order.cpu().numpy(), twin["order"]) and np.array_equal(starts.cpu().numpy(), twin["starts"])
    assert np.array_equal(out_chars.cpu().numpy(), twin["chars"]) and np.array_equal(out_offsets.cpu().numpy(), h_offsets)

    steps = [
        # (name, fn, bytes the step must move, host seconds on 1 thread)
        ("mmh3_hash", do_hash, N * ID_LEN + 8 * (N + 1) + 4 * N, t_hash_1),
        ("bucket_ids", do_ids, 8 * N, t_ids_h),
        ("partition", do_partition, 4 * N * 2 + 8 * N + 8 * (B + 1), t_part_h),
        ("gather", do_gather, 8 * N + 8 * (N + 1) + N * ID_LEN + N * ID_LEN + 8 * (N + 1), t_gather_h),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(rec):
        rec["library"] = efl.lib.version()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    total = 0.0
    for name, fn, nbytes, t_host in steps:
        t = timed(fn)
        total += t
        rec = {"step": name, "rows": N, "id_bytes": ID_LEN, "buckets": B, "calls_timed": reps, "ms": round(t * 1e3, 4),
               "rows_per_s": round(N / t), "bytes": nbytes, "bytes_per_s": round(nbytes / t),
               "hbm_peak_frac": round(nbytes / t / HBM_PEAK, 4), "host_1_thread_ms": round(t_host * 1e3, 3),
               "over_host_1_thread": round(t_host / t, 1)}
        if name == "mmh3_hash":
            rec.update({"host_16_threads_ms": round(t_hash_16 * 1e3, 3), "over_host_16_threads": round(t_hash_16 / t, 1)})
        emit(rec)
    t_all = timed(do_all)
    signed = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    t_sign = timed(lambda: check(lib.efl_x25519_hash(SECRET, b"curve25519", 10, chars.data_ptr(), offsets.data_ptr(),
                                                      signed.data_ptr(), N, sh)))
    host_all = t_hash_1 + t_ids_h + t_part_h + t_gather_h
    emit({"step": "all four", "rows": N, "id_bytes": ID_LEN, "buckets": B, "calls_timed": reps,
          "ms": round(t_all * 1e3, 4), "sum_of_steps_ms": round(total * 1e3, 4), "rows_per_s": round(N / t_all),
          "host_1_thread_ms": round(host_all * 1e3, 3), "host_16_thread_hash_ms": round((host_all - t_hash_1 + t_hash_16) * 1e3, 3),
          "x25519_hash_ms": round(t_sign * 1e3, 4), "share_of_signing": round(t_all / t_sign, 4)})
    out.close()


if __name__ == "__main__":
    main()
