#!/usr/bin/env python3
"""The sort join's order on one MI355X (efl.psi.strsort): efl_strings_sort in both modes
over 2^20 distinct record keys `16-character id # 10-digit time` in 64 segments (the bucket of the id's
hash, the reference's default bucket count), efl_strings_run_heads over the sorted rows, and
efl_strings_search of 2^20 queries (half of them present) in a 2^20-key table. Kernel time between HIP
events on the launch stream after a warm-up call, through the C ABI on caller-owned buffers. One JSON
line per step into profiles/psi/bench_sort.jsonl (--out), each with

  * ms and rows per second on the device;
  * the same work on the host twin in the same run (efl_strings_*_host, one thread), whose result the
    device's is compared with before anything is timed;
  * for the record sort: Python's sorted(keys, key=cmp_to_key(record_cmp)) over a 2^16 subset, what
    the reference's client runs per bucket, and the device and the twin on that subset;
  * the sort at 2^11 .. 2^20 rows (--scaling), which separates the tile sort (the whole of the sort at
    2^11 rows) from the rank merges (one more launch per doubling).

    python tools/bench_sort.py [--out PATH] [--rows 1048576] [--segments 64] [--reps 10]
"""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "elastic-federated-learning-solution_amd")
sys.path.insert(0, PKG)

ID_LEN, TIME_LEN = 16, 10
KEY_LEN = ID_LEN + 1 + TIME_LEN
MODES = (("bytes", 0), ("record", 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi", "bench_sort.jsonl"))
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--subset", type=int, default=1 << 16)
    ap.add_argument("--scaling", action="store_true")
    args = ap.parse_args()
    N, B, reps = args.rows, args.segments, args.reps

    import torch
    import efl
    from efl.psi import record_cmp
    dev = efl.lib.require_gpu()
    lib = efl.lib.raw()
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    check = efl.lib.check

    def timed(fn, times=reps):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(times):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / 1e3 / times

    def host_timed(fn, times=1):
        best = None
        for _ in range(times):
            t0 = time.perf_counter()
            fn()
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        return best

    # N distinct keys from a seeded generator: a 16-digit id, '#', a 10-digit time
    rng = np.random.default_rng(21)
    ids = rng.permutation(N).astype(np.int64) * 7919 + 10 ** 15
    times = rng.integers(1_500_000_000, 1_700_000_000, size=N)
    keys = [b"%016d#%010d" % (i, t) for i, t in zip(ids.tolist(), times.tolist())]
    h_chars = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
    h_offsets = np.arange(N + 1, dtype=np.int64) * KEY_LEN
    chars, offsets = torch.from_numpy(h_chars).to(dev), torch.from_numpy(h_offsets).to(dev)
    id_chars = torch.from_numpy(h_chars.reshape(N, KEY_LEN)[:, :ID_LEN].copy().reshape(-1))
    hashes = efl.psi.mmh3_hash_rows(id_chars, torch.arange(N + 1, dtype=torch.int64) * ID_LEN)
    segment = efl.psi.DefaultKeySelector(B).get_keys(hashes=hashes)
    h_segment = segment.cpu().numpy()
    order = torch.empty(N, dtype=torch.int64, device=dev)
    heads = torch.empty(N, dtype=torch.uint8, device=dev)
    nbytes = int(lib.efl_strings_sort_scratch_bytes(N))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)

    def do_sort(mode, n=N, seg=True):
        check(lib.efl_strings_sort(chars.data_ptr(), offsets.data_ptr(), segment.data_ptr() if seg else None, n, mode,
                                   order.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, sh))

    h_order = np.empty(N, dtype=np.int64)

    def host_sort(mode, n=N, seg=True):
        assert lib.efl_strings_sort_host(h_chars.ctypes.data, h_offsets.ctypes.data, h_segment.ctypes.data if seg else None,
                                         n, mode, h_order.ctypes.data) == 0

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(rec):
        rec["library"] = efl.lib.version()
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    launches = 2 + max(0, int(np.ceil(np.log2(max(1, -(-N // 2048))))))
    for name, mode in MODES:
        t_host = host_timed(lambda: host_sort(mode))
        do_sort(mode)
        torch.cuda.synchronize()
        assert np.array_equal(order.cpu().numpy(), h_order), "the device's order differs from the host twin's"
        t = timed(lambda: do_sort(mode))
        emit({"step": "sort", "mode": name, "rows": N, "key_bytes": KEY_LEN, "segments": B, "launches": launches,
              "calls_timed": reps, "ms": round(t * 1e3, 4), "rows_per_s": round(N / t), "scratch_bytes": nbytes,
              "host_1_thread_ms": round(t_host * 1e3, 3), "over_host_1_thread": round(t_host / t, 2)})

    # the run heads of the bytes order without segments, and the search in that table
    host_sort(0, seg=False)
    t_order = torch.from_numpy(h_order.copy()).to(dev)
    do_heads = lambda: check(lib.efl_strings_run_heads(chars.data_ptr(), offsets.data_ptr(), t_order.data_ptr(), N,
                                                       heads.data_ptr(), sh))
    h_heads = np.empty(N, dtype=np.uint8)
    host_heads = lambda: lib.efl_strings_run_heads_host(h_chars.ctypes.data, h_offsets.ctypes.data, h_order.ctypes.data, N,
                                                        h_heads.ctypes.data)
    t_host = host_timed(host_heads)
    do_heads()
    torch.cuda.synchronize()
    assert np.array_equal(heads.cpu().numpy(), h_heads) and int(h_heads.sum()) == N
    t = timed(do_heads)
    emit({"step": "run_heads", "rows": N, "key_bytes": KEY_LEN, "launches": 1, "calls_timed": reps, "ms": round(t * 1e3, 4),
          "rows_per_s": round(N / t), "host_1_thread_ms": round(t_host * 1e3, 3), "over_host_1_thread": round(t_host / t, 2)})

    # N queries in random order: the even ones are keys of the table, the odd ones have another time
    q_rows = rng.permutation(N)
    q = h_chars.reshape(N, KEY_LEN)[q_rows].copy()
    q[1::2, KEY_LEN - 1] = ord("x")
    hq_chars = q.reshape(-1)
    q_chars = torch.from_numpy(hq_chars).to(dev)
    found = torch.empty(N, dtype=torch.int64, device=dev)
    h_found = np.empty(N, dtype=np.int64)
    do_search = lambda: check(lib.efl_strings_search(chars.data_ptr(), offsets.data_ptr(), t_order.data_ptr(), N,
                                                     q_chars.data_ptr(), offsets.data_ptr(), N, found.data_ptr(), sh))
    host_search = lambda: lib.efl_strings_search_host(h_chars.ctypes.data, h_offsets.ctypes.data, h_order.ctypes.data, N,
                                                      hq_chars.ctypes.data, h_offsets.ctypes.data, N, h_found.ctypes.data)
    t_host = host_timed(host_search)
    do_search()
    torch.cuda.synchronize()
    want = np.where(np.arange(N) % 2 == 0, q_rows, -1)
    assert np.array_equal(h_found, want) and np.array_equal(found.cpu().numpy(), want)
    t = timed(do_search)
    emit({"step": "search", "table_rows": N, "queries": N, "present": N // 2, "key_bytes": KEY_LEN, "launches": 1,
          "calls_timed": reps, "ms": round(t * 1e3, 4), "queries_per_s": round(N / t), "host_1_thread_ms": round(t_host * 1e3, 3),
          "over_host_1_thread": round(t_host / t, 2)})

    # what the reference's client runs: sorted() with a Python comparator, on a subset
    S = min(args.subset, N)
    t_python = host_timed(lambda: sorted(keys[:S], key=functools.cmp_to_key(record_cmp)))
    t_host = host_timed(lambda: host_sort(1, S, seg=False))
    want = sorted(range(S), key=lambda i: (keys[i][ID_LEN + 1:], keys[i][:ID_LEN], i))
    assert h_order[:S].tolist() == want
    t = timed(lambda: do_sort(1, S, seg=False))
    assert order[:S].tolist() == want
    emit({"step": "sort", "mode": "record", "rows": S, "key_bytes": KEY_LEN, "segments": 1, "calls_timed": reps,
          "ms": round(t * 1e3, 4), "rows_per_s": round(S / t), "host_1_thread_ms": round(t_host * 1e3, 3),
          "python_sorted_cmp_to_key_ms": round(t_python * 1e3, 1), "over_host_1_thread": round(t_host / t, 2),
          "over_python": round(t_python / t, 1)})

    if args.scaling:
        n = 2048
        while n <= N:
            for name, mode in MODES:
                t = timed(lambda: do_sort(mode, n))
                t_host = host_timed(lambda: host_sort(mode, n))
                emit({"step": "sort scaling", "mode": name, "rows": n, "launches": 2 + int(np.log2(n // 2048)),
                      "ms": round(t * 1e3, 4), "host_1_thread_ms": round(t_host * 1e3, 3)})
            n *= 2
    out.close()


if __name__ == "__main__":
    main()
