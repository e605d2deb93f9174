#!/usr/bin/env python3
"""Signed-ID store throughput on one MI355X (efl.psi.IdStore): rows per second of
efl_idset_insert and efl_idset_find for 32-byte rows, at batches of 2,048 (the reference's join
batch), 65,536 and 2^20, into stores that hold 2^20 and 2^24 keys in 4x as many slots (a load factor
of 1/4 before the batch, at most 1/2 after it: the range a doubling table lives in). Kernel time
between HIP events on the launch stream after a warm-up call, through the C ABI on caller-owned
buffers; every timed call gets rows of its own (calls_timed sets per figure), so no call probes the
cache lines the call before it touched. One JSON line per (store, batch) into profiles/psi/bench_idset.jsonl (--out), each with

  * insert_new: every row of the batch is a new key (all five launches do their most);
    insert_present: every row is a key already; find_hit / find_miss: every row present / absent.
    Before each timed insert the store is put back to its size (size counter reset, slots rehashed),
    outside the timed interval.
  * the Python-dict baseline of the same run, the reference's DictSampleKvStore
    (efls-data/xfl/data/store/sample_kv_store.py) on one core: `d[k] = v` per row and `k in d` per
    row over `bytes` keys in a dict of the same size, and dict_slice_ms, the cost of cutting a host
    copy of the batch into `bytes` objects, which a caller holding a tensor pays first.
  * on the lines of the 2^20-key store and the 2^20-row batch: x25519_ms, efl_x25519 of the same 2^20
    rows timed in the same process, and the two conditions find_below_x25519 / insert_below_x25519:
    the store must not be the slowest step of an ECDH join.

    python tools/bench_idset.py [--out PATH] [--stores 1048576,16777216] [--batches 2048,65536,1048576]
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "elastic-federated-learning-solution_amd")
sys.path.insert(0, PKG)

SECRET = hashlib.sha256(b"bench_idset secret").digest()
WIDTH = 32
SEED = 0x1D5E7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi", "bench_idset.jsonl"))
    ap.add_argument("--stores", default="1048576,16777216")
    ap.add_argument("--batches", default="2048,65536,1048576")
    ap.add_argument("--no-dict", action="store_true", help="skip the Python-dict baseline")
    args = ap.parse_args()
    stores = [int(s) for s in args.stores.split(",")]
    batches = [int(s) for s in args.batches.split(",")]

    import torch
    import efl
    dev = efl.lib.require_gpu()
    lib = efl.lib.raw()
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    check = efl.lib.check

    def timed(fn, reps, before=None):
        """Mean seconds of fn(rep) between events, rep = 1 .. reps after the warm-up fn(0). With
        `before` (run ahead of each call, outside the interval) every call has an interval of its own;
        without it all calls share one."""
        fn(0)
        if before is None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for rep in range(1, reps + 1):
                fn(rep)
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / 1e3 / reps
        total = 0.0
        for rep in range(1, reps + 1):
            before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn(rep)
            b.record(stream)
            b.synchronize()
            total += a.elapsed_time(b) / 1e3
        return total / reps

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    for S in stores:
        cap = 4 * S
        g = torch.Generator(device=dev).manual_seed(S)
        present = torch.randint(0, 256, (S, WIDTH), dtype=torch.uint8, device=dev, generator=g)
        keys = torch.empty((cap // 2, WIDTH), dtype=torch.uint8, device=dev)
        slots = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        size = torch.zeros(1, dtype=torch.int64, device=dev)
        nmax = max(max(batches), S)
        pos = torch.empty(nmax, dtype=torch.int64, device=dev)
        nbytes = int(lib.efl_idset_scratch_bytes(nmax))
        scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)

        def insert(rows, n, bound):
            check(lib.efl_idset_insert(rows.data_ptr(), n, WIDTH, keys.data_ptr(), cap // 2, size.data_ptr(), bound,
                                       slots.data_ptr(), cap, SEED, pos.data_ptr(), scratch.data_ptr(), nbytes, sh))

        def find(rows, n):
            check(lib.efl_idset_find(rows.data_ptr(), n, WIDTH, keys.data_ptr(), slots.data_ptr(), cap, SEED,
                                     pos.data_ptr(), sh))

        def restore():
            size.fill_(S)
            check(lib.efl_idset_rehash(keys.data_ptr(), WIDTH, size.data_ptr(), S, slots.data_ptr(), cap, SEED, sh))

        # build the store in one batch and check it
        t0 = time.perf_counter()
        insert(present, S, 0)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        assert int(size) == S and torch.equal(pos[:S], torch.arange(S, device=dev)), "random rows collided"
        t_rehash = timed(lambda rep: restore(), 3)

        d = None
        if not args.no_dict:
            raw = present.cpu().numpy().tobytes()
            d = dict.fromkeys((raw[i:i + WIDTH] for i in range(0, len(raw), WIDTH)), 0)
            del raw
            assert len(d) == S

        for B in batches:
            # other rows in every call, so that no call probes lines the call before it left in a cache
            reps = 50 if B <= 65536 else 10
            fresh_sets = [torch.randint(0, 256, (B, WIDTH), dtype=torch.uint8, device=dev, generator=g)
                          for _ in range(reps + 1)]
            known_sets = [present[torch.randperm(S, device=dev, generator=g)[:B]].contiguous() for _ in range(reps + 1)]
            fresh, known = fresh_sets[-1], known_sets[-1]
            t_new = timed(lambda rep: insert(fresh_sets[rep], B, S), reps, before=restore)
            assert int(size) == S + B and int(pos[:B].min()) == S and int(pos[:B].max()) == S + B - 1
            t_old = timed(lambda rep: insert(known_sets[rep], B, S), reps, before=restore)
            assert int(size) == S
            restore()
            t_hit = timed(lambda rep: find(known_sets[rep], B), reps)
            assert int(pos[:B].min()) >= 0
            t_miss = timed(lambda rep: find(fresh_sets[rep], B), reps)
            assert int(pos[:B].max()) == -1
            rec = {"store_keys": S, "slots": cap, "batch": B, "width": WIDTH, "calls_timed": reps,
                   "insert_new_ms": round(t_new * 1e3, 4), "insert_new_per_s": round(B / t_new),
                   "insert_present_ms": round(t_old * 1e3, 4), "insert_present_per_s": round(B / t_old),
                   "find_hit_ms": round(t_hit * 1e3, 4), "find_hit_per_s": round(B / t_hit),
                   "find_miss_ms": round(t_miss * 1e3, 4), "find_miss_per_s": round(B / t_miss),
                   "rehash_ms": round(t_rehash * 1e3, 4), "build_one_batch_s": round(build_s, 4)}
            if d is not None:
                raw = fresh.cpu().numpy().tobytes()
                t0 = time.perf_counter()
                ks = [raw[i:i + WIDTH] for i in range(0, len(raw), WIDTH)]
                t_slice = time.perf_counter() - t0
                t0 = time.perf_counter()
                miss = [k in d for k in ks]                       # DictSampleKvStore.exists
                t_dmiss = time.perf_counter() - t0
                t0 = time.perf_counter()
                for i, k in enumerate(ks):                        # DictSampleKvStore.put, one call per row
                    d[k] = i
                t_dput = time.perf_counter() - t0
                t0 = time.perf_counter()
                hit = [k in d for k in ks]
                t_dhit = time.perf_counter() - t0
                assert not any(miss) and all(hit)
                for k in ks:
                    del d[k]
                rec.update({"dict_put_ms": round(t_dput * 1e3, 3), "dict_put_per_s": round(B / t_dput),
                            "dict_exists_hit_ms": round(t_dhit * 1e3, 3), "dict_exists_miss_ms": round(t_dmiss * 1e3, 3),
                            "dict_exists_per_s": round(B / t_dhit), "dict_slice_ms": round(t_slice * 1e3, 3),
                            "insert_over_dict": round(t_dput / t_new, 1), "find_over_dict": round(t_dhit / t_hit, 1)})
            if S == 1 << 20 and B == 1 << 20:
                r = torch.empty_like(fresh)
                t_x = timed(lambda rep: check(lib.efl_x25519(SECRET, fresh.data_ptr(), r.data_ptr(), B, sh)), 3)
                rec.update({"x25519_ms": round(t_x * 1e3, 4), "find_below_x25519": bool(max(t_hit, t_miss) < t_x),
                            "insert_below_x25519": bool(max(t_new, t_old) < t_x)})
                del r
            rec["library"] = efl.lib.version()
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            del fresh, known, fresh_sets, known_sets
        del present, keys, slots, pos, scratch, d
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
