#!/usr/bin/env python3
"""The tail of an RSA PSI signature on one MI355X (efl.psi): efl_rsa_decimal (the
decimal text of every signature) and efl_rsa_oneway (the 64-bit SHA-256 one-way hash over it), kernel
time between HIP events on the launch stream after a warm-up launch, at 262,144 rows of 64 words (the
2048-bit key of tests/golden/rsa_kat.json) and 65,536 rows of 128 words (the 4096-bit key). The rows
are signatures the same process made, and each line carries two comparisons from the same run:

  * efl_rsa_sign of the same rows: oneway_over_sign = one-way time / sign time. The signer is meant to
    stay the step that sets the protocol's rate.
  * the host tail this replaces, ServerRsaSigner.sign_func's last step as it was: the signatures copied
    to the host, ints_from_rows, then oneway_hash_list with oneway_hash=oneway_sha256 (str(int) and
    hashlib per ID) on one core: host_over_oneway = host time / one-way time.

The one-way rows of the timed launch are checked against the host tail's strings, all of them.
One JSON line per key into profiles/psi/bench_oneway.jsonl (--out).

    python tools/bench_oneway.py [--out PATH] [--keys 2048,4096] [--n 262144]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "elastic-federated-learning-solution_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi", "bench_oneway.jsonl"))
    ap.add_argument("--keys", default="2048,4096")
    ap.add_argument("--n", type=int, default=1 << 18, help="rows at 2048 bits (a quarter at 4096)")
    args = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "rsa_kat.json")) as f:
        kat = {k["name"]: k for k in json.load(f)["keys"]}

    import torch
    import efl
    rc = efl.psi.rsa_cipher
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

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    for bits in (int(b) for b in args.keys.split(",")):
        k = kat[f"openssl-{bits}"]
        v = {f: int(k[f], 16) for f in "nedpq"}
        N = args.n if bits <= 2048 else max(1, args.n // 4)
        key = efl.psi.RsaKey.private(v["n"], v["e"], v["d"], v["p"], v["q"])
        W = key.words
        g = torch.Generator(device=dev).manual_seed(bits)
        x = torch.randint(-2 ** 31, 2 ** 31, (N, W), dtype=torch.int32, device=dev, generator=g)
        s = torch.empty_like(x)
        D = lib.efl_rsa_decimal_digits(W)
        text = torch.empty((N, D), dtype=torch.uint8, device=dev)
        ln = torch.empty(N, dtype=torch.int32, device=dev)
        rows8 = torch.empty((N, 8), dtype=torch.uint8, device=dev)
        t_sign = timed(lambda: efl.lib.check(lib.efl_rsa_sign(key._h, x.data_ptr(), s.data_ptr(), N, sh)), 2)
        t_dec = timed(lambda: efl.lib.check(lib.efl_rsa_decimal(s.data_ptr(), W, N, text.data_ptr(), D, ln.data_ptr(),
                                                                sh)), 5)
        t_one = timed(lambda: efl.lib.check(lib.efl_rsa_oneway(s.data_ptr(), W, N, 1, rows8.data_ptr(), sh)), 5)
        # the host tail as it was, on the same signatures, one core
        signer = efl.psi.RsaSigner(oneway_hash=rc.oneway_sha256)
        t0 = time.perf_counter()
        host = signer.oneway_hash_list(rc.ints_from_rows(s))
        t_host = time.perf_counter() - t0
        ok = rc.oneway_texts(rows8) == host
        sample = rc.ints_from_rows(s[:64])
        raw, lens = text[:64].cpu().numpy().tobytes(), ln[:64].tolist()
        ok_text = all(raw[(i + 1) * D - lens[i]:(i + 1) * D] == str(sv).encode() for i, sv in enumerate(sample))
        rec = {"key_bits": bits, "rows": N, "words": W, "digits_max": D,
               "sign_ms": round(t_sign * 1e3, 3), "decimal_ms": round(t_dec * 1e3, 3),
               "oneway_ms": round(t_one * 1e3, 3), "host_tail_ms": round(t_host * 1e3, 1),
               "sign_per_s": round(N / t_sign), "decimal_per_s": round(N / t_dec), "oneway_per_s": round(N / t_one),
               "host_tail_per_s": round(N / t_host),
               "oneway_over_sign": round(t_one / t_sign, 4), "decimal_over_sign": round(t_dec / t_sign, 4),
               "host_over_oneway": round(t_host / t_one, 1),
               "text_bytes_written": N * D, "text_gb_per_s": round(N * D / t_dec / 1e9, 1),
               "host_tail": "ints_from_rows + oneway_hash_list(oneway_hash=oneway_sha256), one core, D2H included",
               "oneway_rows_equal_host_tail": bool(ok), "text_sample_equals_str": bool(ok_text),
               "library": efl.lib.version()}
        assert ok and ok_text, rec
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        del x, s, text, ln, rows8, key
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
