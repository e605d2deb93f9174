#!/usr/bin/env python3
"""The product step of a mode-C secret-sharing matmul (efl/privacy/secret_sharing.py _matmul) on
one MI355X, two ways over the same operands:

  library  five torch.matmul (hipBLASLt) and the additions around them, on slices and a transposed
           slice of the received tensor, exactly the lines of _matmul's "library" product;
  fused    one efl_ss_products launch of five terms over the same views (csrc/ssgemm.hip), through
           efl.secret_sharing.fused_products and as the bare C call at each workgroup tile.

Shapes: the examples' Dense step (256, 392) x (392, N) for N in 10, 64, 256, and (4096, 1024) x
(1024, 1024). Both results are first compared with float64 (the fused one against the derived bound
of tests/test_ss_products_gpu.py). Timing: HIP events on the launch stream around `--inner` calls,
`--rounds` interleaved rounds per path after a warm-up, the median round reported per call. One
JSON line per shape, also appended to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "elastic-federated-learning-solution_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import efl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--rounds", type=int, default=21)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = efl.lib.require_gpu()
lib, ss = efl.lib.raw(), efl.secret_sharing
stream = torch.cuda.current_stream()
SHAPES = [(256, 392, 10), (256, 392, 64), (256, 392, 256), (4096, 1024, 1024)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.inner):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3   # microseconds per call


for R, C, N in SHAPES:
    g = torch.Generator(device=dev).manual_seed(R + N)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    a, b = rnd(R, C), rnd(C, N)
    a_minus_e, eo_minus_ee = rnd(R, C), rnd(R, C // 2)
    half_plus_f, fo_plus_fe = rnd(C, N), rnd(C // 2, N)
    recv = rnd(R + N, C * 3 // 2)
    a1_e1, b1_f1 = recv[:R], recv[R:].t()
    ra1, re1 = a1_e1[:, :C], a1_e1[:, C:]
    rb1, rf1 = b1_f1[:C], b1_f1[C:]
    terms = [(a, b, 1), (a_minus_e, rb1, 1), (eo_minus_ee, rf1, 1), (ra1, half_plus_f, 1), (re1, fo_plus_fe, -1)]

    def library():
        z = a @ b
        z1 = a_minus_e @ rb1 + eo_minus_ee @ rf1
        z2 = ra1 @ half_plus_f - re1 @ fo_plus_fe
        return z + z1 + z2

    out = torch.empty(R, N, device=dev)
    arr = (efl.lib.SsTerm * efl.lib.SS_MAX_TERMS)()
    for rec, (A, B, s) in zip(arr, terms):
        rec.a, rec.a_rs, rec.a_cs, rec.b, rec.b_rs, rec.b_cs = (A.data_ptr(), A.stride(0), A.stride(1),
                                                               B.data_ptr(), B.stride(0), B.stride(1))
        rec.k, rec.sign = A.shape[1], s

    def bare(tile):
        return lambda: efl.lib.check(lib.efl_ss_products(arr, 5, out.data_ptr(), N, R, N, tile, stream.cuda_stream))

    paths = {"library": library, "fused": lambda: ss.fused_products(terms), "fused_bare": bare(0),
             "fused_bare_tile32": bare(32), "fused_bare_tile64": bare(64)}

    # outputs first: float64 reference and the derived bound
    ref = sum(s * (A.double() @ B.double()) for A, B, s in terms)
    mag = sum(A.double().abs() @ B.double().abs() for A, B, s in terms)
    nu = (sum(A.shape[1] for A, _, _ in terms) + 5) * 2.0 ** -24
    bound = 2 * nu / (1 - nu) * mag
    ratios = {}
    for name, fn in paths.items():
        got = fn()
        got = out if got is None else got
        ratios[name] = float(((got.double() - ref).abs() / bound).max())
    assert all(r <= 1.0 for k, r in ratios.items() if k != "library"), ratios

    for fn in paths.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(args.rounds):          # interleaved: drift hits every path alike
        for name, fn in paths.items():
            times[name].append(timed(fn))
    med = {name: float(np.median(t)) for name, t in times.items()}
    flops = 2.0 * R * N * sum(A.shape[1] for A, _, _ in terms)
    line = {"bench": "ss_products_mode_c", "shape": [R, C, N], "inner_k": [int(A.shape[1]) for A, _, _ in terms],
            "calls_per_round": args.inner, "rounds": args.rounds,
            "us_per_call": {k: round(v, 2) for k, v in med.items()},
            "us_min_max": {k: [round(min(t), 2), round(max(t), 2)] for k, t in times.items()},
            "library_over_fused": round(med["library"] / med["fused"], 3),
            "fused_tflops": round(flops / med["fused_bare"] / 1e6, 3),
            "max_err_over_bound": {k: round(v, 4) for k, v in ratios.items()},
            "library": efl.lib.version()}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
