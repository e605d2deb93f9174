#!/usr/bin/env python3
"""A DP-SGD step's microbatch gradients on one MI355X, two measurements:

  step     compute_gradients of the dp_mnist example's CNN (dp_cnn.py: conv 16@8 s2 same, pool, conv
           32@4 s2, pool, dense 32, dense 10; batch 256, 256 microbatches, l2_norm_clip 1.0, noise
           multiplier 1.0), microbatch_gradients="loop" against "batched" in the same process. The
           forward pass is outside the timed window (both paths share it); the window is a host clock
           around compute_gradients that ends in a device synchronise, `--rounds` interleaved rounds
           after a warm-up, the median reported. The two results are compared first.
           --model criteo_mlp (the criteo leader's dense stack, 181 -> 64 -> 16 -> 2) or wide_mlp
           (1024 -> 1024 -> 1024 -> 10) takes those instead. microbatch_gradients="factored" is timed
           beside the two (csrc/dpdense.hip for the Linear modules, csrc/dpconv.hip for dp_cnn's Conv2d
           modules), with each path's peak device memory over a step.
  kernels  efl_dp_clip_sum alone at [256, 1 Mi] float32 (clip mode 1: the norm pass reads the stack
           once, the sum pass once more; clip mode 0: one read), HIP events around `--inner` calls,
           as a fraction of the 8 TB/s HBM peak: algorithmic bytes (reads of the stack + one write of
           the output) over the time.

One JSON line per measurement, also appended to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "elastic-federated-learning-solution_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import efl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--model", choices=["dp_cnn", "criteo_mlp", "wide_mlp"], default="dp_cnn")
ap.add_argument("--paths", default="loop,batched,factored",
                help="the microbatch_gradients paths to time, the first the one the others are compared with")
ap.add_argument("--no-kernels", action="store_true", help="skip the efl_dp_clip_sum kernel measurement")
ap.add_argument("--kernel-shape", type=int, nargs=2, default=[256, 1 << 20])
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = efl.lib.require_gpu()
HBM_PEAK = 8.0e12


def emit(line):
    line["library"] = efl.lib.version()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


# ---- the whole step ----------------------------------------------------------------------------
torch.manual_seed(0)
nn = torch.nn
model = nn.Sequential(nn.Conv2d(1, 16, 8, stride=2, padding=3), nn.ReLU(), nn.MaxPool2d(2, 1),
                      nn.Conv2d(16, 32, 4, stride=2), nn.ReLU(), nn.MaxPool2d(2, 1), nn.Flatten(),
                      nn.Linear(512, 32), nn.ReLU(), nn.Linear(32, 10)).to(dev)
x = torch.randn(args.batch, 1, 28, 28, device=dev)
paths = tuple(args.paths.split(","))
if args.model != "dp_cnn":
    widths = (181, 64, 16, 2) if args.model == "criteo_mlp" else (1024, 1024, 1024, 10)
    model = nn.Sequential(*[m for i, o in zip(widths, widths[1:]) for m in (nn.Linear(i, o), nn.ReLU())][:-1]).to(dev)
    x = torch.randn(args.batch, widths[0], device=dev)
# "factored" counts the forward passes of its layers between steps: it gets a copy of the model
import copy  # noqa: E402
models = {p: copy.deepcopy(model) if p == "factored" else model for p in paths}
params = list(model.parameters())
y = torch.randint(0, model[-1].out_features, (args.batch,), device=dev)
opts = {p: efl.privacy.DPGradientDescentGaussianOptimizer(list(models[p].parameters()), noise_multiplier=1.0,
                                                          l2_norm_clip=1.0, learning_rate=0.25, microbatch_gradients=p,
                                                          dense_layers=[m for m in models[p] if isinstance(m, nn.Linear)]
                                                          if p == "factored" else None,
                                                          conv_layers=[m for m in models[p] if isinstance(m, nn.Conv2d)]
                                                          if p == "factored" else None)
        for p in paths}


def step(path):
    loss = nn.functional.cross_entropy(models[path](x), y, reduction="none")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gv = opts[path].compute_gradients(loss, list(models[path].parameters()))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, [g for g, _ in gv]


grads = {}
for p in opts:
    efl.privacy.set_noise_seed(5, 0)
    grads[p] = step(p)[1]
# same noise positions; the sums differ by the scales' rounding (fp32 reductions against double)
diff = max([float((a - b).abs().max() / (b.abs().max() + 1e-30)) for p in paths[1:]
            for a, b in zip(grads[p], grads[paths[0]])], default=0.0)
assert diff < 1e-4, diff
del grads
peak = {}
for p in opts:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step(p)
    peak[p] = torch.cuda.max_memory_allocated()
times = {p: [] for p in opts}
for _ in range(args.rounds):
    for p in opts:
        times[p].append(step(p)[0])
med = {p: float(np.median(t)) for p, t in times.items()}
emit({"bench": "dp_step_compute_gradients", "model": args.model, "batch": args.batch, "microbatches": args.batch,
      "variables": len(params), "floats": sum(p.numel() for p in params), "rounds": args.rounds,
      "ms_per_step": {p: round(v, 3) for p, v in med.items()},
      "ms_min_max": {p: [round(min(t), 3), round(max(t), 3)] for p, t in times.items()},
      "peak_bytes": peak,
      **({"loop_over_batched": round(med["loop"] / med["batched"], 2)} if "loop" in med and "batched" in med else {}),
      **({"batched_over_factored": round(med["batched"] / med["factored"], 2)} if "batched" in med and "factored" in med else {}),
      "max_rel_diff": diff})
if args.no_kernels:
    sys.exit(0)

# ---- the kernels alone -------------------------------------------------------------------------
R, N = args.kernel_shape
lib = efl.lib.raw()
g = torch.randn(R, N, device=dev)
out = torch.empty(N, device=dev)
scales = torch.empty(R, device=dev)
numels = (ctypes.c_int64 * 1)(N)
we = lib.efl_dp_clip_work_elems(numels, 1, R)
work = torch.empty(we, dtype=torch.float64, device=dev)
arr = (efl.lib.DpVar * 1)()
arr[0].grads, arr[0].out, arr[0].numel, arr[0].row_stride, arr[0].ctr0 = g.data_ptr(), out.data_ptr(), N, N, 0
stream = torch.cuda.current_stream()


def call(clip_mode):
    efl.lib.check(lib.efl_dp_clip_sum(arr, 1, R, clip_mode, 1.0, 1, 1.0, float(R), 7, scales.data_ptr(),
                                      work.data_ptr(), we, stream.cuda_stream))


def timed(clip_mode):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.inner):
        call(clip_mode)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e-3


for m in (1, 0):
    call(m)
torch.cuda.synchronize()
ref = (g.double() * scales.double()[:, None]).sum(0)          # after the clip_mode 1 warm-up: its scales
kt = {m: [] for m in (1, 0)}
for _ in range(args.rounds):
    for m in kt:
        kt[m].append(timed(m))
for m, name in ((1, "clip_sum_noise"), (0, "sum_noise")):
    t = float(np.median(kt[m]))
    nbytes = 4 * (R * N * (2 if m == 1 else 1) + N)
    emit({"bench": "dp_clip_sum_kernels", "kind": name, "clip_mode": m, "shape": [R, N], "calls_per_round": args.inner,
          "rounds": args.rounds, "ms_per_call": round(t * 1e3, 4),
          "ms_min_max": [round(min(kt[m]) * 1e3, 4), round(max(kt[m]) * 1e3, 4)],
          "algorithmic_bytes": nbytes, "hbm_frac": round(nbytes / t / HBM_PEAK, 4)})
call(1)
noise_free = out.double() * R - ref                             # = z sigma: bounded, not a blow-up
assert float(noise_free.abs().max()) < 8.0, float(noise_free.abs().max())
