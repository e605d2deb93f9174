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
           --model criteo_embed is the criteo example's shape with its embedding tables in: 21
           EmbeddingBag(V_i, 8, mode="mean") tables of one hashed id each (V_i spread geometrically from 3 to
           the example's largest, 2,000,000 rows), then 168 -> 64 -> 16 -> 2. Run it with --paths loop,factored:
           "batched" cannot allocate its [256, V, 8] stacks (16 GB for the largest table alone). --loop-rounds
           gives the slow path fewer rounds. The table sizes are this tool's own, not the example's list of
           hash-bucket sizes. After the step it times efl_dp_embed_clip_sum with clip mode 0 on the largest
           table, the WHOLE call: the 256 ids' sort (one launch) and the noise of 16,000,000 floats (one
           launch), against efl_dp_noise over as many floats, HIP events around `--inner` calls, in alternating
           rounds. The C ABI has no entry for the noise launch alone; a kernel trace splits the call.
           --model seq_mlp is a behaviour-sequence tower: a [256, 64, 128] input, Linear 128 -> 128 twice at
           every position, the mean over the 64 positions, Linear 128 -> 2. Under "factored" the two position-wise
           layers take csrc/dpseq.hip (P = 64 rows per microbatch), the head csrc/dpdense.hip, one shared norm.
           --model norm_cnn is dp_cnn with a GroupNorm after each convolution (4 groups of 16, 8 of 32), and
           --model seq_ln is seq_mlp with a LayerNorm(128) after each Linear over the positions: the scale and bias
           of the norm layers take csrc/dpnorm.hip under the same shared norm.
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
ap.add_argument("--model", choices=["dp_cnn", "criteo_mlp", "wide_mlp", "criteo_embed", "seq_mlp", "norm_cnn", "seq_ln"],
                default="dp_cnn")
ap.add_argument("--loop-rounds", type=int, default=None, help='rounds of the "loop" path (default: --rounds)')
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

TABLES = [round(3 * (2.0e6 / 3) ** (i / 20)) for i in range(21)]


class CriteoEmbed(nn.Module):
    def __init__(self):
        super().__init__()
        self.tables = nn.ModuleList(nn.EmbeddingBag(v, 8, mode="mean") for v in TABLES)
        self.mlp = nn.Sequential(nn.Linear(8 * len(TABLES), 64), nn.ReLU(), nn.Linear(64, 16), nn.ReLU(), nn.Linear(16, 2))

    def forward(self, ids):
        return self.mlp(torch.cat([t(ids[:, i:i + 1]) for i, t in enumerate(self.tables)], 1))


class SeqMlp(nn.Module):
    def __init__(self, ln=False):
        super().__init__()
        self.tower = nn.Sequential(*[m for _ in range(2)
                                     for m in (nn.Linear(128, 128), *([nn.LayerNorm(128)] if ln else []), nn.ReLU())])
        self.head = nn.Linear(128, 2)

    def forward(self, seq):
        return self.head(self.tower(seq).mean(1))


if args.model == "criteo_embed":
    model = CriteoEmbed().to(dev)
    x = torch.stack([torch.randint(0, v, (args.batch,), device=dev) for v in TABLES], 1)
elif args.model in ("seq_mlp", "seq_ln"):
    model = SeqMlp(ln=args.model == "seq_ln").to(dev)
    x = torch.randn(args.batch, 64, 128, device=dev)
elif args.model == "norm_cnn":
    model = nn.Sequential(nn.Conv2d(1, 16, 8, stride=2, padding=3), nn.GroupNorm(4, 16), nn.ReLU(), nn.MaxPool2d(2, 1),
                          nn.Conv2d(16, 32, 4, stride=2), nn.GroupNorm(8, 32), nn.ReLU(), nn.MaxPool2d(2, 1), nn.Flatten(),
                          nn.Linear(512, 32), nn.ReLU(), nn.Linear(32, 10)).to(dev)
elif args.model != "dp_cnn":
    widths = (181, 64, 16, 2) if args.model == "criteo_mlp" else (1024, 1024, 1024, 10)
    model = nn.Sequential(*[m for i, o in zip(widths, widths[1:]) for m in (nn.Linear(i, o), nn.ReLU())][:-1]).to(dev)
    x = torch.randn(args.batch, widths[0], device=dev)
# "factored" counts the forward passes of its layers between steps: it gets a copy of the model
import copy  # noqa: E402
models = {p: copy.deepcopy(model) if p == "factored" else model for p in paths}
params = list(model.parameters())
y = torch.randint(0, [m for m in model.modules() if isinstance(m, nn.Linear)][-1].out_features, (args.batch,), device=dev)


def of_kind(path, *kinds):
    return [m for m in models[path].modules() if isinstance(m, kinds)] if path == "factored" else None


opts = {p: efl.privacy.DPGradientDescentGaussianOptimizer(list(models[p].parameters()), noise_multiplier=1.0,
                                                          l2_norm_clip=1.0, learning_rate=0.25, microbatch_gradients=p,
                                                          dense_layers=of_kind(p, nn.Linear), conv_layers=of_kind(p, nn.Conv2d),
                                                          embedding_layers=of_kind(p, nn.EmbeddingBag),
                                                          norm_layers=of_kind(p, nn.LayerNorm, nn.GroupNorm))
        for p in paths}


def step(path, n=None):
    loss = nn.functional.cross_entropy(models[path](x[:n]), y[:n], reduction="none")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gv = opts[path].compute_gradients(loss, list(models[path].parameters()))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, [g for g, _ in gv]


# torch's GroupNorm backward on ROCm gave wrong weight and bias gradients at 256 examples (right at 64 and on the
# CPU), which "loop" and "batched" inherit: norm_cnn's paths are compared on the first 64 examples
compare_n = min(args.batch, 64) if args.model == "norm_cnn" else None
grads = {}
for p in opts:
    efl.privacy.set_noise_seed(5, 0)
    grads[p] = step(p, compare_n)[1]
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
for k in range(args.rounds):
    for p in opts:
        if p != "loop" or args.loop_rounds is None or k < args.loop_rounds:
            times[p].append(step(p)[0])
med = {p: float(np.median(t)) for p, t in times.items()}
emit({"bench": "dp_step_compute_gradients", "model": args.model, "batch": args.batch, "microbatches": args.batch,
      "variables": len(params), "floats": sum(p.numel() for p in params), "rounds": args.rounds, **({"loop_rounds": len(times["loop"])} if args.loop_rounds and "loop" in times else {}),
      "ms_per_step": {p: round(v, 3) for p, v in med.items()},
      "ms_min_max": {p: [round(min(t), 3), round(max(t), 3)] for p, t in times.items()},
      "peak_bytes": peak,
      **({"loop_over_batched": round(med["loop"] / med["batched"], 2)} if "loop" in med and "batched" in med else {}),
      **({"batched_over_factored": round(med["batched"] / med["factored"], 2)} if "batched" in med and "factored" in med else {}),
      "max_rel_diff": diff, **({"max_rel_diff_examples": compare_n} if compare_n else {})})
if args.model == "criteo_embed":
    # ---- the dense pass over the largest table against efl_dp_noise over as many floats ---------
    lib, V, dim, B = efl.lib.raw(), max(TABLES), 8, args.batch
    stream = torch.cuda.current_stream()
    ids, d = torch.randint(0, V, (B, 1), device=dev), torch.randn(B, dim, device=dev)
    out, zeros = torch.empty(V, dim, device=dev), torch.zeros(V * dim, device=dev)
    arr = (efl.lib.DpEmbed * 1)()
    L = arr[0]
    L.ids, L.d, L.out, L.V, L.dim, L.L, L.w, L.d_row_stride, L.d_l_stride = ids.data_ptr(), d.data_ptr(), out.data_ptr(), V, dim, 1, 1.0, dim, 0
    nbytes = lib.efl_dp_embed_scratch_bytes(arr, 1, B)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    calls = {"embed_clip_sum": lambda: efl.lib.check(lib.efl_dp_embed_clip_sum(
                 arr, 1, B, B, 0, 0.0, 1, 1.0, float(B), 7, None, None, 0, scratch.data_ptr(), nbytes, stream.cuda_stream)),
             "dp_noise": lambda: efl.lib.check(lib.efl_dp_noise(zeros.data_ptr(), zeros.data_ptr(), V * dim, 1, 0.0, 1.0, 7, 0,
                                                                stream.cuda_stream))}
    kt = {k: [] for k in calls}
    for k in range(args.rounds + 1):                # the first round warms up
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.inner):
                fn()
            e1.record(stream)
            e1.synchronize()
            if k:
                kt[name].append(e0.elapsed_time(e1) / args.inner)
    med = {k: float(np.median(t)) for k, t in kt.items()}
    emit({"bench": "dp_embed_clip_sum_call", "measures": "efl_dp_embed_clip_sum, clip mode 0: the group launch and the noise "
          "launch together (the noise launch alone is not timed here); hbm_frac: bytes written by the call / its time",
          "table": [V, dim], "entries": B, "calls_per_round": args.inner, "rounds": args.rounds,
          "ms_per_call": {k: round(v, 4) for k, v in med.items()},
          "ms_min_max": {k: [round(min(t), 4), round(max(t), 4)] for k, t in kt.items()},
          "hbm_frac": {"embed_clip_sum": round(4 * V * dim / (med["embed_clip_sum"] * 1e-3) / HBM_PEAK, 4),
                       "dp_noise": round(8 * V * dim / (med["dp_noise"] * 1e-3) / HBM_PEAK, 4)},
          "embed_median_no_slower_than_dp_noise_slowest": med["embed_clip_sum"] <= max(kt["dp_noise"])})
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
