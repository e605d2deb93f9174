#!/usr/bin/env python3
"""efl.metrics on the MI355X: one JSON line appended to profiles/metrics/bench_metrics.jsonl.

Three measurements, each beside two comparisons taken in the same process:
  auc           efl.metrics.Auc.update without weights, n = 2^24, T = 200, uint8 labels
  auc_weighted  the same shape with float32 weights
  gauc          efl.metrics.Gauc.update, n = 2^20, about 2^14 groups
  read          a compute-free read of the same bytes (torch.sum over each input, one launch per input)
  torch         the reference's formulation in plain torch: tf.metrics.auc's [T, n] compare-and-sum (in
                slices of --torch-chunk elements: the whole [200, 2^24] boolean tensor is 3.4 GB, four
                times over), and for gauc torch.sort by (indicator, prediction) plus a host loop over the
                groups, on --torch-groups groups and scaled to all of them
Timing: device events around --inner calls, --rounds interleaved rounds after a warm-up round, the median
reported. The unweighted update is reported as a fraction of the read, the other two as multiples of torch.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "elastic-federated-learning-solution_amd"))
import efl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 24)
ap.add_argument("--thresholds", type=int, default=200)
ap.add_argument("--gauc-n", type=int, default=1 << 20)
ap.add_argument("--groups", type=int, default=1 << 14)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--torch-chunk", type=int, default=1 << 20)
ap.add_argument("--torch-groups", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics", "bench_metrics.jsonl"))
args = ap.parse_args()

dev = efl.lib.require_gpu()
g = torch.Generator(device=dev).manual_seed(0)
T = args.thresholds
pred = torch.rand(args.n, generator=g, device=dev)
lab = (torch.rand(args.n, generator=g, device=dev) < 0.25).to(torch.uint8)
w = torch.rand(args.n, generator=g, device=dev) + 0.5
gp = torch.rand(args.gauc_n, generator=g, device=dev)
gl = (torch.rand(args.gauc_n, generator=g, device=dev) < 0.25).to(torch.uint8)
gi = torch.randint(0, args.groups, (args.gauc_n,), generator=g, device=dev)
thr = torch.tensor([-1e-7] + [i / (T - 1) for i in range(1, T - 1)] + [1 + 1e-7], dtype=torch.float32, device=dev)
m_auc, m_w, m_gauc = efl.metrics.Auc(T), efl.metrics.Auc(T), efl.metrics.Gauc()


def torch_auc(weights):
    """tf.metrics.auc's update: tile the predictions against the thresholds, and-and-sum the four ways."""
    out = torch.zeros(4, T, dtype=torch.float64, device=dev)
    for s in range(0, args.n, args.torch_chunk):
        p, pos = pred[s:s + args.torch_chunk], lab[s:s + args.torch_chunk] != 0
        ww = torch.ones_like(p) if weights is None else weights[s:s + args.torch_chunk]
        gt = p[None, :] > thr[:, None]
        for r, mask in enumerate((gt & pos, gt & ~pos, ~gt & ~pos, ~gt & pos)):
            out[r] += (mask * ww).sum(1, dtype=torch.float64)
    return out


def torch_gauc():
    """sort by (indicator, prediction), then a host loop over the first --torch-groups groups."""
    o = torch.argsort(gp, stable=True)
    o = o[torch.argsort(gi[o], stable=True)]
    si, sp, sl = gi[o], gp[o], gl[o]
    ids, counts = torch.unique_consecutive(si, return_counts=True)
    ends = counts.cumsum(0).tolist()
    total = 0.0
    for k in range(min(args.torch_groups, len(ends))):
        a, b = (ends[k - 1] if k else 0), ends[k]
        p, l = sp[a:b], sl[a:b] != 0
        pn = int(l.sum()) * int((~l).sum())
        if pn:
            u = (p[l][:, None] > p[~l][None, :]).sum() + 0.5 * (p[l][:, None] == p[~l][None, :]).sum()
            total += (b - a) * float(u) / pn
    return total, len(ends)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


groups_seen = torch_gauc()[1]
paths = {
    "auc": (lambda: m_auc.update(lab, pred), args.inner),
    "auc_read": (lambda: (pred.sum(), lab.sum()), args.inner),
    "auc_torch": (lambda: torch_auc(None), 1),
    "auc_weighted": (lambda: m_w.update(lab, pred, w), args.inner),
    "auc_weighted_read": (lambda: (pred.sum(), lab.sum(), w.sum()), args.inner),
    "auc_weighted_torch": (lambda: torch_auc(w), 1),
    "gauc": (lambda: m_gauc.update(gl, gp, gi), args.inner),
    "gauc_read": (lambda: (gp.sum(), gl.sum(), gi.sum()), args.inner),
    "gauc_torch": (torch_gauc, 1),
}
# the two formulations agree before anything is timed
m_auc.update(lab, pred)
assert torch.equal(torch.stack(m_auc.confusion()), torch_auc(None)), "confusion counts differ from the torch formulation"
times = {k: [] for k in paths}
for r in range(args.rounds + 1):                      # the first round warms up
    for k, (fn, inner) in paths.items():
        t = timed(fn, inner)
        if r:
            times[k].append(t)
med = {k: float(np.median(v)) for k, v in times.items()}
med["gauc_torch"] *= groups_seen / min(args.torch_groups, groups_seen)      # the host loop, scaled to every group
line = {"tool": "bench_metrics", "library": efl.lib.version(), "device": torch.cuda.get_device_name(0),
        "n": args.n, "num_thresholds": T, "gauc_n": args.gauc_n, "gauc_groups": groups_seen,
        "rounds": args.rounds, "inner": args.inner, "torch_chunk": args.torch_chunk,
        "torch_groups_timed": min(args.torch_groups, groups_seen),
        "ms": {k: round(v, 4) for k, v in med.items()},
        "auc_bytes_per_element": 5, "auc_GBps": round(5 * args.n / med["auc"] / 1e6, 1),
        "auc_fraction_of_read": round(med["auc_read"] / med["auc"], 4),
        "auc_weighted_times_read": round(med["auc_weighted"] / med["auc_weighted_read"], 2),
        "auc_times_faster_than_torch": round(med["auc_torch"] / med["auc"], 1),
        "auc_weighted_times_faster_than_torch": round(med["auc_weighted_torch"] / med["auc_weighted"], 1),
        "gauc_times_faster_than_torch": round(med["gauc_torch"] / med["gauc"], 1),
        "gauc_times_read": round(med["gauc"] / med["gauc_read"], 1)}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    f.write(json.dumps(line) + "\n")
print(json.dumps(line))
