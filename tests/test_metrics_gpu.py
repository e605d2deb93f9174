"""GPU: efl.metrics (csrc/auc.hip) against plain float64 numpy written from the definitions in
include/efl_hip.h: the [T, n] comparison on float32 arrays for the confusion sums, the curve's terms
from the device's own sums for the value, and every (positive, negative) pair of a group for gauc."""
import functools

import numpy as np
import pytest
import torch

import efl

pytestmark = pytest.mark.gpu
TILE = efl.lib.AUC_TILE
DTYPES = [torch.uint8, torch.bool, torch.int32, torch.int64, torch.float32]
TS = [2, 3, 200, 201, 4096]
CURVES = [(c, m) for c in ("ROC", "PR") for m in ("trapezoidal", "careful_interpolation", "minoring", "majoring")]


def sizes(T):
    """1, a wave +- 1, a tile +- 1, and three workgroups + 1 or (if more) every threshold's three values."""
    return [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, max(3 * TILE + 1, 3 * T + 9)]


def thresholds(T):
    thr = (np.arange(T) / (T - 1)).astype(np.float32)
    thr[0], thr[-1] = np.float32(-1e-7), np.float32(1 + 1e-7)
    return thr


@functools.lru_cache(maxsize=None)
def case(T, n):
    """(predictions, labels with non-zero values other than 1, weights 2^-20 .. 2^20 with zeros, and the
    reference's unweighted and weighted (tp, fp, tn, fn) [4, T]); every threshold, its two neighbours
    and the special values come first in a seeded shuffle when n has room for them."""
    rng = np.random.default_rng(1000 * T + n)
    thr = thresholds(T)
    special = np.concatenate([thr, np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf)),
                              np.array([-0.0, 0.0, 1.0, -1e-6, -3.0, 1.000001, 7.0, np.nan, np.inf], np.float32)])
    pred = np.concatenate([rng.permutation(special), rng.random(n, dtype=np.float32)])[:n]
    pred = rng.permutation(pred).astype(np.float32)
    lab = rng.choice(np.array([0, 0, 1, 2, 255]), n)
    w = np.ldexp(1 + rng.random(n), rng.integers(-20, 20, n)).astype(np.float32) * (rng.random(n) > 0.1)
    gt, pos = pred[None, :] > thr[:, None], lab != 0
    refs = [np.array([[x[m].sum() for m in mask] for mask in (gt & pos, gt & ~pos, ~gt & ~pos, ~gt & pos)])
            for x in (np.ones(n), w.astype(np.float64))]
    return pred, lab, w, refs[0], refs[1]


def confusion(T, pred, lab, w=None, dtype=torch.uint8, splits=()):
    m = efl.metrics.Auc(num_thresholds=T)
    for part in np.split(np.arange(len(pred)), list(splits)):
        args = [torch.tensor(a[part]).cuda() for a in ((lab, pred) if w is None else (lab, pred, w))]
        m.update(args[0].to(dtype), *args[1:])
    return m, torch.stack(m.confusion()).cpu().numpy()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ni", range(8))
def test_confusion_counts_are_exact(T, ni):
    n = sizes(T)[ni]
    pred, lab, _, ref, _ = case(T, n)
    m, got = confusion(T, pred, lab, dtype=DTYPES[(ni + T) % 5])
    assert np.array_equal(got, ref)
    _, twice = confusion(T, pred, lab, dtype=DTYPES[(ni + T + 1) % 5], splits=(n // 3,))
    assert np.array_equal(twice, ref)                      # two updates: the concatenation's counts
    m.reset()
    assert not torch.stack(m.confusion()).any()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("ni", range(8))
def test_confusion_sums_with_weights(T, ni):
    n = sizes(T)[ni]
    pred, lab, w, _, ref = case(T, n)
    _, got = confusion(T, pred, lab, w, dtype=DTYPES[(ni + T) % 5])
    bound = n * 2.0 ** -53 * np.abs(w.astype(np.float64)).sum()     # at most n additions, each rounded once
    print("weights", T, n, np.abs(got - ref).max(), bound)
    assert np.abs(got - ref).max() <= bound
    assert confusion(T, pred, lab, w, dtype=DTYPES[(ni + T) % 5])[1].tobytes() == got.tobytes()


def value_reference(tp, fp, tn, fn, curve, method):
    """(the sum of the curve's terms, the sum of their magnitudes)."""
    def div0(a, b):
        return np.divide(a, b, out=np.zeros_like(a), where=b != 0)
    eps = 1e-6
    rec = (tp + eps) / (tp + fn + eps)
    if (curve, method) == ("PR", "careful_interpolation"):
        p = tp + fp
        dtp = tp[:-1] - tp[1:]
        slope = div0(dtp, np.maximum(p[:-1] - p[1:], 0))
        intercept = tp[1:] - slope * p[1:]
        ratio = np.where((p[:-1] > 0) & (p[1:] > 0), div0(p[:-1], p[1:]), 1.0)
        terms = div0(slope * (dtp + intercept * np.log(ratio)), np.maximum(tp[1:] + fn[1:], 0))
    else:
        x, y = (fp / (fp + tn + eps), rec) if curve == "ROC" else (rec, (tp + eps) / (tp + fp + eps))
        mean = {"minoring": np.minimum, "majoring": np.maximum}.get(method, lambda a, b: (a + b) / 2)
        terms = (x[:-1] - x[1:]) * mean(y[:-1], y[1:])
    return terms.sum(), np.abs(terms).sum()


@pytest.mark.parametrize("curve,method", CURVES)
@pytest.mark.parametrize("labels", ["mixed", "all positive", "all negative"])
@pytest.mark.parametrize("T,weighted", [(200, False), (201, True), (2, False), (4096, True)])
def test_value(curve, method, labels, T, weighted):
    pred, lab, w = case(T, TILE + 1)[:3]
    lab = {"mixed": lab, "all positive": np.ones_like(lab), "all negative": np.zeros_like(lab)}[labels]
    m = efl.metrics.Auc(T, curve, method)
    v32 = m.update(*(torch.tensor(a).cuda() for a in ((lab, pred, w) if weighted else (lab, pred))))
    ref, mag = value_reference(*(c.cpu().numpy() for c in m.confusion()), curve, method)
    v64 = m.result64().item()
    print("value", curve, method, labels, T, v64, ref, T * 2.0 ** -50 * mag)
    assert abs(v64 - ref) <= T * 2.0 ** -50 * mag and np.isfinite(v64)
    assert v32.dtype == torch.float32 and v32.dim() == 0 and v32.is_cuda
    assert abs(np.float64(v32.item()) - v64) <= np.spacing(np.float32(v64))
    value, again = efl.metrics.auc(torch.tensor(lab).cuda(), torch.tensor(pred).cuda(),
                                   torch.tensor(w).cuda() if weighted else None, T, curve=curve,
                                   summation_method=method)
    assert value.item() == v32.item() and isinstance(again, efl.metrics.Auc)


# (name, n, groups): "mixed" indicators are negative, above 2^32, at both ends of int64, and interleaved
GAUC_CASES = [("mixed", 1, 1), ("one", 300, 1), ("singles", 100, 100), ("mixed", TILE - 1, 50), ("mixed", TILE, 50),
              ("mixed", TILE + 1, 50), ("mixed", 3 * TILE + 1, 700), ("big", 4 * TILE - 192, 40), ("one", 3 * TILE + 1, 1)]
IDS = np.array([-5, -(1 << 40), (1 << 33) + 7, 0, 1, np.iinfo(np.int64).max, np.iinfo(np.int64).min], np.int64)


@functools.lru_cache(maxsize=None)
def gauc_case(kind, n, groups):
    """(labels, predictions, indicators, total, count, kept groups): predictions from a few values (ties,
    -0.0 and 0.0, NaN, the infinities) and 32 levels; "big": one group of three tiles among small ones."""
    rng = np.random.default_rng(n + groups)
    ids = np.concatenate([IDS, rng.integers(-1 << 62, 1 << 62, max(groups - len(IDS), 0))])[:groups]
    ind = np.arange(n) if kind == "singles" else ids[rng.integers(0, groups, n)]
    if kind == "big":
        ind[rng.permutation(n)[:3 * TILE]] = 12345
    levels = np.concatenate([np.array([-0.0, 0.0, np.nan, np.nan, np.inf, -np.inf, 1.0], np.float32),
                             (rng.integers(0, 32, 64) / np.float32(32)).astype(np.float32)])
    pred, lab = levels[rng.integers(0, len(levels), n)], rng.choice(np.array([0, 1, 3]), n)
    key = pred.astype(np.float64)                       # the order with every NaN one value above +inf
    key[np.isinf(pred)] = np.sign(key[np.isinf(pred)]) * 1e300
    key[np.isnan(pred)] = np.inf
    total, count, kept = 0.0, 0, 0
    for g in np.unique(ind):
        a, b = key[(ind == g) & (lab != 0)], key[(ind == g) & (lab == 0)]
        if len(a) and len(b):
            u = (a[:, None] > b[None, :]).sum() + 0.5 * (a[:, None] == b[None, :]).sum()
            total, count, kept = total + (len(a) + len(b)) * (u / (len(a) * len(b))), count + len(a) + len(b), kept + 1
    return lab, pred, ind.astype(np.int64), total, count, kept


@pytest.mark.parametrize("ci", range(len(GAUC_CASES)))
def test_gauc(ci):
    lab, pred, ind, total, count, kept = gauc_case(*GAUC_CASES[ci])
    args = [torch.tensor(lab).cuda().to(DTYPES[ci % 5]), torch.tensor(pred).cuda(), torch.tensor(ind).cuda()]
    value, m = efl.metrics.gauc(*args)
    got = m.last_call().cpu().numpy()
    print("gauc", GAUC_CASES[ci], got, total, count, kept * 2.0 ** -52 * count)
    assert got[1] == count and abs(got[0] - total) <= kept * 2.0 ** -52 * count
    want = total / count if count else 0.0
    assert np.isfinite(value.item()) and abs(m.result64().item() - want) <= (kept + 1) * 2.0 ** -52
    assert value.dtype == torch.float32 and value.item() == np.float32(m.result64().item())
    fresh = efl.metrics.Gauc()
    fresh.update(*args)
    assert fresh.last_call().cpu().numpy().tobytes() == got.tobytes()        # the same bytes on a second call
    # the running metric: a second batch doubles both sums; reset clears them
    value2, m = efl.metrics.gauc(*args, metric=m)
    assert value2.item() == value.item() and m.last_call().cpu().numpy().tobytes() == got.tobytes()
    m.reset()
    assert m.result().item() == 0.0
