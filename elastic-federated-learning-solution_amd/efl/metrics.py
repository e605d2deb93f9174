"""efl.metrics: streaming AUC and grouped AUC on the GPU (csrc/auc.hip).

Reference: efls-train/python/efl/utils/metrics.py:25-58 exports `metrics.auc` (tf.metrics.auc of
TF 1.15, argument for argument) and `metrics.gauc`. TF's metric is a (value, update_op) pair over
graph variables; eager code has no update op, so the functions here return (value, metric) and take
the metric back on the next batch:

    value, m = efl.metrics.auc(labels, predictions)              # first batch
    value, m = efl.metrics.auc(labels, predictions, metric=m)    # every later one

`value` is a 0-dim float32 tensor on the GPU (TF's result dtype); nothing synchronises.

AUC is TF's: T = num_thresholds thresholds (-1e-7, i / (T - 1), 1 + 1e-7, rounded once to float32), an
element predicted positive at t iff prediction > thr[t], a label positive iff non-zero. The state is
the summed weight per (label, bucket of the prediction), which is all the [T, n] comparison leaves.

GAUC. The reference's gauc calls `_ops.gauc_calc`, an op it never defines, so the definition is ours.
A group is all elements of one call with the same indicator, wherever they lie. A group with P
positives and N negatives, P N > 0, has AUC_g = U / (P N): U counts 1 for each (positive, negative)
pair whose positive has the greater prediction and 1/2 for each pair with equal predictions (-0.0
equals 0.0; every NaN is one value above every number). Groups with P N = 0 are left out. A call adds
total = sum n_g AUC_g and count = sum n_g (n_g = P + N) to the running sums; the metric is their
quotient over all calls, the reference's `metrics.mean(aucs, counts)`, and 0 while the count is 0.

There is no CPU fallback: tensors off the GPU are refused.
"""
from __future__ import annotations

import torch

from efl import errors, exporter, lib

_CURVES = {"ROC": 0, "PR": 1}
_METHODS = {"trapezoidal": 0, "careful_interpolation": 1, "minoring": 2, "majoring": 3}
_LABEL_DT = {torch.float32: lib.DT_FLOAT, torch.int32: lib.DT_INT32, torch.uint8: lib.DT_UINT8,
             torch.int64: lib.DT_INT64, torch.bool: lib.DT_BOOL}


def _flat(who, name, t, like=None):
    """`t` as a flat, contiguous, 16-byte aligned device tensor of `like`'s size and device."""
    if not isinstance(t, torch.Tensor):
        raise errors.InvalidArgumentError(f"{who}: {name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise errors.InvalidArgumentError(f"{who}: {name} is on {t.device}; the metrics run on the GPU only")
    if like is not None and (t.numel() != like.numel() or t.device != like.device):
        raise errors.InvalidArgumentError(
            f"{who}: {name} has {t.numel()} elements on {t.device}, predictions {like.numel()} on {like.device}")
    t = t.contiguous().view(-1)
    return t.clone() if t.data_ptr() % 16 else t


def _inputs(who, labels, predictions):
    if isinstance(predictions, torch.Tensor) and predictions.dtype != torch.float32:
        raise errors.InvalidArgumentError(f"{who}: predictions must be float32, got {predictions.dtype}")
    p = _flat(who, "predictions", predictions)
    lab = _flat(who, "labels", labels, p)
    if lab.dtype not in _LABEL_DT:
        raise errors.InvalidArgumentError(f"{who}: labels must be bool, uint8, int32, int64 or float32, got {lab.dtype}")
    return p, lab, _LABEL_DT[lab.dtype]


@exporter.export("metrics.Auc")
class Auc:
    """The running tf.metrics.auc. update() adds a batch and returns the value so far."""

    def __init__(self, num_thresholds=200, curve="ROC", summation_method="trapezoidal"):
        if curve not in _CURVES:
            raise errors.InvalidArgumentError(f'metrics.auc: curve must be "ROC" or "PR", got {curve!r}')
        if summation_method not in _METHODS:
            raise errors.InvalidArgumentError(
                f"metrics.auc: summation_method must be one of {sorted(_METHODS)}, got {summation_method!r}")
        if not isinstance(num_thresholds, int) or not 2 <= num_thresholds <= 4096:
            raise errors.InvalidArgumentError(f"metrics.auc: num_thresholds must be in [2, 4096], got {num_thresholds!r}")
        self.num_thresholds, self.curve, self.summation_method = num_thresholds, curve, summation_method
        self._state = self._work = None

    def _alloc(self, dev):
        T = self.num_thresholds
        if self._state is None:
            self._state = torch.zeros(2, T + 1, dtype=torch.float64, device=dev)
            self._conf = torch.empty(4, T, dtype=torch.float64, device=dev)
            self._v32 = torch.empty((), dtype=torch.float32, device=dev)
            self._v64 = torch.empty((), dtype=torch.float64, device=dev)
        elif self._state.device != dev:
            raise errors.InvalidArgumentError(f"metrics.auc: the metric lives on {self._state.device}, the batch on {dev}")

    def update(self, labels, predictions, weights=None):
        p, lab, code = _inputs("metrics.auc", labels, predictions)
        w = None
        if weights is not None:
            if isinstance(weights, torch.Tensor) and weights.dtype != torch.float32:
                raise errors.InvalidArgumentError(f"metrics.auc: weights must be float32, got {weights.dtype}")
            w = _flat("metrics.auc", "weights", weights, p)
        self._alloc(p.device)
        need = lib.raw().efl_auc_work_elems(p.numel(), self.num_thresholds)
        if need < 0:
            lib.check(need)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float64, device=p.device)
        lib.check(lib.raw().efl_auc_update(p.data_ptr(), lab.data_ptr(), code, w.data_ptr() if w is not None else None,
                                           p.numel(), self.num_thresholds, self._state.data_ptr(),
                                           self._work.data_ptr(), self._work.numel(), lib.stream_handle(p.device)))
        return self.result()

    def _value(self):
        if self._state is None:
            self._alloc(lib.require_gpu())
        lib.check(lib.raw().efl_auc_value(self._state.data_ptr(), self.num_thresholds, _CURVES[self.curve],
                                          _METHODS[self.summation_method], self._v32.data_ptr(), self._v64.data_ptr(),
                                          self._conf.data_ptr(), lib.stream_handle(self._state.device)))

    def result(self):
        """The value over every batch so far: a 0-dim float32 device tensor."""
        self._value()
        return self._v32.clone()

    def result64(self):
        """The same value before its rounding to float32."""
        self._value()
        return self._v64.clone()

    def confusion(self):
        """(tp, fp, tn, fn), each float64 [num_thresholds]."""
        self._value()
        return tuple(self._conf.clone().unbind(0))

    def reset(self):
        if self._state is not None:
            self._state.zero_()


@exporter.export("metrics.auc")
def auc(labels, predictions, weights=None, num_thresholds=200, metrics_collections=None, updates_collections=None,
        curve="ROC", name=None, summation_method="trapezoidal", metric=None):
    """tf.metrics.auc's arguments in the reference's order (the collections and the name are accepted and
    ignored). Returns (value, metric); pass `metric` back with the next batch."""
    if metric is None:
        metric = Auc(num_thresholds, curve, summation_method)
    elif (metric.num_thresholds, metric.curve, metric.summation_method) != (num_thresholds, curve, summation_method):
        raise errors.InvalidArgumentError("metrics.auc: metric= was made with other num_thresholds, curve or summation_method")
    return metric.update(labels, predictions, weights), metric


@exporter.export("metrics.Gauc")
class Gauc:
    """The running grouped AUC (the definition is the module's docstring)."""

    def __init__(self):
        self._state = self._scratch = None

    def _alloc(self, dev):
        if self._state is None:
            self._state = torch.zeros(2, dtype=torch.float64, device=dev)
            self._call = torch.zeros(2, dtype=torch.float64, device=dev)
            self._v32 = torch.zeros((), dtype=torch.float32, device=dev)
            self._v64 = torch.zeros((), dtype=torch.float64, device=dev)
        elif self._state.device != dev:
            raise errors.InvalidArgumentError(f"metrics.gauc: the metric lives on {self._state.device}, the batch on {dev}")

    def update(self, labels, predictions, indicators):
        p, lab, code = _inputs("metrics.gauc", labels, predictions)
        if isinstance(indicators, torch.Tensor) and indicators.dtype != torch.int64:
            raise errors.InvalidArgumentError(f"metrics.gauc: indicators must be int64, got {indicators.dtype}")
        ind = _flat("metrics.gauc", "indicators", indicators, p)
        if p.numel() > lib.GAUC_MAX_N:
            raise errors.InvalidArgumentError(f"metrics.gauc: {p.numel()} elements: one call takes at most 2^22")
        self._alloc(p.device)
        need = lib.raw().efl_gauc_scratch_bytes(p.numel())
        if need < 0:
            lib.check(need)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=p.device)
        lib.check(lib.raw().efl_gauc_update(p.data_ptr(), lab.data_ptr(), code, ind.data_ptr(), p.numel(),
                                            self._state.data_ptr(), self._call.data_ptr(), self._v32.data_ptr(),
                                            self._v64.data_ptr(), self._scratch.data_ptr(), self._scratch.numel(),
                                            lib.stream_handle(p.device)))
        return self._v32.clone()

    def last_call(self):
        """(total, count) of the last update as a float64 [2] device tensor."""
        if self._state is None:
            self._alloc(lib.require_gpu())
        return self._call.clone()

    def result(self):
        if self._state is None:
            self._alloc(lib.require_gpu())
        return self._v32.clone()

    def result64(self):
        if self._state is None:
            self._alloc(lib.require_gpu())
        return self._v64.clone()

    def reset(self):
        if self._state is not None:
            for t in (self._state, self._call, self._v32, self._v64):
                t.zero_()


@exporter.export("metrics.gauc")
def gauc(labels, predictions, indicators, metrics_collections=None, updates_collections=None, name=None, metric=None):
    """The reference's arguments in its order (the collections and the name are accepted and ignored).
    Returns (value, metric); pass `metric` back with the next batch."""
    if metric is None:
        metric = Gauc()
    return metric.update(labels, predictions, indicators), metric
