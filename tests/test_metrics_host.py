"""CPU: the argument checks of efl_auc_* and efl_gauc_* (csrc/auc.hip), which run before any HIP call,
efl.metrics' refusals in Python, and its names in the exporter's registry."""
import ctypes

import pytest
import torch

import efl

P = ctypes.c_void_p(64)


def auc_update(pred=P, labels=P, dtype=4, weights=None, n=10, T=200, state=P, work=P, work_elems=1 << 20):
    return efl.lib.raw().efl_auc_update(pred, labels, dtype, weights, n, T, state, work, work_elems, None)


def auc_value(state=P, T=200, curve=0, method=0, v=P, v64=P, conf=P):
    return efl.lib.raw().efl_auc_value(state, T, curve, method, v, v64, conf, None)


def gauc_update(pred=P, labels=P, dtype=9, ind=P, n=10, state=P, out=P, v=P, v64=P, scratch=P, nbytes=1 << 20):
    return efl.lib.raw().efl_gauc_update(pred, labels, dtype, ind, n, state, out, v, v64, scratch, nbytes, None)


@pytest.mark.parametrize("call,kw", [(f, kw) for f, kws in [
    (auc_update, [dict(T=1), dict(T=4097), dict(n=-1), dict(n=1 << 31), dict(dtype=2), dict(state=None), dict(pred=None),
                  dict(labels=None), dict(pred=72), dict(weights=72), dict(labels=66), dict(dtype=3, labels=68),
                  dict(work=None), dict(work_elems=401), dict(state=68)]),
    (auc_value, [dict(T=1), dict(T=4097), dict(curve=2), dict(curve=-1), dict(method=4), dict(state=None), dict(v=None),
                 dict(v64=None), dict(conf=None), dict(v64=68)]),
    (gauc_update, [dict(n=-1), dict(n=(1 << 22) + 1), dict(dtype=5), dict(state=None), dict(v=None), dict(pred=None),
                   dict(labels=None), dict(ind=None), dict(ind=68), dict(labels=68), dict(scratch=None), dict(scratch=72),
                   dict(nbytes=100)])] for kw in kws])
def test_argument_errors_without_gpu(call, kw):
    assert call(**kw) == -3, kw
    assert efl.lib.raw().efl_last_error().decode()


def test_sizes_and_no_ops():
    lib = efl.lib.raw()
    assert "2^22" in (gauc_update(n=(1 << 22) + 1), lib.efl_last_error().decode())[1]
    assert auc_update(n=0, pred=None, labels=None, work=None) == 0
    # one workgroup per tile up to 512 of them; T = 4096 caps the work buffer at 2^20 doubles
    assert lib.efl_auc_work_elems(efl.lib.AUC_TILE + 1, 200) == 2 * 402
    assert lib.efl_auc_work_elems(1 << 24, 200) == 512 * 402
    assert lib.efl_auc_work_elems(1 << 24, 4096) == 127 * 8194
    assert lib.efl_auc_work_elems(0, 200) == 0 and lib.efl_auc_work_elems(5, 1) == -3
    # two key buffers, neg [n + 1] int32, cloc [n] int64, two tables of tiles + 1, one slot per 256 places
    assert lib.efl_gauc_scratch_bytes(10) == 160 + 160 + 48 + 80 + 16 + 16 + 16
    assert lib.efl_gauc_scratch_bytes(0) == 0 and lib.efl_gauc_scratch_bytes((1 << 22) + 1) == -3


@pytest.mark.parametrize("make", [
    lambda: efl.metrics.Auc(curve="roc"), lambda: efl.metrics.Auc(summation_method="simpson"),
    lambda: efl.metrics.Auc(num_thresholds=1), lambda: efl.metrics.Auc(num_thresholds=4097),
    lambda: efl.metrics.auc(torch.zeros(4), torch.zeros(4)),                              # off the GPU
    lambda: efl.metrics.auc(torch.zeros(4), torch.zeros(4, dtype=torch.float64)),
    lambda: efl.metrics.gauc(torch.zeros(4), torch.zeros(4), torch.zeros(4, dtype=torch.int64)),
    lambda: efl.metrics.gauc(torch.zeros(4), torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.int64)),
    lambda: efl.metrics.Auc().update([0, 1], torch.zeros(2)),
])
def test_python_refusals(make):
    with pytest.raises(efl.errors.InvalidArgumentError):
        make()


def test_names_resolve_through_the_exporter():
    from efl import exporter, metrics
    for name in ("auc", "gauc", "Auc", "Gauc"):
        assert getattr(efl.metrics, name) is exporter._registry["metrics." + name] is getattr(metrics, name)
    assert efl.metrics.auc is efl.metrics.auc
