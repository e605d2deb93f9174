"""CPU: efl_dp_clip_sum checks its arguments before any HIP call, and the DP optimisers'
microbatch_gradients="batched" gives the loop's gradients on CPU records (the restated loop of
_SumQuery.accumulate_batch over one batched autograd.grad)."""
import ctypes

import pytest
import torch


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    p = ctypes.c_void_p(64)

    def call(var=(64, 64, 8, 8), nvars=1, rows=2, clip_mode=1, clip=1.0, noise_mode=1, div=2.0, scales=p, work=p,
             work_elems=2, table=True):
        arr = (efl.lib.DpVar * 1)()
        arr[0].grads, arr[0].out, arr[0].numel, arr[0].row_stride = var
        return lib.efl_dp_clip_sum(arr if table else None, nvars, rows, clip_mode, clip, noise_mode, 1.0, div, 7, scales,
                                   work, work_elems, None)

    bad = [dict(var=(None, 64, 8, 8)), dict(var=(64, None, 8, 8)), dict(var=(64, 68, 8, 8)), dict(var=(64, 64, 8, 7)),
           dict(var=(64, 64, -1, 8)), dict(table=False), dict(rows=0), dict(nvars=-1), dict(clip_mode=3),
           dict(clip_mode=-1), dict(noise_mode=2), dict(div=0.0), dict(div=float("nan")), dict(clip=0.0),
           dict(scales=None), dict(clip_mode=2, scales=None), dict(work=None), dict(work_elems=1)]
    for kw in bad:
        assert call(**kw) == -3, kw
        assert lib.efl_last_error().decode()
    assert call(nvars=0, table=False) == 0                    # no variables: a no-op
    assert call(var=(None, None, 0, 0)) == 0                  # an empty variable is skipped
    numels = (ctypes.c_int64 * 3)(3, 8192, 8193)
    assert lib.efl_dp_clip_work_elems(numels, 3, 5) == 5 * (1 + 1 + 2)
    assert lib.efl_dp_clip_work_elems(numels, 3, 0) == -3


@pytest.mark.parametrize("batch,nm", [(8, 4), (7, 4)])
def test_batched_equals_loop_on_cpu(batch, nm):
    """A noise-free clipping query on CPU: both paths give equal gradients, also for a batch that
    num_microbatches does not divide (every example its own microbatch) and an unused variable. The
    model is element-wise, so a row's gradient has at most two non-zero terms and is the same float
    in any order: the paths' own code is under test here, not the summation order of torch's matmul
    and convolution backward, which depends on the call's shape and on the CPU."""
    from efl.privacy import dp_optimizer as dpo

    class Clip(dpo.GaussianSumQuery):
        def get_noised_result(self, sample_state, global_state, divisor=1.0):
            return [v / divisor for v in sample_state], global_state

    got = {}
    for path in dpo.MICROBATCH_GRADIENTS:
        torch.manual_seed(1)
        vs = [torch.randn(5, requires_grad=True), torch.randn(5, requires_grad=True), torch.zeros(2, requires_grad=True)]
        x = torch.randn(batch, 5)
        loss = (torch.tanh(x * vs[0] + vs[1]) ** 2).sum(1)
        opt = dpo.DPGradientDescentOptimizer(Clip(0.5, 0.0), nm, params=vs, lr=0.1, microbatch_gradients=path)
        got[path] = [g for g, _ in opt.compute_gradients(loss, vs)]
    assert all(torch.equal(a, b) for a, b in zip(got["loop"], got["batched"]))
    with pytest.raises(ValueError, match="microbatch_gradients"):
        dpo.DPGradientDescentOptimizer(Clip(0.5, 0.0), nm, lr=0.1, microbatch_gradients="vmap")
