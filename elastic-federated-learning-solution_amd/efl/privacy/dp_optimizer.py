"""DP-SGD optimisers: per-microbatch gradients, summed (clipped for the Gaussian query), noised and
averaged, then the wrapped optimiser's update.

Reference: efls-train/python/efl/privacy/dp_optimizer.py
  GaussianSumQuery (:54-57) = tensorflow_privacy 0.3.0's (setup.py:26) with zero initial state:
    per record clip_by_global_norm(record, l2_norm_clip), sum, + N(0, stddev^2), stddev = clip * mult;
  ElementWiseGaussianSumQuery (:60-73): sum, then v + normal(shape) * v * noise_multiplier;
  make_optimizer_class (:80-220): compute_gradients splits the per-example loss into
    num_microbatches rows (:148-157; all rows when the batch does not divide), takes each row's
    gradient (:170-183), accumulates it through the query, noises the sums (:206-208) and divides
    by num_microbatches (:210-216);
  make_gaussian_optimizer_class (:224-256): ElementWise query without l2_norm_clip, Gaussian with it;
  DPAdagrad / DPAdam / DPGradientDescent (+ Gaussian) optimisers (:258-284).

The noise and the division run as ONE HIP kernel per variable (csrc/mask.hip efl_dp_noise: read the
sum once, write the averaged noised gradient once) with TF's normal construction (Philox4x32-10,
Box-Muller) from a per-process `NoiseStream`. No CPU fallback: the kernel needs the GPU.

The per-microbatch gradients come one of three ways (`microbatch_gradients=`, process default by
`set_microbatch_gradients`). "loop", the default: one autograd.grad per microbatch, the clip a
torch reduction and the sum a torch addition per variable, as the reference's loop. "batched": ONE
autograd.grad with is_grads_batched=True gives every variable's gradients stacked as [rows, ...],
and for float32 device records the norms, the clip scales, the row-ordered sum, the noise and the
division are two or three HIP launches whatever the model (csrc/dpclip.hip efl_dp_clip_sum,
`dp_clip_sum_noise`): the same sum as the loop's given the same scales, the scales from a double
accumulation instead of float32 reductions. Custom queries and other dtypes take
`_SumQuery.accumulate_batch`, the loop restated over the stack. "factored", for models whose
variables are all weights and biases of torch.nn.Linear layers given as `dense_layers=`: forward hooks
keep each layer's input X and output, ONE ordinary autograd.grad of the loss to the outputs gives D,
and the norms (from the layers' r x r Gram matrices), the clipped sum (one fp32-MFMA GEMM D^T diag(s) X
per layer), the noise and the division are csrc/dpdense.hip's efl_dp_dense_clip_sum
(`dp_dense_clip_sum_noise`): no [rows, out, in] stack exists at any point. It needs microbatches of at
most 16 examples, the stock queries, float32, and examples that are independent in the forward pass
(no batch statistics), which cannot be checked; anything else raises InvalidArgumentError, as there is
no stack to fall back on. torch.nn.Conv2d layers (groups = 1, zero padding) given as `conv_layers=` take
the same path through csrc/dpconv.hip's efl_dp_conv_clip_sum (`dp_conv_clip_sum_noise`): the norm pass
forms each microbatch's [Cout, Cin kh kw] gradient on chip in double and drops it, the sum is one implicit
GEMM over all (example, output position) pairs. A model of both kinds clips under ONE norm: both families
write their partial sums of squares into one buffer, one launch makes the scales, and both sums take them
(`dp_factored_clip_sum_noise`). torch.nn.Embedding and torch.nn.EmbeddingBag (modes "sum" and "mean", 2-D
input) tables given as `embedding_layers=` are the third family (csrc/dpembed.hip's efl_dp_embed_clip_sum,
`dp_embed_clip_sum_noise`): a microbatch's gradient of a table is zero but for the rows its ids name, so the
norm and the clipped sum come from a sort of the step's at most 8,192 (id, entry) keys per table and the
entries' rows of d, and the only dense pass is the noise, one write of the table and no read. A recommender
of tables and an MLP runs under one norm. A Linear of `dense_layers=` applied at every position of a sequence
(input [B, *, in]: T positions per example) is the fourth (csrc/dpseq.hip's efl_dp_seq_clip_sum): a microbatch
of r examples has P = r T rows (at most 8,192), its norm is sum Gd (Gx + 1) over the [P, P] Grams of the rows
of X and of D, formed in 64 x 64 blocks on the fp64 matrix cores and never stored, and its sum is the GEMM
D^T diag(s) X over all B T rows, split over groups of microbatches. torch.nn.LayerNorm (over the last
dimension) and torch.nn.GroupNorm modules given as `norm_layers=` are the fifth (csrc/dpnorm.hip's
efl_dp_norm_clip_sum, `dp_norm_clip_sum_noise`): the gradient of their scale and bias is a column reduction of
d (x - mean) / sqrt(var + eps) and of d over a microbatch's elements, with the statistics and the sums in
double; each microbatch's [C] results are stacked (rows x 2 C floats, the only per-microbatch storage of the
path) and efl_dp_clip_sum adds them. A model with any other variable is out of its scope.

Torch mapping. TF optimisers get their variables at minimize time; torch ones at construction.
These classes take either: `params` (as `params=`, or first positional with the DP arguments as
keywords, torch style: `DPAdamGaussianOptimizer(model.parameters(), noise_multiplier=1.0, lr=..)`),
or none (the reference's call shape, e.g. `DPGradientDescentGaussianOptimizer(noise_multiplier=1.0,
learning_rate=0.25)`), in which case the wrapped optimiser is built on the first
`compute_gradients` / `minimize` var_list. `learning_rate` is accepted for `lr`. Float64 (and
half-precision) variables train: their noise is TF's float32 normal cast to the variable's dtype,
and the clip norm is taken in float64 for float64 records.

One reference quirk is kept: each microbatch's loss is `reduce_func(tf.gather(loss, [i]), axis=0)`
(:172), a reduction over a length-1 axis, so 'mean' and 'sum' both leave the row as it is and its
gradient is that of the row's SUM (TF differentiates a non-scalar loss as its sum).
"""
from __future__ import annotations

import ctypes

import torch

from efl import errors, exporter, lib
from efl.privacy.secret_sharing import NoiseStream

_stream = NoiseStream()


@exporter.export("privacy.set_noise_seed")
def set_noise_seed(seed: int | None, counter: int = 0) -> None:
    """Fix (or, with None, re-randomise) this process's DP noise stream."""
    _stream.reset(seed, counter)


def noise_stream() -> NoiseStream:
    return _stream


def dp_noise(x: torch.Tensor, mode: int, sigma: float, divisor: float = 1.0, stream: NoiseStream | None = None):
    """efl_dp_noise over one float32 tensor: mode 0 (x + z x sigma) / divisor, mode 1
    (x + z sigma) / divisor, z ~ N(0, 1) drawn from `stream` (default: the process's)."""
    x = lib.as_tensor(x)
    if not x.dtype.is_floating_point:
        raise errors.InvalidArgumentError(f"DP noise needs a floating-point gradient, got {x.dtype}")
    if x.dtype != torch.float32:
        # the reference draws tf.random.normal(..., dtype=v.dtype); the kernel draws TF's float32
        # normal, so other float dtypes are noised in float32 and cast back (float64 variables keep
        # float32-accurate noise; parity with TF's noise stream is distributional either way)
        return dp_noise(x.float(), mode, sigma, divisor, stream).to(x.dtype)
    v, home = lib.on_device(x.detach())
    v = v.contiguous()
    if v.data_ptr() % 16:
        v = v.clone()
    seed, ctr0 = (stream or _stream).take(v.numel())
    out = torch.empty_like(v)
    lib.check(lib.raw().efl_dp_noise(v.data_ptr(), out.data_ptr(), v.numel(), int(mode), float(sigma),
                                     float(divisor), seed, ctr0, lib.stream_handle(v.device)))
    return lib.back(out, home)


MICROBATCH_GRADIENTS = ("loop", "batched")       # for any model and any query
DENSE_MICROBATCH_GRADIENTS = ("factored",)        # for models of registered Linear layers (dense_layers=)
MAX_ROWS_PER_MICROBATCH = 16                      # efl_dp_dense_clip_sum's limit on batch rows per microbatch
MAX_EMBEDDING_ENTRIES = lib.DP_EMBED_MAX_ENTRIES  # efl_dp_embed_clip_sum's limit on looked-up ids per table and step
MAX_SEQUENCE_ROWS = lib.DP_SEQ_MAX_ROWS           # efl_dp_seq_clip_sum's limit on (example, position) rows per microbatch
_microbatch_gradients = "loop"


@exporter.export("privacy.set_microbatch_gradients")
def set_microbatch_gradients(name: str) -> None:
    """The process default of the DP optimisers' `microbatch_gradients` keyword: "loop" (one
    autograd.grad and one torch clip-and-add per microbatch, the default), "batched" (one batched
    autograd.grad, then efl_dp_clip_sum over the stacked gradients) or "factored" (one ordinary
    autograd.grad to the outputs of the layers registered as dense_layers=, conv_layers=,
    embedding_layers= and norm_layers=, then efl_dp_dense_clip_sum, efl_dp_seq_clip_sum, efl_dp_conv_clip_sum,
    efl_dp_embed_clip_sum and efl_dp_norm_clip_sum under one shared clip norm; a model with any other
    variable is refused)."""
    global _microbatch_gradients
    _microbatch_gradients = _resolve_microbatch_gradients(name)


def _resolve_microbatch_gradients(name):
    name = _microbatch_gradients if name is None else name
    if name not in MICROBATCH_GRADIENTS + DENSE_MICROBATCH_GRADIENTS:
        raise ValueError(f"microbatch_gradients must be one of {MICROBATCH_GRADIENTS + DENSE_MICROBATCH_GRADIENTS}, "
                         f"got {name!r}")
    return name


def _rows_view(t):
    """(view, numel, row_stride) of a [rows, ...] float32 device tensor as efl_dp_clip_sum reads it:
    a view whose rows are contiguous and at least numel apart is taken as it is (a padded row
    stride included), anything else is made contiguous."""
    rows = t.shape[0]
    numel = t[0].numel() if rows else 0
    if rows and numel and not (t[0].is_contiguous() and (rows == 1 or t.stride(0) >= numel)):
        t = t.contiguous()
    return t, numel, int(t.stride(0)) if rows > 1 and numel else numel


@exporter.export("privacy.dp_clip_sum_noise")
def dp_clip_sum_noise(stacked, l2_norm_clip, mode: int, sigma: float, divisor: float = 1.0,
                      stream: NoiseStream | None = None, scales=None, return_scales: bool = False):
    """efl_dp_clip_sum over a record's stacked microbatch gradients: `stacked` is a list of
    [rows, ...] float32 device tensors, one per variable. Returns, per variable,
    noise(sum over rows, in row order, of g_r * scale_r) / divisor with efl_dp_noise's `mode`, `sigma`
    and `divisor`; the noise positions are taken from `stream` (default: the process's) as the loop
    path takes them, one take(numel) per variable, in order.
    scale_r: 1 with l2_norm_clip None and no `scales`; `scales` ([rows] float32) when given; else
    clip * min(1 / ||g_r||, 1 / clip), the norm over all variables of row r accumulated in double.
    return_scales: also return the [rows] scales used (ones when there are none)."""
    stacked = [lib.as_tensor(t).detach() for t in stacked]
    if not stacked:
        return ([], None) if return_scales else []
    dev, rows = stacked[0].device, stacked[0].shape[0] if stacked[0].dim() else 0
    for t in stacked:
        if t.dtype != torch.float32 or t.device != dev or dev.type != "cuda" or t.dim() < 1 or t.shape[0] != rows:
            raise errors.InvalidArgumentError(
                "dp_clip_sum_noise: every variable is a [rows, ...] float32 tensor on one ROCm device")
    if rows < 1:
        raise errors.InvalidArgumentError("dp_clip_sum_noise: no rows")
    views = [_rows_view(t) for t in stacked]
    outs = lib._carve([t[0] for t in stacked], torch.float32, dev)
    arr = (lib.DpVar * len(views))()
    seed = None
    for rec, (t, numel, stride), out in zip(arr, views, outs):
        seed, ctr0 = (stream or _stream).take(numel)
        rec.grads, rec.out, rec.numel, rec.row_stride, rec.ctr0 = t.data_ptr(), out.data_ptr(), numel, stride, ctr0
    clip_mode = 2 if scales is not None else 0 if l2_norm_clip is None else 1
    work, work_elems = None, 0
    if clip_mode == 2:
        scales = lib.as_tensor(scales).detach().to(dev, torch.float32).contiguous()
        if scales.shape != (rows,):
            raise errors.InvalidArgumentError(f"dp_clip_sum_noise: scales must be [{rows}]")
    elif clip_mode == 1:
        numels = (ctypes.c_int64 * len(views))(*[v[1] for v in views])
        work_elems = lib.raw().efl_dp_clip_work_elems(numels, len(views), rows)
        if work_elems < 0:
            lib.check(int(work_elems))
        work = torch.empty(max(work_elems, 1), dtype=torch.float64, device=dev)
        scales = torch.empty(rows, dtype=torch.float32, device=dev)
    lib.check(lib.raw().efl_dp_clip_sum(arr, len(views), rows, clip_mode, float(l2_norm_clip or 0.0), int(mode),
                                        float(sigma), float(divisor), seed,
                                        None if scales is None else scales.data_ptr(),
                                        None if work is None else work.data_ptr(), work_elems,
                                        lib.stream_handle(dev)))
    if return_scales:
        return outs, torch.ones(rows, device=dev) if scales is None else scales
    return outs


def _rows_2d(t):
    """A [B, width] float32 device tensor as efl_dp_dense_clip_sum reads it: rows contiguous and at
    least `width` apart (a padded row stride is taken as it is), anything else made contiguous."""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or t.data_ptr() % 4:
        t = t.contiguous()
    return t


def _dense_table(layers, ctrs):
    """The DpDense table of checked dense layers with freshly carved outputs: (table, [(w_grad, b_grad |
    None)], tensors to keep alive)."""
    dev = layers[0][0].device
    like = []
    for x, d, has_bias in layers:
        like.append(torch.empty(d.shape[1], x.shape[1], device="meta"))
        if has_bias:
            like.append(torch.empty(d.shape[1], device="meta"))
    flat = iter(lib._carve(like, torch.float32, dev))
    arr, outs, keep = (lib.DpDense * len(layers))(), [], []
    for rec, (x, d, has_bias), (cw, cb) in zip(arr, layers, ctrs):
        x, d = _rows_2d(x), _rows_2d(d)
        keep += [x, d]
        w, b = next(flat), next(flat) if has_bias else None
        rec.x, rec.x_row_stride, rec.d, rec.d_row_stride = x.data_ptr(), max(x.stride(0), x.shape[1]), d.data_ptr(), max(d.stride(0), d.shape[1])
        rec.w_out, rec.b_out, rec.in_, rec.out = w.data_ptr(), None if b is None else b.data_ptr(), x.shape[1], d.shape[1]
        rec.ctr0_w, rec.ctr0_b = cw, cb
        outs.append((w, b))
    return arr, outs, keep


def _dense_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, scales, table=None):
    """efl_dp_dense_clip_sum over checked layers [(x, d, has_bias)]; ctrs: per layer the first Philox
    block of (weight, bias); table: their _dense_table when the caller has made it. Returns
    ([(w_grad, b_grad | None)], scales | None)."""
    dev, B = layers[0][0].device, layers[0][0].shape[0]
    arr, outs, keep = table or _dense_table(layers, ctrs)
    clip_mode = 2 if scales is not None else 0 if l2_norm_clip is None else 1
    work, work_elems = None, 0
    if clip_mode == 2:
        scales = lib.as_tensor(scales).detach().to(dev, torch.float32).contiguous()
        if scales.shape != (rows,):
            raise errors.InvalidArgumentError(f"dp_dense_clip_sum_noise: scales must be [{rows}]")
    elif clip_mode == 1:
        work_elems = lib.raw().efl_dp_dense_work_elems(len(layers), rows)
        if work_elems < 0:
            lib.check(int(work_elems))
        work = torch.empty(max(work_elems, 1), dtype=torch.float64, device=dev)
        scales = torch.empty(rows, dtype=torch.float32, device=dev)
    lib.check(lib.raw().efl_dp_dense_clip_sum(arr, len(layers), B, rows, clip_mode, float(l2_norm_clip or 0.0),
                                              int(mode), float(sigma), float(divisor), seed,
                                              None if scales is None else scales.data_ptr(),
                                              None if work is None else work.data_ptr(), work_elems,
                                              lib.stream_handle(dev)))
    return outs, scales


def _check_dense_layers(layers, rows, who):
    """[(x, d, has_bias)] with detached tensors: x [B, in] and d [B, out] as they are (csrc/dpdense.hip's
    layers), x [B, *, in] and d [B, *, out] flattened to [B, T, .] (csrc/dpseq.hip's)."""
    layers = [(lib.as_tensor(x).detach(), lib.as_tensor(d).detach(), bool(has_bias)) for x, d, has_bias in layers]
    dev, B = layers[0][0].device, layers[0][0].shape[0] if layers[0][0].dim() else 0
    for k, (x, d, has_bias) in enumerate(layers):
        if x.dtype != torch.float32 or d.dtype != torch.float32:
            raise errors.InvalidArgumentError(f"{who}: x and d must be float32, got {x.dtype} and {d.dtype}")
        if x.device != dev or d.device != dev or dev.type != "cuda":
            raise errors.InvalidArgumentError(f"{who}: every x and d lies on one ROCm device")
        if x.dim() < 2 or d.dim() < 2 or x.shape[0] != B or d.shape[0] != B or 0 in x.shape or 0 in d.shape:
            raise errors.InvalidArgumentError(
                f"{who}: a layer takes x [B, in] and d [B, out] with B = {B}, got {tuple(x.shape)} and {tuple(d.shape)}")
        if x.shape[1:-1] != d.shape[1:-1]:
            raise errors.InvalidArgumentError(
                f"{who}: a layer over a sequence takes x [B, *, in] and d [B, *, out] with equal middle dimensions, "
                f"got {tuple(x.shape)} and {tuple(d.shape)}")
        if x.dim() > 2:
            layers[k] = (x.reshape(B, -1, x.shape[-1]), d.reshape(B, -1, d.shape[-1]), has_bias)
    rows = int(rows)
    if rows < 1 or B % rows:
        raise errors.InvalidArgumentError(f"{who}: {rows} microbatches do not divide the batch of {B}")
    if B // rows > MAX_ROWS_PER_MICROBATCH:
        raise errors.InvalidArgumentError(f"{who}: {B // rows} examples per microbatch, at most "
                                          f"{MAX_ROWS_PER_MICROBATCH} (r > {MAX_ROWS_PER_MICROBATCH})")
    for x, _, _ in layers:
        if x.dim() == 3 and B // rows * x.shape[1] > MAX_SEQUENCE_ROWS:
            raise errors.InvalidArgumentError(
                f"{who}: {B // rows} examples of {x.shape[1]} positions per microbatch, at most {MAX_SEQUENCE_ROWS} "
                f"rows (r T > {MAX_SEQUENCE_ROWS})")
    return layers, rows


def _seq_table(layers, ctrs):
    """The DpSeq table of checked sequence layers [(x [B, T, in], d [B, T, out], has_bias)] with freshly
    carved outputs: (table, [(w_grad, b_grad | None)], tensors to keep alive). A tensor whose positions are
    contiguous rows at least a width apart is taken as it lies (a padded row stride included)."""
    dev, like = layers[0][0].device, []
    for x, d, has_bias in layers:
        like.append(torch.empty(d.shape[2], x.shape[2], device="meta"))
        if has_bias:
            like.append(torch.empty(d.shape[2], device="meta"))
    flat = iter(lib._carve(like, torch.float32, dev))
    arr, outs, keep = (lib.DpSeq * len(layers))(), [], []

    def rows_of(t):     # the flattened [B T, width] rows and their stride
        B, T, width = t.shape
        s = t.stride(1) if T > 1 else t.stride(0) if B > 1 else width
        if t.stride(2) != 1 or s < width or (B > 1 and T > 1 and t.stride(0) != T * s) or t.data_ptr() % 4:
            t, s = t.contiguous(), width
        return t, s

    for rec, (x, d, has_bias), (cw, cb) in zip(arr, layers, ctrs):
        (x, xs), (d, ds) = rows_of(x), rows_of(d)
        keep += [x, d]
        w, b = next(flat), next(flat) if has_bias else None
        rec.x, rec.x_row_stride, rec.d, rec.d_row_stride = x.data_ptr(), xs, d.data_ptr(), ds
        rec.w_out, rec.b_out, rec.T, rec.in_, rec.out = w.data_ptr(), None if b is None else b.data_ptr(), x.shape[1], x.shape[2], d.shape[2]
        rec.ctr0_w, rec.ctr0_b = cw, cb
        outs.append((w, b))
    return arr, outs, keep


def _seq_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, scales, table=None):
    """efl_dp_seq_clip_sum over checked sequence layers; ctrs: per layer the first Philox block of (weight,
    bias); table: their _seq_table when the caller has made it. Returns ([(w_grad, b_grad | None)],
    scales | None)."""
    dev, B, raw = layers[0][0].device, layers[0][0].shape[0], lib.raw()
    arr, outs, keep = table or _seq_table(layers, ctrs)
    clip_mode = 2 if scales is not None else 0 if l2_norm_clip is None else 1
    work, work_elems = None, 0
    if clip_mode == 2:
        scales = lib.as_tensor(scales).detach().to(dev, torch.float32).contiguous()
        if scales.shape != (rows,):
            raise errors.InvalidArgumentError(f"dp_dense_clip_sum_noise: scales must be [{rows}]")
    elif clip_mode == 1:
        work_elems = _elems(raw.efl_dp_seq_work_elems(arr, len(layers), B, rows))
        work = torch.empty(max(work_elems, 1), dtype=torch.float64, device=dev)
        scales = torch.empty(rows, dtype=torch.float32, device=dev)
    pe = _elems(raw.efl_dp_seq_partial_elems(arr, len(layers), B, rows))
    partials = torch.empty(max(pe, 4), dtype=torch.float32, device=dev)
    lib.check(raw.efl_dp_seq_clip_sum(arr, len(layers), B, rows, clip_mode, float(l2_norm_clip or 0.0), int(mode),
                                      float(sigma), float(divisor), seed,
                                      None if scales is None else scales.data_ptr(),
                                      None if work is None else work.data_ptr(), work_elems, partials.data_ptr(), pe,
                                      lib.stream_handle(dev)))
    return outs, scales


@exporter.export("privacy.dp_dense_clip_sum_noise")
def dp_dense_clip_sum_noise(layers, rows: int, l2_norm_clip, mode: int, sigma: float, divisor: float = 1.0,
                            stream: NoiseStream | None = None, scales=None, return_scales: bool = False):
    """efl_dp_dense_clip_sum: a DP-SGD step's clipped, summed, noised and divided gradients of dense
    layers from their inputs and output gradients, without the per-microbatch gradients. `layers` is
    a list of (x [B, in], d [B, out], has_bias) float32 ROCm tensors, d the gradient of the SUM of the
    per-example losses by the layer's output; microbatch i is the B / rows (at most 16) consecutive
    rows from i * B / rows. Returns [(w_grad [out, in], b_grad [out] | None), ...]: per layer
    noise(sum_i scale_i D_i^T X_i) / divisor and noise(sum_i scale_i colsum(D_i)) / divisor with
    efl_dp_noise's `mode`, `sigma` and `divisor`; the noise positions are taken from `stream` (default:
    the process's) one take(numel) per variable, weight then bias, in layer order.
    scale_i: 1 with l2_norm_clip None and no `scales`; `scales` ([rows] float32) when given; else
    clip * min(1 / ||g_i||, 1 / clip), g_i microbatch i's gradient of all the layers' variables, its
    norm from the layers' Gram matrices in double. return_scales: also return the [rows] scales.
    A layer applied at every position of a sequence gives x [B, *, in] and d [B, *, out] with equal middle
    dimensions (T positions in all, at most 8,192 / (B / rows)): it takes efl_dp_seq_clip_sum
    (csrc/dpseq.hip), its norm from the [r T, r T] Grams on the fp64 matrix cores, under the same shared
    norm and at the same stream positions."""
    layers = list(layers)
    if not layers:
        return ([], None) if return_scales else []
    layers, rows = _check_dense_layers(layers, rows, "dp_dense_clip_sum_noise")
    ctrs, seed = [], None
    for x, d, has_bias in layers:
        seed, cw = (stream or _stream).take(d.shape[-1] * x.shape[-1])
        ctrs.append((cw, (stream or _stream).take(d.shape[-1])[1] if has_bias else 0))
    outs, _, _, _, scales = _factored_clip_sum(layers, [], rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, [], scales)
    if return_scales:
        return outs, torch.ones(rows, device=layers[0][0].device) if scales is None else scales
    return outs


def _pair(v, name):
    """An int or a pair of ints as Conv2d takes them, as (vertical, horizontal)."""
    try:
        v = (int(v), int(v)) if isinstance(v, int) else tuple(int(a) for a in v)
    except (TypeError, ValueError):
        v = ()
    if len(v) != 2:
        raise errors.InvalidArgumentError(f"{name} must be an int or a pair of ints")
    return v


def _conv_padding(padding, kernel, dilation, who):
    """Conv2d's padding as a pair of ints: "valid" is 0, "same" d (k - 1) / 2 (which has to be whole:
    torch pads the odd one on one side only, which no symmetric padding reproduces)."""
    if padding == "valid":
        return 0, 0
    if padding == "same":
        total = [d * (k - 1) for k, d in zip(kernel, dilation)]
        if any(t % 2 for t in total):
            raise errors.InvalidArgumentError(
                f'{who}: padding="same" with kernel {kernel} and dilation {dilation} pads d (k - 1) = {tuple(total)}, '
                f"odd in a dimension, unevenly")
        return total[0] // 2, total[1] // 2
    return _pair(padding, "padding")


def _check_conv_layers(layers, rows, who):
    """[(x, d, has_bias, kernel, stride, padding, dilation)] with detached tensors and pairs of ints."""
    out = []
    for x, d, has_bias, kernel, stride, padding, dilation in layers:
        x, d = lib.as_tensor(x).detach(), lib.as_tensor(d).detach()
        kernel, stride, dilation = _pair(kernel, "kernel_size"), _pair(stride, "stride"), _pair(dilation, "dilation")
        out.append((x, d, bool(has_bias), kernel, stride, _conv_padding(padding, kernel, dilation, who), dilation))
    dev, B = out[0][0].device, out[0][0].shape[0] if out[0][0].dim() else 0
    for x, d, *_ in out:
        if x.dtype != torch.float32 or d.dtype != torch.float32:
            raise errors.InvalidArgumentError(f"{who}: x and d must be float32, got {x.dtype} and {d.dtype}")
        if x.device != dev or d.device != dev or dev.type != "cuda":
            raise errors.InvalidArgumentError(f"{who}: every x and d lies on one ROCm device")
        if x.dim() != 4 or d.dim() != 4 or x.shape[0] != B or d.shape[0] != B or 0 in x.shape or 0 in d.shape:
            raise errors.InvalidArgumentError(
                f"{who}: a conv layer takes x [B, Cin, H, W] and d [B, Cout, Ho, Wo] with B = {B}, got "
                f"{tuple(x.shape)} and {tuple(d.shape)}")
    rows = int(rows)
    if rows < 1 or B % rows:
        raise errors.InvalidArgumentError(f"{who}: {rows} microbatches do not divide the batch of {B}")
    if B // rows > MAX_ROWS_PER_MICROBATCH:
        raise errors.InvalidArgumentError(f"{who}: {B // rows} examples per microbatch, at most "
                                          f"{MAX_ROWS_PER_MICROBATCH} (r > {MAX_ROWS_PER_MICROBATCH})")
    return out, rows


def _conv_table(layers, ctrs):
    """The DpConv table of checked conv layers with freshly carved outputs: (table, [(w_grad, b_grad |
    None)], tensors to keep alive)."""
    dev, like = layers[0][0].device, []
    for x, d, has_bias, kernel, *_ in layers:
        like.append(torch.empty(d.shape[1], x.shape[1], *kernel, device="meta"))
        if has_bias:
            like.append(torch.empty(d.shape[1], device="meta"))
    flat = iter(lib._carve(like, torch.float32, dev))
    arr, outs, keep = (lib.DpConv * len(layers))(), [], []
    for rec, (x, d, has_bias, kernel, stride, padding, dilation), (cw, cb) in zip(arr, layers, ctrs):
        x, d = x.contiguous(), d.contiguous()
        keep += [x, d]
        w, b = next(flat), next(flat) if has_bias else None
        rec.x, rec.d, rec.w_out, rec.b_out = x.data_ptr(), d.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr()
        _, rec.cin, rec.h, rec.w = x.shape
        _, rec.cout, rec.ho, rec.wo = d.shape
        (rec.kh, rec.kw), (rec.sh, rec.sw), (rec.ph, rec.pw), (rec.dh, rec.dw) = kernel, stride, padding, dilation
        rec.ctr0_w, rec.ctr0_b = cw, cb
        outs.append((w, b))
    return arr, outs, keep


def _elems(n):
    if n < 0:
        lib.check(int(n))
    return int(n)


def _conv_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, scales, table=None):
    """efl_dp_conv_clip_sum over checked layers; ctrs: per layer the first Philox block of (weight,
    bias); table: their _conv_table when the caller has made it. Returns ([(w_grad, b_grad | None)],
    scales | None)."""
    dev, B, raw = layers[0][0].device, layers[0][0].shape[0], lib.raw()
    arr, outs, keep = table or _conv_table(layers, ctrs)
    clip_mode = 2 if scales is not None else 0 if l2_norm_clip is None else 1
    work, work_elems = None, 0
    if clip_mode == 2:
        scales = lib.as_tensor(scales).detach().to(dev, torch.float32).contiguous()
        if scales.shape != (rows,):
            raise errors.InvalidArgumentError(f"dp_conv_clip_sum_noise: scales must be [{rows}]")
    elif clip_mode == 1:
        work_elems = _elems(raw.efl_dp_conv_work_elems(arr, len(layers), rows))
        work = torch.empty(max(work_elems, 1), dtype=torch.float64, device=dev)
        scales = torch.empty(rows, dtype=torch.float32, device=dev)
    pe = _elems(raw.efl_dp_conv_partial_elems(arr, len(layers), B, rows))
    partials = torch.empty(max(pe, 4), dtype=torch.float32, device=dev)
    lib.check(raw.efl_dp_conv_clip_sum(arr, len(layers), B, rows, clip_mode, float(l2_norm_clip or 0.0), int(mode),
                                       float(sigma), float(divisor), seed,
                                       None if scales is None else scales.data_ptr(),
                                       None if work is None else work.data_ptr(), work_elems, partials.data_ptr(), pe,
                                       lib.stream_handle(dev)))
    return outs, scales


def _take_layers(shapes, stream):
    """One take(numel) per variable, weight then bias, in layer order: (seed, [(ctr0_w, ctr0_b)])."""
    ctrs, seed = [], None
    for wn, bn in shapes:
        seed, cw = stream.take(wn)
        ctrs.append((cw, stream.take(bn)[1] if bn else 0))
    return seed, ctrs


def _conv_numels(layers):
    return [(d.shape[1] * x.shape[1] * k[0] * k[1], d.shape[1] if has_bias else 0) for x, d, has_bias, k, *_ in layers]


@exporter.export("privacy.dp_conv_clip_sum_noise")
def dp_conv_clip_sum_noise(layers, rows: int, l2_norm_clip, mode: int, sigma: float, divisor: float = 1.0,
                           stream: NoiseStream | None = None, scales=None, return_scales: bool = False):
    """efl_dp_conv_clip_sum: a DP-SGD step's clipped, summed, noised and divided gradients of Conv2d
    layers (groups = 1, zero padding) from their inputs and output gradients, without the per-microbatch
    gradients. `layers` is a list of (x [B, Cin, H, W], d [B, Cout, Ho, Wo], has_bias, kernel_size,
    stride, padding, dilation): float32 ROCm tensors, d the gradient of the SUM of the per-example losses
    by the layer's output, the rest as Conv2d takes them. Microbatch i is the B / rows (at most 16)
    consecutive examples from i * B / rows. Returns [(w_grad [Cout, Cin, kh, kw], b_grad [Cout] | None)];
    mode, sigma, divisor, scales, return_scales and the stream positions (one take(numel) per variable,
    weight then bias, in layer order) are dp_dense_clip_sum_noise's. The norms come from the gradients
    themselves, formed on chip in double and never stored."""
    layers = list(layers)
    if not layers:
        return ([], None) if return_scales else []
    layers, rows = _check_conv_layers(layers, rows, "dp_conv_clip_sum_noise")
    seed, ctrs = _take_layers(_conv_numels(layers), stream or _stream)
    outs, scales = _conv_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, scales)
    if return_scales:
        return outs, torch.ones(rows, device=layers[0][0].device) if scales is None else scales
    return outs


def _check_embed_layers(layers, rows, who):
    """[(ids [B, L], d [B, L, dim] | [B, dim], num_embeddings, weight)] with detached tensors."""
    out = []
    for ids, d, V, weight in layers:
        ids, d = lib.as_tensor(ids).detach(), lib.as_tensor(d).detach()
        if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
            raise errors.InvalidArgumentError(f"{who}: ids must have an integer dtype, got {ids.dtype}")
        out.append((ids[:, None] if ids.dim() == 1 else ids, d, int(V), float(weight)))
    dev, B = out[0][1].device, out[0][1].shape[0] if out[0][1].dim() else 0
    for ids, d, V, _ in out:
        if d.dtype != torch.float32:
            raise errors.InvalidArgumentError(f"{who}: d must be float32, got {d.dtype}")
        if ids.device != dev or d.device != dev or dev.type != "cuda":
            raise errors.InvalidArgumentError(f"{who}: every ids and d lies on one ROCm device")
        if (ids.dim() != 2 or d.dim() not in (2, 3) or ids.shape[0] != B or d.shape[0] != B or 0 in ids.shape
                or 0 in d.shape or (d.dim() == 3 and d.shape[1] != ids.shape[1]) or V < 1):
            raise errors.InvalidArgumentError(
                f"{who}: a table takes ids [B, L] and d [B, L, dim] (an embedding) or [B, dim] (a bag) with B = {B} "
                f"and at least one row, got {tuple(ids.shape)}, {tuple(d.shape)} and {V} rows")
        if ids.numel() > MAX_EMBEDDING_ENTRIES:
            raise errors.InvalidArgumentError(
                f"{who}: {ids.numel()} ids looked up in one table, more than {MAX_EMBEDDING_ENTRIES} entries per layer")
    rows = int(rows)
    if rows < 1 or B % rows:
        raise errors.InvalidArgumentError(f"{who}: {rows} microbatches do not divide the batch of {B}")
    if B // rows > MAX_ROWS_PER_MICROBATCH:
        raise errors.InvalidArgumentError(f"{who}: {B // rows} examples per microbatch, at most "
                                          f"{MAX_ROWS_PER_MICROBATCH} (r > {MAX_ROWS_PER_MICROBATCH})")
    return out, rows


def _embed_table(layers, ctrs):
    """The DpEmbed table of checked embedding layers with freshly carved outputs: (table, [table_grad],
    tensors to keep alive)."""
    dev = layers[0][1].device
    outs = lib._carve([torch.empty(V, d.shape[-1], device="meta") for _, d, V, _ in layers], torch.float32, dev)
    arr, keep = (lib.DpEmbed * len(layers))(), []
    for rec, (ids, d, V, weight), ctr0, out in zip(arr, layers, ctrs, outs):
        ids, d = ids.to(torch.int64).contiguous(), d.contiguous()
        keep += [ids, d]
        L, dim = ids.shape[1], d.shape[-1]
        rec.ids, rec.d, rec.out, rec.V, rec.dim, rec.L, rec.w, rec.ctr0 = ids.data_ptr(), d.data_ptr(), out.data_ptr(), V, dim, L, weight, ctr0
        rec.d_row_stride, rec.d_l_stride = (L * dim, dim) if d.dim() == 3 else (dim, 0)
    return arr, outs, keep


def _embed_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, scales, table=None):
    """efl_dp_embed_clip_sum over checked layers; ctrs: per table its first Philox block; table: their
    _embed_table when the caller has made it. Returns ([table_grad], scales | None)."""
    dev, B, raw = layers[0][1].device, layers[0][1].shape[0], lib.raw()
    arr, outs, keep = table or _embed_table(layers, ctrs)
    clip_mode = 2 if scales is not None else 0 if l2_norm_clip is None else 1
    work, work_elems = None, 0
    if clip_mode == 2:
        scales = lib.as_tensor(scales).detach().to(dev, torch.float32).contiguous()
        if scales.shape != (rows,):
            raise errors.InvalidArgumentError(f"dp_embed_clip_sum_noise: scales must be [{rows}]")
    elif clip_mode == 1:
        work_elems = _elems(raw.efl_dp_embed_work_elems(len(layers), rows))
        work = torch.empty(max(work_elems, 1), dtype=torch.float64, device=dev)
        scales = torch.empty(rows, dtype=torch.float32, device=dev)
    nbytes = _elems(raw.efl_dp_embed_scratch_bytes(arr, len(layers), B))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    lib.check(raw.efl_dp_embed_clip_sum(arr, len(layers), B, rows, clip_mode, float(l2_norm_clip or 0.0), int(mode),
                                        float(sigma), float(divisor), seed,
                                        None if scales is None else scales.data_ptr(),
                                        None if work is None else work.data_ptr(), work_elems, scratch.data_ptr(),
                                        nbytes, lib.stream_handle(dev)))
    return outs, scales


@exporter.export("privacy.dp_embed_clip_sum_noise")
def dp_embed_clip_sum_noise(layers, rows: int, l2_norm_clip, mode: int, sigma: float, divisor: float = 1.0,
                            stream: NoiseStream | None = None, scales=None, return_scales: bool = False):
    """efl_dp_embed_clip_sum: a DP-SGD step's clipped, summed, noised and divided gradients of embedding
    tables from the looked-up ids and the output gradients, without a dense gradient per microbatch.
    `layers` is a list of (ids [B, L] or [B], d, num_embeddings, weight): ids of an integer dtype, d the
    float32 gradient of the SUM of the per-example losses by the layer's output, [B, L, dim] for a
    torch.nn.Embedding and [B, dim] for a torch.nn.EmbeddingBag (which decides the kind), weight the factor
    of every entry (1; 1 / L for a bag of mode "mean"). At most 8,192 ids per table; an id outside
    [0, num_embeddings) hits no row. Microbatch i is the B / rows (at most 16) consecutive examples from
    i * B / rows. Returns [table_grad [num_embeddings, dim], ...]; mode, sigma, divisor, scales,
    return_scales and the stream positions (one take(numel) per table, in layer order) are
    dp_dense_clip_sum_noise's. A row no id names is the noise of zero."""
    layers = list(layers)
    if not layers:
        return ([], None) if return_scales else []
    layers, rows = _check_embed_layers(layers, rows, "dp_embed_clip_sum_noise")
    st = stream or _stream
    takes = [st.take(V * d.shape[-1]) for _, d, V, _ in layers]
    outs, scales = _embed_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, takes[0][0], [t[1] for t in takes], scales)
    if return_scales:
        return outs, torch.ones(rows, device=layers[0][1].device) if scales is None else scales
    return outs


def _check_norm_layers(layers, rows, who):
    """[(x, d, has_bias, groups | None, eps)] with detached tensors: a LayerNorm over the last dimension
    (groups None) gives x and d [B, *, C], flattened to [B, T, C]; a GroupNorm of `groups` groups gives
    [B, C, *], flattened to [B, C, L]."""
    out = []
    for x, d, has_bias, groups, eps in layers:
        out.append((lib.as_tensor(x).detach(), lib.as_tensor(d).detach(), bool(has_bias),
                    None if groups is None else int(groups), float(eps)))
    dev, B = out[0][0].device, out[0][0].shape[0] if out[0][0].dim() else 0
    for k, (x, d, has_bias, groups, eps) in enumerate(out):
        if x.dtype != torch.float32 or d.dtype != torch.float32:
            raise errors.InvalidArgumentError(f"{who}: x and d must be float32, got {x.dtype} and {d.dtype}")
        if x.device != dev or d.device != dev or dev.type != "cuda":
            raise errors.InvalidArgumentError(f"{who}: every x and d lies on one ROCm device")
        if x.dim() < 2 or x.shape != d.shape or x.shape[0] != B or 0 in x.shape:
            raise errors.InvalidArgumentError(
                f"{who}: a norm layer takes x and d of one shape, [B, *, C] (LayerNorm) or [B, C, *] (GroupNorm) with "
                f"B = {B}, got {tuple(x.shape)} and {tuple(d.shape)}")
        shape = (B, -1, x.shape[-1]) if groups is None else (B, x.shape[1], -1)
        out[k] = (x.reshape(shape), d.reshape(shape), has_bias, groups, eps)
    rows = int(rows)
    if rows < 1 or B % rows:
        raise errors.InvalidArgumentError(f"{who}: {rows} microbatches do not divide the batch of {B}")
    if B // rows > MAX_ROWS_PER_MICROBATCH:
        raise errors.InvalidArgumentError(f"{who}: {B // rows} examples per microbatch, at most "
                                          f"{MAX_ROWS_PER_MICROBATCH} (r > {MAX_ROWS_PER_MICROBATCH})")
    return out, rows


def _norm_table(layers, ctrs, rows):
    """The DpNorm table of checked norm layers with freshly carved outputs and the call's scratch: (table,
    [(w_grad, b_grad | None)], tensors to keep alive, scratch, its bytes). A channel-last tensor whose
    positions are contiguous rows at least C apart is taken as it lies (a padded row stride included)."""
    dev, B, like = layers[0][0].device, layers[0][0].shape[0], []
    for x, _, has_bias, groups, _ in layers:
        like += [torch.empty(x.shape[2 if groups is None else 1], device="meta")] * (2 if has_bias else 1)
    flat = iter(lib._carve(like, torch.float32, dev))
    arr, outs, keep = (lib.DpNorm * len(layers))(), [], []

    def rows_of(t):     # the flattened [B T, C] rows and their stride
        _, T, width = t.shape
        s = t.stride(1) if T > 1 else t.stride(0) if B > 1 else width
        if t.stride(2) != 1 or s < width or (B > 1 and T > 1 and t.stride(0) != T * s) or t.data_ptr() % 4:
            t, s = t.contiguous(), width
        return t, s

    for rec, (x, d, has_bias, groups, eps), (cw, cb) in zip(arr, layers, ctrs):
        if groups is None:
            (x, rec.x_row_stride), (d, rec.d_row_stride) = rows_of(x), rows_of(d)
            rec.kind, rec.groups, rec.T_or_L, rec.C = 0, 1, x.shape[1], x.shape[2]
        else:
            x, d = x.contiguous(), d.contiguous()
            rec.kind, rec.groups, rec.T_or_L, rec.C = 1, groups, x.shape[2], x.shape[1]
        keep += [x, d]
        w, b = next(flat), next(flat) if has_bias else None
        rec.x, rec.d, rec.w_out, rec.b_out, rec.eps = x.data_ptr(), d.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), eps
        rec.ctr0_w, rec.ctr0_b = cw, cb
        outs.append((w, b))
    nbytes = _elems(lib.raw().efl_dp_norm_scratch_bytes(arr, len(layers), B, rows))
    return arr, outs, keep, torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev), nbytes


def _norm_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, scales, table=None):
    """efl_dp_norm_clip_sum over checked norm layers; ctrs: per layer the first Philox block of (weight,
    bias); table: their _norm_table when the caller has made it. Returns ([(w_grad, b_grad | None)],
    scales | None)."""
    dev, B, raw = layers[0][0].device, layers[0][0].shape[0], lib.raw()
    arr, outs, keep, scratch, nbytes = table or _norm_table(layers, ctrs, rows)
    clip_mode = 2 if scales is not None else 0 if l2_norm_clip is None else 1
    work, work_elems = None, 0
    if clip_mode == 2:
        scales = lib.as_tensor(scales).detach().to(dev, torch.float32).contiguous()
        if scales.shape != (rows,):
            raise errors.InvalidArgumentError(f"dp_norm_clip_sum_noise: scales must be [{rows}]")
    elif clip_mode == 1:
        work_elems = _elems(raw.efl_dp_norm_work_elems(arr, len(layers), B, rows))
        work = torch.empty(max(work_elems, 1), dtype=torch.float64, device=dev)
        scales = torch.empty(rows, dtype=torch.float32, device=dev)
    lib.check(raw.efl_dp_norm_clip_sum(arr, len(layers), B, rows, clip_mode, float(l2_norm_clip or 0.0), int(mode),
                                       float(sigma), float(divisor), seed,
                                       None if scales is None else scales.data_ptr(),
                                       None if work is None else work.data_ptr(), work_elems, scratch.data_ptr(),
                                       nbytes, lib.stream_handle(dev)))
    return outs, scales


def _norm_numels(layers):
    return [(x.shape[2 if groups is None else 1],) * 2 if has_bias else (x.shape[2 if groups is None else 1], 0)
            for x, _, has_bias, groups, _ in layers]


@exporter.export("privacy.dp_norm_clip_sum_noise")
def dp_norm_clip_sum_noise(layers, rows: int, l2_norm_clip, mode: int, sigma: float, divisor: float = 1.0,
                           stream: NoiseStream | None = None, scales=None, return_scales: bool = False):
    """efl_dp_norm_clip_sum: a DP-SGD step's clipped, summed, noised and divided gradients of the scale
    (weight) and bias of per-example normalisation layers from their inputs and output gradients. `layers`
    is a list of (x, d, has_bias, groups, eps): float32 ROCm tensors of one shape, d the gradient of the SUM
    of the per-example losses by the layer's output. groups None is a torch.nn.LayerNorm over the last
    dimension (x [B, *, C], statistics per row); an int G a torch.nn.GroupNorm of G groups (x [B, C, *],
    statistics per example and group). Microbatch i is the B / rows (at most 16) consecutive examples from
    i * B / rows. Returns [(w_grad [C], b_grad [C] | None)]: noise(sum_i scale_i sum d xh) / divisor and
    noise(sum_i scale_i sum d) / divisor, xh = (x - mean) / sqrt(var + eps) with the statistics in double;
    mode, sigma, divisor, scales, return_scales and the stream positions (one take(numel) per variable,
    weight then bias, in layer order) are dp_dense_clip_sum_noise's."""
    layers = list(layers)
    if not layers:
        return ([], None) if return_scales else []
    layers, rows = _check_norm_layers(layers, rows, "dp_norm_clip_sum_noise")
    seed, ctrs = _take_layers(_norm_numels(layers), stream or _stream)
    outs, scales = _norm_clip_sum(layers, rows, l2_norm_clip, mode, sigma, divisor, seed, ctrs, scales)
    if return_scales:
        return outs, torch.ones(rows, device=layers[0][0].device) if scales is None else scales
    return outs


def _factored_clip_sum(dense, conv, rows, l2_norm_clip, mode, sigma, divisor, seed, dctrs, cctrs, scales,
                       embed=(), ectrs=(), norm=(), nctrs=()):
    """Checked dense, conv, embedding and norm layers under ONE norm: (dense outs, conv outs, embedding outs,
    norm outs, scales | None). With more than one family and no given scales, all write their norm slots into
    one work buffer [rows, slots] (dense, then conv, then embedding, then norm), efl_dp_scales makes the
    scales, and every sum runs with them (clip_mode 2). The dense layers over sequences (x [B, T, in]) are a
    family of their own (csrc/dpseq.hip), their slots after the 2-D dense layers'; their outputs come back in
    `dense`'s order."""
    seq_at = [k for k, (x, _, _) in enumerate(dense) if x.dim() == 3]
    seq, sctrs = [dense[k] for k in seq_at], [dctrs[k] for k in seq_at]
    dense_at = [k for k in range(len(dense)) if k not in seq_at]
    dense, dctrs = [dense[k] for k in dense_at], [dctrs[k] for k in dense_at]
    dtab = stab = ctab = etab = ntab = None
    if (bool(dense) + bool(seq) + bool(conv) + bool(embed) + bool(norm)) > 1 and scales is None and l2_norm_clip is not None:
        first = dense[0][0] if dense else seq[0][0] if seq else conv[0][0] if conv else norm[0][0]
        dev, B, raw, h = first.device, first.shape[0], lib.raw(), lib.stream_handle(first.device)
        dtab, ctab, etab = dense and _dense_table(dense, dctrs), conv and _conv_table(conv, cctrs), embed and _embed_table(embed, ectrs)
        stab, ntab = seq and _seq_table(seq, sctrs), norm and _norm_table(norm, nctrs, rows)
        ns = _elems(raw.efl_dp_seq_work_elems(stab[0], len(seq), B, rows)) // rows if seq else 0
        nc = _elems(raw.efl_dp_conv_work_elems(ctab[0], len(conv), rows)) // rows if conv else 0
        nn = _elems(raw.efl_dp_norm_work_elems(ntab[0], len(norm), B, rows)) // rows if norm else 0
        slots = len(dense) + ns + nc + len(embed) + nn
        work = torch.empty(rows * slots, dtype=torch.float64, device=dev)
        scales = torch.empty(rows, dtype=torch.float32, device=dev)
        if dense:
            lib.check(raw.efl_dp_dense_sqnorm(dtab[0], len(dense), B, rows, work.data_ptr(), 0, slots, h))
        if seq:
            lib.check(raw.efl_dp_seq_sqnorm(stab[0], len(seq), B, rows, work.data_ptr(), len(dense), slots, h))
        if conv:
            lib.check(raw.efl_dp_conv_sqnorm(ctab[0], len(conv), B, rows, work.data_ptr(), len(dense) + ns, slots, h))
        if embed:
            lib.check(raw.efl_dp_embed_sqnorm(etab[0], len(embed), B, rows, work.data_ptr(), len(dense) + ns + nc, slots, h))
        if norm:
            lib.check(raw.efl_dp_norm_sqnorm(ntab[0], len(norm), B, rows, work.data_ptr(), slots - nn, slots,
                                             ntab[3].data_ptr(), ntab[4], h))
        lib.check(raw.efl_dp_scales(work.data_ptr(), slots, rows, float(l2_norm_clip), scales.data_ptr(), h))
    douts = couts = eouts = nouts = []
    if dense:                               # one family alone takes its own norm pass (clip_mode 1)
        douts, scales = _dense_clip_sum(dense, rows, l2_norm_clip, mode, sigma, divisor, seed, dctrs, scales, dtab or None)
    if seq:
        souts, scales = _seq_clip_sum(seq, rows, l2_norm_clip, mode, sigma, divisor, seed, sctrs, scales, stab or None)
        merged = [None] * (len(dense_at) + len(seq_at))
        for k, o in zip(dense_at + seq_at, [*douts, *souts]):
            merged[k] = o
        douts = merged
    if conv:
        couts, scales = _conv_clip_sum(conv, rows, l2_norm_clip, mode, sigma, divisor, seed, cctrs, scales, ctab or None)
    if embed:
        eouts, scales = _embed_clip_sum(embed, rows, l2_norm_clip, mode, sigma, divisor, seed, ectrs, scales, etab or None)
    if norm:
        nouts, scales = _norm_clip_sum(norm, rows, l2_norm_clip, mode, sigma, divisor, seed, nctrs, scales, ntab or None)
    return douts, couts, eouts, nouts, scales


@exporter.export("privacy.dp_factored_clip_sum_noise")
def dp_factored_clip_sum_noise(dense_layers, conv_layers, rows: int, l2_norm_clip, mode: int, sigma: float,
                               divisor: float = 1.0, stream: NoiseStream | None = None, scales=None,
                               return_scales: bool = False, *, embedding_layers=None, norm_layers=None):
    """dp_dense_clip_sum_noise, dp_conv_clip_sum_noise, dp_embed_clip_sum_noise and dp_norm_clip_sum_noise
    over one model's layers under ONE shared clip norm: scale_i = clip * min(1 / ||g_i||, 1 / clip) with g_i
    microbatch i's gradient of ALL the layers' variables. `dense_layers`, `conv_layers`, `embedding_layers`
    and `norm_layers` (the last two keyword only) are those functions' lists (any may be empty); the dense
    variables come first in the stream, then the conv ones, then the tables, then the norm layers'. Returns
    (dense_outs, conv_outs), with `embedding_layers` given embedding_outs after them, with `norm_layers`
    given norm_outs after those, and the scales last with return_scales."""
    dense, conv, embed, norm = list(dense_layers), list(conv_layers), list(embedding_layers or ()), list(norm_layers or ())
    who = "dp_factored_clip_sum_noise"
    tail = (() if embedding_layers is None else ([],)) + (() if norm_layers is None else ([],))
    if not dense and not conv and not embed and not norm:
        return ([], [], *tail, None) if return_scales else ([], [], *tail)
    if dense:
        dense, rows = _check_dense_layers(dense, rows, who)
    if conv:
        conv, rows = _check_conv_layers(conv, rows, who)
    if embed:
        embed, rows = _check_embed_layers(embed, rows, who)
    if norm:
        norm, rows = _check_norm_layers(norm, rows, who)
    firsts = [f[0][0] for f in (dense, conv, embed, norm) if f]
    if any(t.shape[0] != firsts[0].shape[0] or t.device != firsts[0].device for t in firsts):
        raise errors.InvalidArgumentError(f"{who}: the dense, conv, embedding and norm layers take one batch on one device")
    st = stream or _stream
    seed, dctrs = _take_layers([(d.shape[-1] * x.shape[-1], d.shape[-1] if b else 0) for x, d, b in dense], st)
    seed_c, cctrs = _take_layers(_conv_numels(conv), st)
    seed_e, ectrs = _take_layers([(V * d.shape[-1], 0) for _, d, V, _ in embed], st)
    seed_n, nctrs = _take_layers(_norm_numels(norm), st)
    seed = next(v for v in (seed, seed_c, seed_e, seed_n) if v is not None)
    douts, couts, eouts, nouts, scales = _factored_clip_sum(dense, conv, rows, l2_norm_clip, mode, sigma, divisor, seed,
                                                            dctrs, cctrs, scales, embed, [c for c, _ in ectrs], norm, nctrs)
    outs = (douts, couts, *(() if embedding_layers is None else (eouts,)), *(() if norm_layers is None else (nouts,)))
    if return_scales:
        return (*outs, torch.ones(rows, device=firsts[0].device) if scales is None else scales)
    return outs


def _fusable(query, cls, stacked):
    """efl_dp_clip_sum does exactly the stock query's clip, sum and noise: only an instance of the
    stock class itself over a float32 device stack takes it. A subclass (its own clip, noise, ledger
    or state) keeps the restated loop, so what it overrides is honoured as under "loop"."""
    return type(query) is cls and bool(stacked) and all(t.dtype == torch.float32 and t.is_cuda and t.dim() >= 1 and t.shape[0] > 0
                                 for t in stacked)


def _zeros_like(t):
    return torch.zeros_like(t)


class _SumQuery:
    """DPQuery protocol (tensorflow_privacy dp_query.SumAggregationDPQuery) on lists of tensors."""

    def initial_global_state(self):
        return None

    def derive_sample_params(self, global_state):
        return None

    def initial_sample_state(self, template):
        return [_zeros_like(t) for t in template]

    def preprocess_record(self, params, record):
        return record

    def accumulate_record(self, params, sample_state, record):
        rec = self.preprocess_record(params, record)
        return [s + r for s, r in zip(sample_state, rec)]

    def accumulate_batch(self, params, stacked):
        """The sample state of a record whose microbatch gradients lie stacked as [rows, ...] per
        variable: accumulate_record row by row, the loop restated over the stack."""
        state = self.initial_sample_state([t[0] for t in stacked])
        for i in range(stacked[0].shape[0]):
            state = self.accumulate_record(params, state, [t[i] for t in stacked])
        return state

    def get_noised_result(self, sample_state, global_state, divisor: float = 1.0):
        raise NotImplementedError

    def get_noised_batch(self, params, stacked, global_state, divisor: float = 1.0):
        """get_noised_result of accumulate_batch; the Gaussian queries fuse the two into
        efl_dp_clip_sum for float32 device stacks."""
        return self.get_noised_result(self.accumulate_batch(params, stacked), global_state, divisor)


@exporter.export("privacy.GaussianSumQuery")
class GaussianSumQuery(_SumQuery):
    """Clip each record to l2_norm_clip (global norm over its tensors), sum, add N(0, stddev^2)
    (dp_optimizer.py:54-57; tensorflow_privacy 0.3.0 gaussian_query.GaussianSumQuery)."""

    def __init__(self, l2_norm_clip: float, stddev: float):
        self._l2_norm_clip = float(l2_norm_clip)
        self._stddev = float(stddev)

    def derive_sample_params(self, global_state):
        return self._l2_norm_clip

    def preprocess_record(self, params, record):
        # tf.clip_by_global_norm: t * clip * min(1 / ||record||, 1 / clip), in the record's dtype
        # (the widest of its tensors)
        dt = torch.float64 if any(t.dtype == torch.float64 for t in record) else torch.float32
        norm = torch.sqrt(sum((t.to(dt) * t.to(dt)).sum() for t in record))
        scale = params * torch.minimum(1.0 / norm, torch.tensor(1.0 / params, dtype=dt, device=norm.device))
        return [t * scale.to(t.dtype) for t in record]

    def get_noised_result(self, sample_state, global_state, divisor: float = 1.0):
        return [dp_noise(v, 1, self._stddev, divisor) for v in sample_state], global_state

    def get_noised_batch(self, params, stacked, global_state, divisor: float = 1.0):
        if not _fusable(self, GaussianSumQuery, stacked):
            return super().get_noised_batch(params, stacked, global_state, divisor)
        return dp_clip_sum_noise(stacked, params, 1, self._stddev, divisor), global_state


@exporter.export("privacy.ElementWiseGaussianSumQuery")
class ElementWiseGaussianSumQuery(_SumQuery):
    """Sum, then v + normal(shape(v)) * v * noise_multiplier (dp_optimizer.py:60-73)."""

    def __init__(self, noise_multiplier: float = 1):
        self._noise_multiplier = float(noise_multiplier)

    def get_noised_result(self, sample_state, global_state, divisor: float = 1.0):
        return [dp_noise(v, 0, self._noise_multiplier, divisor) for v in sample_state], global_state

    def get_noised_batch(self, params, stacked, global_state, divisor: float = 1.0):
        if not _fusable(self, ElementWiseGaussianSumQuery, stacked):
            return super().get_noised_batch(params, stacked, global_state, divisor)
        return dp_clip_sum_noise(stacked, None, 0, self._noise_multiplier, divisor), global_state


_DEFAULT_OPT_CONFIG = {"REDUCE": "mean"}


def _split_params(args, kwargs):
    """The torch optimiser's params if the caller gave them (first positional or `params=`)."""
    if "params" in kwargs:
        return kwargs.pop("params"), args
    if args and not isinstance(args[0], (int, float)):
        return args[0], args[1:]
    return None, args


def _bind(args, kwargs, *spec):
    """Bind the leading (name, default) parameters from positional args, then keywords; returns
    their values followed by the remaining positional args."""
    args = list(args)
    vals = []
    for name, default in spec:
        if args:
            if name in kwargs:
                raise TypeError(f"got multiple values for argument {name!r}")
            vals.append(args.pop(0))
        else:
            vals.append(kwargs.pop(name, default))
    return (*vals, tuple(args))


def _as_params(obj):
    """obj as a torch optimiser's params (a list of tensors or param-group dicts), or None when it
    is something else (a number, a query): lets `DPAdamGaussianOptimizer(model.parameters(), lr=..)`
    work although the reference's first positional argument is noise_multiplier."""
    if obj is None or isinstance(obj, (int, float, bool, str)) or hasattr(obj, "get_noised_result"):
        return None
    if isinstance(obj, torch.Tensor):
        return [obj]
    try:
        items = list(obj)
    except TypeError:
        return None
    if items and all(isinstance(t, (torch.Tensor, dict)) for t in items):
        return items
    return None


@exporter.export("privacy.make_optimizer_class")
def make_optimizer_class(cls):
    """A DP subclass of the torch optimiser class `cls` (dp_optimizer.py:80-220)."""

    class DPOptimizerClass(cls):
        def __init__(self, *args, **kwargs):
            """(dp_sum_query, num_microbatches=None, unroll_microbatches=False, [params], **opt
            kwargs), or torch style (params, dp_sum_query=..., ...). microbatch_gradients= "loop" /
            "batched" / "factored" (keyword only; None: the process default, set_microbatch_gradients).
            dense_layers=, conv_layers= and embedding_layers= (keyword only): the torch.nn.Linear, the
            torch.nn.Conv2d and the torch.nn.Embedding / torch.nn.EmbeddingBag modules "factored" takes its
            gradients from; each gets a forward hook that keeps its input and output of the current step.
            norm_layers= (keyword only): the torch.nn.LayerNorm (elementwise_affine, a 1-D normalized_shape, with
            or without a bias) and torch.nn.GroupNorm (affine) modules, the same way."""
            self._microbatch_gradients = kwargs.pop("microbatch_gradients", None)
            _resolve_microbatch_gradients(self._microbatch_gradients)
            self._dense = {}                # Linear module -> [(detached input, output)] since the last step
            for layer in kwargs.pop("dense_layers", None) or ():
                if not isinstance(layer, torch.nn.Linear):
                    raise errors.InvalidArgumentError(f"dense_layers takes torch.nn.Linear modules, got {type(layer).__name__}")
                self._dense[layer] = []
                layer.register_forward_hook(self._keep_dense)
            self._conv = {}                 # Conv2d module -> the same
            for layer in kwargs.pop("conv_layers", None) or ():
                if not isinstance(layer, torch.nn.Conv2d):
                    raise errors.InvalidArgumentError(
                        f"conv_layers takes torch.nn.Conv2d modules (no transposed, 1-d or 3-d convolutions), got "
                        f"{type(layer).__name__}")
                if layer.groups != 1 or layer.padding_mode != "zeros":
                    raise errors.InvalidArgumentError(
                        f"conv_layers takes convolutions with groups = 1 and padding_mode 'zeros', got groups = "
                        f"{layer.groups} and padding_mode {layer.padding_mode!r}")
                _conv_padding(layer.padding, layer.kernel_size, layer.dilation, "conv_layers")
                self._conv[layer] = []
                layer.register_forward_hook(self._keep_dense)
            self._embed = {}                # Embedding / EmbeddingBag module -> [(ids, output, plain call)]
            for layer in kwargs.pop("embedding_layers", None) or ():
                if not isinstance(layer, (torch.nn.Embedding, torch.nn.EmbeddingBag)):
                    raise errors.InvalidArgumentError(
                        f"embedding_layers takes torch.nn.Embedding and torch.nn.EmbeddingBag modules, got "
                        f"{type(layer).__name__}")
                for name, plain in (("padding_idx", None), ("max_norm", None), ("scale_grad_by_freq", False), ("sparse", False)):
                    if getattr(layer, name) is not plain and getattr(layer, name) != plain:
                        raise errors.InvalidArgumentError(
                            f"embedding_layers takes tables without {name}, got {name}={getattr(layer, name)!r}")
                if getattr(layer, "mode", "sum") not in ("sum", "mean"):
                    raise errors.InvalidArgumentError(
                        f'embedding_layers takes bags of mode "sum" or "mean", got mode {layer.mode!r} (a max has no '
                        f"weighted sum of rows)")
                self._embed[layer] = []
                layer.register_forward_hook(self._keep_embed, with_kwargs=True)
            self._norm = {}                 # LayerNorm / GroupNorm module -> [(detached input, output)]
            for layer in kwargs.pop("norm_layers", None) or ():
                if not isinstance(layer, (torch.nn.LayerNorm, torch.nn.GroupNorm)):
                    raise errors.InvalidArgumentError(
                        f"norm_layers takes torch.nn.LayerNorm and torch.nn.GroupNorm modules (per-example statistics), "
                        f"got {type(layer).__name__}")
                if getattr(layer, "weight", None) is None:
                    raise errors.InvalidArgumentError(f"norm_layers takes layers with affine parameters, got {layer}")
                if isinstance(layer, torch.nn.LayerNorm) and len(layer.normalized_shape) != 1:
                    raise errors.InvalidArgumentError(
                        f"norm_layers takes a LayerNorm over the last dimension alone, got normalized_shape "
                        f"{tuple(layer.normalized_shape)}")
                self._norm[layer] = []
                layer.register_forward_hook(self._keep_dense)
            if "learning_rate" in kwargs:
                kwargs["lr"] = kwargs.pop("learning_rate")
            lead = _as_params(args[0]) if args else None
            if lead is not None:    # params first, torch style: the DP arguments are keywords then
                if "dp_sum_query" not in kwargs:
                    raise TypeError("params given first: pass dp_sum_query= as a keyword")
                kwargs["params"] = lead
                args = args[1:]
            dp_sum_query, num_microbatches, unroll_microbatches, args = _bind(
                args, kwargs, ("dp_sum_query", None), ("num_microbatches", None), ("unroll_microbatches", False))
            if dp_sum_query is None:
                raise TypeError("dp_sum_query is required")
            params, args = _split_params(args, kwargs)
            self._dp_sum_query = dp_sum_query
            self._num_microbatches = num_microbatches
            self._global_state = dp_sum_query.initial_global_state()
            self._unroll_microbatches = unroll_microbatches   # kept for the signature: see microbatch_gradients
            self._was_compute_gradients_called = False
            self._opt_args, self._opt_kwargs = args, kwargs
            self._built = False
            if params is not None:
                self._build(params)

        def _build(self, params):
            cls.__init__(self, params, *self._opt_args, **self._opt_kwargs)
            self._built = True

        def compute_gradients(self, loss, var_list=None, grad_loss=None, opt_config=None):
            """[(gradient, variable)] for a per-example loss tensor (first dim = batch)."""
            self._was_compute_gradients_called = True
            if callable(loss):
                raise NotImplementedError("Eager mode is not available yet")
            if var_list is None:
                if not self._built:
                    raise errors.InvalidArgumentError("var_list is required before the optimiser has params")
                var_list = [p for group in self.param_groups for p in group["params"]]
            var_list = list(var_list)
            if not self._built:
                self._build(var_list)
            opt_config = dict(_DEFAULT_OPT_CONFIG if opt_config is None else opt_config)
            reduce_func = opt_config.pop("REDUCE", "mean")
            if reduce_func not in ("mean", "sum") and not callable(reduce_func):
                raise ValueError("No such reduce function called '{}'.".format(str(reduce_func)))
            batch_size = int(loss.shape[0])
            nm = batch_size if self._num_microbatches is None else int(self._num_microbatches)
            if nm <= 0 or batch_size % nm != 0:
                nm = batch_size
            loss = loss.reshape(nm, -1)
            grad_loss = None if grad_loss is None else grad_loss.reshape(nm, -1)
            params = self._dp_sum_query.derive_sample_params(self._global_state)
            path = _resolve_microbatch_gradients(self._microbatch_gradients)
            if path == "factored":
                try:
                    return list(zip(self._factored_gradients(loss, var_list, grad_loss, reduce_func, params, nm,
                                                             batch_size), var_list))
                finally:                    # the kept inputs and outputs belong to this step alone
                    for seen in (*self._dense.values(), *self._conv.values(), *self._embed.values(), *self._norm.values()):
                        seen.clear()
            if path == "batched":
                stacked = self._stacked_gradients(loss, var_list, grad_loss, reduce_func)
                final, self._global_state = self._dp_sum_query.get_noised_batch(params, stacked, self._global_state,
                                                                                divisor=float(nm))
                return list(zip(final, var_list))
            state = self._dp_sum_query.initial_sample_state([v.detach() for v in var_list])
            for i in range(nm):
                row = loss[i]
                if callable(reduce_func):
                    row = reduce_func(loss[i:i + 1], 0)
                # a non-scalar row differentiates as its sum (TF's gradients of a tensor loss)
                go = torch.ones_like(row) if grad_loss is None else grad_loss[i].reshape(row.shape)
                grads = torch.autograd.grad(row, var_list, grad_outputs=go, retain_graph=True, allow_unused=True)
                grads = [g if g is not None else torch.zeros_like(v) for g, v in zip(grads, var_list)]
                state = self._dp_sum_query.accumulate_record(params, state, grads)
            final, self._global_state = self._dp_sum_query.get_noised_result(state, self._global_state,
                                                                             divisor=float(nm))
            return list(zip(final, var_list))

        @staticmethod
        def _stacked_gradients(loss, var_list, grad_loss, reduce_func):
            """Every microbatch's gradients from ONE backward: [nm, *v.shape] per variable, row i the
            gradient the loop takes of row i of the [nm, k] loss, up to the summation order of torch's
            batched backward kernels (equal bits for the linear model of the GPU test; a CPU
            convolution backward has given other last bits). An unused variable gives zeros."""
            nm = loss.shape[0]
            if callable(reduce_func):
                loss = torch.stack([reduce_func(loss[i:i + 1], 0) for i in range(nm)])
            go = torch.ones_like(loss) if grad_loss is None else grad_loss.reshape(loss.shape)
            # E[i] selects row i: zero but for row i, which carries that row's grad_outputs
            sel = torch.zeros((nm,) + tuple(loss.shape), dtype=loss.dtype, device=loss.device)
            idx = torch.arange(nm, device=loss.device)
            sel[idx, idx] = go
            try:
                grads = torch.autograd.grad(loss, var_list, grad_outputs=sel, retain_graph=True, allow_unused=True,
                                            is_grads_batched=True)
            except RuntimeError as e:
                raise RuntimeError(f'microbatch_gradients="batched": the backward failed under is_grads_batched '
                                   f'(an op without a batching rule does); microbatch_gradients="loop" takes '
                                   f'one backward per microbatch instead ({e})') from e
            return [g.detach() if g is not None else torch.zeros((nm,) + tuple(v.shape), dtype=v.dtype, device=v.device)
                    for g, v in zip(grads, var_list)]

        def _keep_dense(self, layer, inputs, output):
            # a forward pass outside autograd (an evaluation under no_grad) is not part of a step
            if (torch.is_grad_enabled() and output.requires_grad
                    and _resolve_microbatch_gradients(self._microbatch_gradients) == "factored"):
                kept = self._dense if layer in self._dense else self._conv if layer in self._conv else self._norm
                kept[layer].append((inputs[0].detach(), output))

        def _keep_embed(self, layer, inputs, kwargs, output):
            if (torch.is_grad_enabled() and output.requires_grad
                    and _resolve_microbatch_gradients(self._microbatch_gradients) == "factored"):
                rest = dict(kwargs)         # the ids come first or as input=; anything else set is refused later
                ids = inputs[0] if inputs else rest.pop("input")
                plain = all(a is None for a in (*inputs[1:], *rest.values()))
                self._embed[layer].append((ids.detach(), output, plain))

        def _factored_gradients(self, loss, var_list, grad_loss, reduce_func, params, nm, batch):
            """The step's gradients of the registered dense, conv, embedding and norm layers' variables from ONE
            ordinary backward to the layers' outputs, then efl_dp_dense_clip_sum (csrc/dpdense.hip),
            efl_dp_conv_clip_sum (csrc/dpconv.hip), efl_dp_embed_clip_sum (csrc/dpembed.hip) and
            efl_dp_norm_clip_sum (csrc/dpnorm.hip) under one shared norm. Precondition that cannot be
            checked here: the examples are independent in the forward pass (no batch statistics), so
            that row k of d(sum of the loss)/d(output) is example k's own."""
            who = 'microbatch_gradients="factored"'
            q = self._dp_sum_query
            if type(q) not in (GaussianSumQuery, ElementWiseGaussianSumQuery):
                raise errors.InvalidArgumentError(
                    f"{who}: only the stock GaussianSumQuery and ElementWiseGaussianSumQuery are fused, got "
                    f"{type(q).__name__} (a subclass's overrides need the per-microbatch gradients)")
            if callable(reduce_func):
                raise errors.InvalidArgumentError(f"{who}: a callable REDUCE needs the per-microbatch losses")
            owner = {}
            for layer in (*self._dense, *self._conv, *self._embed, *self._norm):
                owner[layer.weight] = (layer, 0)
                if getattr(layer, "bias", None) is not None:
                    owner[layer.bias] = (layer, 1)
            used = {}                           # layer -> [index of its weight in var_list, of its bias]
            for i, v in enumerate(var_list):
                if v not in owner:
                    raise errors.InvalidArgumentError(
                        f"{who}: variable {i} of var_list {tuple(v.shape)} is not the weight or bias of a layer "
                        f"given as dense_layers=, conv_layers=, embedding_layers= or norm_layers=")
                used.setdefault(owner[v][0], [None, None])[owner[v][1]] = i
            layers = []
            for layer, (wi, bi) in used.items():
                if wi is None:
                    raise errors.InvalidArgumentError(f"{who}: the bias of {layer} is in var_list without its weight")
                is_conv, is_norm = layer in self._conv, layer in self._norm
                seen = (self._embed if layer in self._embed else self._conv if is_conv else self._norm if is_norm
                        else self._dense)[layer]
                if len(seen) != 1:
                    raise errors.InvalidArgumentError(
                        f"{who}: {layer} ran {len(seen)} times since the last step; each layer runs once")
                x, out = seen[0][:2]
                if layer in self._embed:
                    bag = isinstance(layer, torch.nn.EmbeddingBag)
                    if not seen[0][2] or (bag and x.dim() != 2):
                        raise errors.InvalidArgumentError(
                            f"{who}: {layer} takes its ids alone, a bag as a 2-D [B, L] input: offsets (a 1-D input) "
                            f"and per_sample_weights are not supported")
                    if x.dim() not in (1, 2) or x.shape[0] != batch or out.dtype != torch.float32:
                        raise errors.InvalidArgumentError(
                            f"{who}: {layer} takes [B] or [B, L] ids with B = {batch} per-example losses and gives "
                            f"float32, got {tuple(x.shape)} and {out.dtype}")
                elif ((x.dim() != 4 if is_conv else x.dim() < 2) or x.shape[0] != batch or x.dtype != torch.float32
                        or out.dtype != torch.float32):
                    raise errors.InvalidArgumentError(
                        f"{who}: {layer} takes a float32 {'[B, Cin, H, W]' if is_conv else '[B, ...]' if is_norm else '[B, in] or [B, *, in]'} input with "
                        f"B = {batch} per-example losses, got {x.dtype} {tuple(x.shape)}")
                layers.append((layer, wi, bi, x, out))
            go = torch.ones_like(loss) if grad_loss is None else grad_loss.reshape(loss.shape)
            ds = torch.autograd.grad(loss, [l[4] for l in layers], grad_outputs=go, retain_graph=True, allow_unused=True)
            dense, conv, embed, norm = [], [], [], []     # (position in `layers`, record)
            for k, ((layer, _, bi, x, out), d) in enumerate(zip(layers, ds)):
                d = d if d is not None else torch.zeros_like(out)
                if layer in self._norm:
                    norm.append((k, (x, d, bi is not None, getattr(layer, "num_groups", None), layer.eps)))
                elif layer in self._embed:
                    mean = getattr(layer, "mode", "sum") == "mean"
                    embed.append((k, (x, d, layer.num_embeddings, 1.0 / x.shape[1] if mean else 1.0)))
                elif layer in self._conv:
                    conv.append((k, (x, d, bi is not None, layer.kernel_size, layer.stride, layer.padding, layer.dilation)))
                else:
                    dense.append((k, (x, d, bi is not None)))
            drecs, crecs, erecs, nrecs = ([r for _, r in f] for f in (dense, conv, embed, norm))
            if nrecs:
                nrecs, nm = _check_norm_layers(nrecs, nm, who)
            if erecs:
                erecs, nm = _check_embed_layers(erecs, nm, who)
            if drecs:
                drecs, nm = _check_dense_layers(drecs, nm, who)
            if crecs:
                crecs, nm = _check_conv_layers(crecs, nm, who)
            takes = [_stream.take(v.numel()) for v in var_list]          # as the loop: var_list order
            ctr = [(takes[wi][1], takes[bi][1] if bi is not None else 0) for _, wi, bi, _, _ in layers]
            clip, mode, sigma = (params, 1, q._stddev) if type(q) is GaussianSumQuery else (None, 0, q._noise_multiplier)
            douts, couts, eouts, nouts, _ = _factored_clip_sum(drecs, crecs, nm, clip, mode, sigma, float(nm), takes[0][0],
                                                               [ctr[k] for k, _ in dense], [ctr[k] for k, _ in conv], None,
                                                               erecs, [ctr[k][0] for k, _ in embed],
                                                               nrecs, [ctr[k] for k, _ in norm])
            final = [None] * len(var_list)
            for k, (w, b) in zip([k for k, _ in dense + conv + embed + norm],
                                 [*douts, *couts, *((t, None) for t in eouts), *nouts]):
                _, wi, bi, _, _ = layers[k]
                final[wi] = w
                if bi is not None:
                    final[bi] = b
            return final

        def apply_gradients(self, grads_and_vars):
            for g, v in grads_and_vars:
                v.grad = g.to(v.dtype)
            self.step()

        def minimize(self, loss, var_list=None, grad_loss=None, opt_config=None):
            self.apply_gradients(self.compute_gradients(loss, var_list, grad_loss, opt_config))

    DPOptimizerClass.__name__ = "DP" + cls.__name__
    return DPOptimizerClass


@exporter.export("privacy.make_gaussian_optimizer_class")
def make_gaussian_optimizer_class(cls):
    """A DP optimiser with Gaussian noise (dp_optimizer.py:224-256): element-wise noise scaled by
    each summed gradient without l2_norm_clip, clipped records + N(0, (clip * mult)^2) with it."""

    class DPGaussianOptimizerClass(make_optimizer_class(cls)):
        def __init__(self, *args, **kwargs):
            """(noise_multiplier=0, l2_norm_clip=None, num_microbatches=None,
            unroll_microbatches=False, [params], **opt kwargs), or torch style (params, ...)."""
            lead = _as_params(args[0]) if args else None
            if lead is not None:    # torch style: params first, the DP arguments as keywords
                kwargs["params"] = lead
                args = args[1:]
            noise_multiplier, l2_norm_clip, num_microbatches, unroll_microbatches, args = _bind(
                args, kwargs, ("noise_multiplier", 0), ("l2_norm_clip", None), ("num_microbatches", None),
                ("unroll_microbatches", False))
            if l2_norm_clip is None:
                q = ElementWiseGaussianSumQuery(noise_multiplier)
            else:
                q = GaussianSumQuery(l2_norm_clip, l2_norm_clip * noise_multiplier)
            super().__init__(q, num_microbatches, unroll_microbatches, *args, **kwargs)

        @property
        def ledger(self):
            return getattr(self._dp_sum_query, "ledger", None)

    DPGaussianOptimizerClass.__name__ = "DP" + cls.__name__ + "Gaussian"
    return DPGaussianOptimizerClass


# tf.train.{Adagrad, Adam, GradientDescent}Optimizer (dp_optimizer.py:258-260)
AdagradOptimizer = torch.optim.Adagrad
AdamOptimizer = torch.optim.Adam
GradientDescentOptimizer = torch.optim.SGD

DPAdagradOptimizer = exporter.export("privacy.DPAdagradOptimizer")(make_optimizer_class(AdagradOptimizer))
DPAdamOptimizer = exporter.export("privacy.DPAdamOptimizer")(make_optimizer_class(AdamOptimizer))
DPGradientDescentOptimizer = exporter.export("privacy.DPGradientDescentOptimizer")(
    make_optimizer_class(GradientDescentOptimizer))
DPAdagradGaussianOptimizer = exporter.export("privacy.DPAdagradGaussianOptimizer")(
    make_gaussian_optimizer_class(AdagradOptimizer))
DPAdamGaussianOptimizer = exporter.export("privacy.DPAdamGaussianOptimizer")(
    make_gaussian_optimizer_class(AdamOptimizer))
DPGradientDescentGaussianOptimizer = exporter.export("privacy.DPGradientDescentGaussianOptimizer")(
    make_gaussian_optimizer_class(GradientDescentOptimizer))
