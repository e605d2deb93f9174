"""CPU: the float64 reference of tests/test_dp_conv_gpu.py (torch.nn.functional.unfold and an einsum that
materialise every microbatch's G_m [Cout, Cin kh kw] and g_m [Cout]; equal to autograd's per-example
conv weight gradient to 1e-10 on these shapes), its inputs, and efl_dp_conv_*'s argument checks, which
run before any HIP call (csrc/dpconv.hip)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_dp_dense_host import zero_microbatch

CASES = [(6, 6), (6, 2), (34, 34), (32, 2)]     # (B, rows): r = 1; r = 3; a ragged last split group; r = 16
# (Cin, Cout, kernel, stride, padding, dilation, (H, W), bias)
LAYERS = [(1, 16, (8, 8), (2, 2), (3, 3), (1, 1), (28, 28), True),    # dp_cnn's first layer, T = 196
          (3, 5, (3, 2), (2, 1), (1, 0), (1, 2), (9, 10), True),      # anisotropic; K = 18; ragged in q and o
          (32, 32, (1, 1), (1, 1), (0, 0), (1, 1), (4, 4), False),    # whole blocks, 1x1, no bias
          (5, 33, (3, 3), (1, 1), (1, 1), (1, 1), (7, 7), True),      # Cout crosses a block
          (1, 2, (3, 3), (1, 1), (0, 0), (1, 1), (40, 40), True)]     # T = 1,444: several rectangles


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


@functools.lru_cache(maxsize=None)
def conv_case(B, rows, layers=tuple(LAYERS)):
    """[(x [B, Cin, H, W], d [B, Cout, Ho, Wo], has_bias, kernel, stride, padding, dilation)] float32:
    seeded normals, microbatch 0 scaled by 1e-3 in x and in d (unclipped), microbatch
    zero_microbatch(rows) all zero."""
    rng = np.random.default_rng(B * 1000 + rows)
    r, case, z = B // rows, [], zero_microbatch(rows)
    for cin, cout, k, s, p, dil, hw, bias in layers:
        ho, wo = (out_size(hw[a], k[a], s[a], p[a], dil[a]) for a in (0, 1))
        x = rng.standard_normal((B, cin, *hw)).astype(np.float32)
        d = rng.standard_normal((B, cout, ho, wo)).astype(np.float32)
        for t in (x, d):
            t[:r] *= np.float32(1e-3)
            t[z * r:(z + 1) * r] = 0
        case.append((x, d, bias, k, s, p, dil))
    return case


def unfolded(x, d, k, s, p, dil, scale=None):
    """float64 U [B, K, T] and D [B, Cout, T] (times scale [B] when given)."""
    U = torch.nn.functional.unfold(torch.from_numpy(x).double(), k, dilation=dil, padding=p, stride=s).numpy()
    D = d.astype(np.float64).reshape(d.shape[0], d.shape[1], -1)
    return U, D if scale is None else D * scale[:, None, None]


@functools.lru_cache(maxsize=None)
def materialised(B, rows, layers=tuple(LAYERS)):
    """S [rows]: the squared global norm of every microbatch's gradient over conv_case(B, rows)."""
    S = np.zeros(rows)
    for x, d, bias, k, s, p, dil in conv_case(B, rows, layers):
        U, D = unfolded(x, d, k, s, p, dil)
        G = np.einsum("bot,bkt->bok", D, U).reshape(rows, B // rows, d.shape[1], -1).sum(axis=1)
        S += (G ** 2).sum(axis=(1, 2))
        if bias:
            S += (D.sum(axis=2).reshape(rows, B // rows, -1).sum(axis=1) ** 2).sum(axis=1)
    return S


@pytest.mark.parametrize("B,rows", CASES)
def test_inputs_clip_some_microbatches_and_not_others(B, rows):
    S, z = materialised(B, rows), zero_microbatch(rows)
    assert S[z] == 0 and (np.delete(S, z) > 0).all()
    assert (z == 0 or S[0] < 0.25) and S.max() > 9.0       # unclipped and clipped at both of the GPU test's clips


def test_reference_is_autograd_weight_gradient():
    x, d, _, k, s, p, dil = conv_case(6, 6)[1]
    w = torch.zeros(d.shape[1], x.shape[1], *k, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.from_numpy(x[1:2]).double(), w, None, s, p, dil)
    g, = torch.autograd.grad(y, w, torch.from_numpy(d[1:2]).double())
    U, D = unfolded(x[1:2], d[1:2], k, s, p, dil)
    assert np.abs(np.einsum("bot,bkt->ok", D, U) - g.numpy().reshape(d.shape[1], -1)).max() <= 1e-10


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    p = ctypes.c_void_p(64)

    def call(x=64, d=64, w=64, b=64, nlayers=1, B=6, rows=3, clip_mode=1, clip=1.0, mode=1, div=2.0, scales=p, work=p,
             work_elems=3, partials=p, partial_elems=180, table=True, **geom):
        arr = (efl.lib.DpConv * 1)()
        L = arr[0]
        L.x, L.d, L.w_out, L.b_out = x, d, w, b
        for name, v in dict(dict(cin=2, h=5, w=6, cout=3, ho=3, wo=2, kh=3, kw=3, sh=2, sw=2, ph=1, pw=0, dh=1, dw=1),
                            **geom).items():
            setattr(L, name, v)
        return lib.efl_dp_conv_clip_sum(arr if table else None, nlayers, B, rows, clip_mode, clip, mode, 1.0, div, 7,
                                        scales, work, work_elems, partials, partial_elems, None)

    bad = [dict(x=None), dict(d=None), dict(w=None), dict(w=72), dict(b=68), dict(table=False), dict(rows=4),
           dict(B=34, rows=2), dict(rows=0), dict(nlayers=-1), dict(cin=0), dict(sh=0), dict(dw=0), dict(ph=-1),
           dict(ho=2), dict(wo=3), dict(kh=8), dict(work=None), dict(work_elems=2), dict(partials=None),
           dict(partials=68), dict(partial_elems=179), dict(scales=None), dict(clip_mode=2, scales=None),
           dict(clip_mode=3), dict(mode=2), dict(div=0.0), dict(clip=0.0)]
    for kw in bad:
        assert call(**kw) == -3, kw
        assert lib.efl_last_error().decode()
    assert call(nlayers=0, table=False) == 0                  # no layers: a no-op
    arr = (efl.lib.DpConv * 1)()
    arr[0].x, arr[0].d, arr[0].w_out = 64, 64, 64
    arr[0].cin, arr[0].h, arr[0].w, arr[0].cout, arr[0].ho, arr[0].wo, arr[0].kh, arr[0].kw = 2, 5, 6, 3, 3, 2, 3, 3
    arr[0].sh, arr[0].sw, arr[0].ph, arr[0].pw, arr[0].dh, arr[0].dw = 2, 2, 1, 0, 1, 1
    # one 32x32 block per microbatch; 3 splits of pad4(3 * 18) weight sums (no bias here)
    assert lib.efl_dp_conv_work_elems(arr, 1, 3) == 3 and lib.efl_dp_conv_partial_elems(arr, 1, 6, 3) == 3 * 56
    arr[0].ho = 4
    assert lib.efl_dp_conv_work_elems(arr, 1, 3) == -3 and lib.efl_dp_conv_partial_elems(arr, 1, 6, 3) == -3
    assert lib.efl_dp_conv_sqnorm(arr, 0, 6, 4, p, 0, 1, None) == -3
    assert lib.efl_dp_scales(None, 1, 3, 1.0, p, None) == -3
    assert lib.efl_dp_dense_sqnorm(None, 1, 6, 3, p, 0, 1, None) == -3
