"""CPU: efl_dp_dense_clip_sum (csrc/dpdense.hip) checks its layer table before any HIP call, and the
inputs of tests/test_dp_dense_gpu.py are ones on which the Gram identity the kernel computes,
||D_i^T X_i||_F^2 = sum_{a,b} (x_a . x_b)(d_a . d_b), agrees in float64 with the materialised
gradients the GPU test measures against, so that test's 1-ulp condition rests on the reference alone."""
import ctypes

import numpy as np
import pytest

CASES = [(6, 6), (6, 3), (6, 2), (130, 130), (64, 4)]     # (B, rows): r = 1, 2, 3, an odd K tail, r = 16
LAYERS = [(36, 33, True), (35, 5, True), (64, 32, False)]  # ragged tiles; in % 4 != 0; whole tiles, no bias


def zero_microbatch(rows):
    """The all-zero microbatch: the third, or the first where there are only two (one has to be
    clipped, and microbatch 0's scale is 1 either way)."""
    return 2 if rows > 2 else 0


def dense_case(B, rows):
    """[(x [B, in], d [B, out], has_bias)] float32: seeded normals, microbatch 0 scaled by 1e-3 in x
    and in d (unclipped), microbatch zero_microbatch(rows) all zero."""
    rng = np.random.default_rng(B * 1000 + rows)
    r, case, z = B // rows, [], zero_microbatch(rows)
    for nin, nout, bias in LAYERS:
        x, d = rng.standard_normal((B, nin)).astype(np.float32), rng.standard_normal((B, nout)).astype(np.float32)
        x[:r] *= np.float32(1e-3)
        d[:r] *= np.float32(1e-3)
        x[z * r:(z + 1) * r], d[z * r:(z + 1) * r] = 0, 0
        case.append((x, d, bias))
    return case


def materialised(case, rows):
    """Per layer the float64 G_i = D_i^T X_i [rows, out, in] and g_i = colsum(D_i) [rows, out] (None
    without a bias), and S [rows], the squared global norm of every microbatch's gradient."""
    grads, S = [], np.zeros(rows)
    for x, d, bias in case:
        xr, dr = (t.astype(np.float64).reshape(rows, -1, t.shape[1]) for t in (x, d))
        G = np.einsum("iao,ian->ion", dr, xr)
        g = dr.sum(axis=1) if bias else None
        S += (G ** 2).sum(axis=(1, 2)) + (0 if g is None else (g ** 2).sum(axis=1))
        grads.append((G, g))
    return grads, S


@pytest.mark.parametrize("B,rows", CASES)
def test_gram_identity_agrees_with_materialised_gradients(B, rows):
    case = dense_case(B, rows)
    S = materialised(case, rows)[1]
    gram = np.zeros(rows)
    for x, d, bias in case:
        xr, dr = (t.astype(np.float64).reshape(rows, -1, t.shape[1]) for t in (x, d))
        gram += (np.einsum("iak,ibk->iab", xr, xr) * np.einsum("iak,ibk->iab", dr, dr)).sum(axis=(1, 2))
        if bias:
            gram += (dr.sum(axis=1) ** 2).sum(axis=1)
    z = zero_microbatch(rows)
    assert S[z] == 0 and gram[z] == 0 and (np.delete(S, z) > 0).all()
    assert (np.abs(gram - S) <= 1e-12 * S).all()


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    p = ctypes.c_void_p(64)

    def call(x=64, xs=8, d=64, ds=4, w=64, b=64, nin=8, nout=4, nlayers=1, B=6, rows=3, clip_mode=1, clip=1.0, mode=1,
             div=2.0, scales=p, work=p, work_elems=3, table=True):
        arr = (efl.lib.DpDense * 1)()
        L = arr[0]
        L.x, L.x_row_stride, L.d, L.d_row_stride, L.w_out, L.b_out, L.in_, L.out = x, xs, d, ds, w, b, nin, nout
        return lib.efl_dp_dense_clip_sum(arr if table else None, nlayers, B, rows, clip_mode, clip, mode, 1.0, div, 7,
                                         scales, work, work_elems, None)

    bad = [dict(x=None), dict(d=None), dict(w=None), dict(table=False), dict(rows=4), dict(B=34, rows=2),
           dict(xs=7), dict(ds=3), dict(w=72), dict(work=None), dict(work_elems=2), dict(scales=None),
           dict(clip_mode=2, scales=None), dict(clip_mode=3), dict(mode=2), dict(div=0.0), dict(clip=0.0),
           dict(rows=0), dict(nlayers=-1), dict(nin=0)]
    for kw in bad:
        assert call(**kw) == -3, kw
        assert lib.efl_last_error().decode()
    assert call(nlayers=0, table=False) == 0                  # no layers: a no-op
    assert lib.efl_dp_dense_work_elems(3, 5) == 15
    assert lib.efl_dp_dense_work_elems(3, 0) == -3
