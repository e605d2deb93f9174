"""CPU: efl_dp_seq_clip_sum and efl_dp_seq_sqnorm (csrc/dpseq.hip) check their layer table and buffers
before any HIP call, and the two size functions give the hand-computed sizes."""
import ctypes

import pytest

P64 = ctypes.c_void_p(64)


def call(fn="clip_sum", x=64, xs=8, d=64, ds=4, w=64, b=64, T=5, nin=8, nout=4, nlayers=1, B=6, rows=3, clip_mode=1,
         clip=1.0, mode=1, div=2.0, scales=P64, work=P64, work_elems=3, partials=P64, partial_elems=108, table=True,
         slot0=0, slots=1):
    import efl
    lib = efl.lib.raw()
    arr = (efl.lib.DpSeq * 1)()
    L = arr[0]
    L.x, L.x_row_stride, L.d, L.d_row_stride, L.w_out, L.b_out, L.T, L.in_, L.out = x, xs, d, ds, w, b, T, nin, nout
    tab = arr if table else None
    if fn == "work":
        return lib.efl_dp_seq_work_elems(tab, nlayers, B, rows)
    if fn == "partial":
        return lib.efl_dp_seq_partial_elems(tab, nlayers, B, rows)
    if fn == "sqnorm":
        return lib.efl_dp_seq_sqnorm(tab, nlayers, B, rows, work, slot0, slots, None)
    return lib.efl_dp_seq_clip_sum(tab, nlayers, B, rows, clip_mode, clip, mode, 1.0, div, 7, scales, work, work_elems,
                                   partials, partial_elems, None)


@pytest.mark.parametrize("kw", [
    # what efl_dp_dense_clip_sum refuses
    dict(x=None), dict(d=None), dict(w=None), dict(table=False), dict(rows=4), dict(xs=7), dict(ds=3), dict(w=72),
    dict(x=66), dict(work=None), dict(work_elems=2), dict(scales=None), dict(clip_mode=2, scales=None),
    dict(clip_mode=3), dict(mode=2), dict(div=0.0), dict(clip=0.0), dict(rows=0), dict(B=0), dict(nlayers=-1),
    dict(nin=0), dict(nout=0),
    # the family's own: T < 1, r > 16, r T > 8192, b_out alignment, the scratch buffers
    dict(T=0), dict(B=34, rows=2), dict(T=4097), dict(B=32, rows=2, T=513), dict(b=68),
    dict(work=ctypes.c_void_p(68)), dict(partials=None), dict(partials=ctypes.c_void_p(72)), dict(partial_elems=107),
    dict(fn="sqnorm", work=None), dict(fn="sqnorm", work=ctypes.c_void_p(68)), dict(fn="sqnorm", slot0=-1),
    dict(fn="sqnorm", slot0=1), dict(fn="sqnorm", T=0), dict(fn="sqnorm", B=34, rows=2), dict(fn="sqnorm", T=4097),
    dict(fn="work", T=4097), dict(fn="partial", rows=4),
], ids=str)
def test_refusals_before_any_hip_call(kw):
    import efl
    assert call(**kw) == -3
    assert efl.lib.raw().efl_last_error().decode()


def test_no_layers_and_sizes():
    assert call(nlayers=0, table=False) == 0 and call(fn="sqnorm", nlayers=0, table=False) == 0
    # B 6, rows 3, T 5: P = 10, one 64-row tile, one pair per microbatch; 3 splits of pad4(8 * 4) + pad4(4) floats
    assert call(fn="work") == 3 and call(fn="partial") == 3 * 36
    # B 34, rows 17, T 100: P = 200, 4 tiles, 10 pairs; 17 rows in 9 splits of 2; 5 x 3 weights, no bias
    kw = dict(B=34, rows=17, T=100, nin=5, nout=3, xs=5, ds=3, b=None)
    assert call(fn="work", **kw) == 17 * 10 and call(fn="partial", **kw) == 9 * 16
