"""CPU: the float64 reference of tests/test_dp_embed_gpu.py (np.add.at of every microbatch's weighted rows
of d into a dense [V, dim] array: its squared norm, and the clipped sum), its inputs, and
efl_dp_embed_*'s argument checks, which run before any HIP call (csrc/dpembed.hip)."""
import ctypes
import functools

import numpy as np

from test_dp_dense_host import zero_microbatch

TILE = 4096         # efl.lib.DP_EMBED_NOISE_TILE (checked below): elements of a table per noise workgroup
# (B, rows, ((V, dim, L, kind), ...)); kind None: an Embedding, d [B, L, dim]; "sum" / "mean": a bag, d [B, dim]
CASES = [(6, 6, ((11, 3, 1, None), (9, 8, 1, "sum"))),          # r = 1, L = 1; V dim % 4 != 0; two layers
         (6, 2, ((23, 3, 5, "mean"), (13, 2, 3, None))),        # r = 3; N = 30 and 18; w = 1 / 5; few rows, many repeats
         (32, 2, ((200, 8, 4, "sum"),)),                        # r = 16; L a power of two
         (12, 4, ((1029, 8, 2, None), (2741, 3, 5, "mean"))),   # two tiles and a ragged tail; rows astride the tiles
         (512, 32, ((9000, 8, 16, "mean"),))]                   # N = 8,192, the limit; 17 tiles and a tail


@functools.lru_cache(maxsize=None)
def embed_case(B, rows, layers):
    """[(ids [B, L] int64, d float32, V, w)]: seeded ids with 0, V - 1 and the rows at both ends of the
    first two noise tiles among them, one id repeated inside the last example, in the example before it and
    in the first; d = 3 x normals, microbatch 0 scaled by 1e-3 (unclipped), microbatch zero_microbatch(rows)
    all zero."""
    rng = np.random.default_rng(B * 1000 + rows)
    r, case, z = B // rows, [], zero_microbatch(rows)
    for V, dim, L, kind in layers:
        ids = rng.integers(0, V, (B, L))
        special = [v for v in (0, V - 1, TILE // dim - 1, TILE // dim, 2 * TILE // dim - 1, 2 * TILE // dim) if v < V]
        ids.reshape(-1)[rng.choice(np.arange(1, B * L - 2 * L), len(special), replace=False)] = special
        ids[0, 0] = ids[-2, 0] = ids[-1, -1] = ids[-1, 0]
        d = (3 * rng.standard_normal((B, dim) if kind else (B, L, dim))).astype(np.float32)
        d[:r] *= np.float32(1e-3)
        d[z * r:(z + 1) * r] = 0
        case.append((ids, d, V, float(np.float32(1.0 / L)) if kind == "mean" else 1.0))
    return case


def materialised(case, rows, scales=None):
    """([(sum [V, dim], sum of magnitudes [V, dim], entries per row [V])], S [rows]) in float64: every
    microbatch's weighted rows of d added into a dense array, its squared norm into S, the array times
    scales[m] (1 without scales) into the sum."""
    S, out = np.zeros(rows), []
    for ids, d, V, w in case:
        B, L = ids.shape
        de = np.broadcast_to(d.astype(np.float64).reshape(B, -1, d.shape[-1]), (B, L, d.shape[-1])) * w
        total, mag = np.zeros((V, d.shape[-1])), np.zeros((V, d.shape[-1]))
        for m, (i, g) in enumerate(zip(ids.reshape(rows, -1), de.reshape(rows, -1, d.shape[-1]))):
            G = np.zeros_like(total)
            np.add.at(G, i, g)
            S[m] += (G ** 2).sum()
            s = 1.0 if scales is None else float(scales[m])
            total += s * G
            np.add.at(mag, i, np.abs(s * g))
        out.append((total, mag, np.bincount(ids.reshape(-1), minlength=V)))
    return out, S


def test_argument_errors_without_gpu():
    import efl
    lib = efl.lib.raw()
    p = ctypes.c_void_p(64)
    assert efl.lib.DP_EMBED_NOISE_TILE == TILE

    def table(ids=64, d=64, out=64, V=10, dim=3, L=5, rs=15, ls=3):
        arr = (efl.lib.DpEmbed * 1)()
        arr[0].ids, arr[0].d, arr[0].out, arr[0].V, arr[0].dim, arr[0].L = ids, d, out, V, dim, L
        arr[0].d_row_stride, arr[0].d_l_stride, arr[0].w = rs, ls, 1.0
        return arr

    def call(nlayers=1, B=6, rows=3, clip_mode=1, clip=1.0, mode=1, div=2.0, scales=p, work=p, work_elems=3, scratch=p,
             scratch_bytes=1 << 20, with_table=True, **layer):
        return lib.efl_dp_embed_clip_sum(table(**layer) if with_table else None, nlayers, B, rows, clip_mode, clip, mode,
                                         1.0, div, 7, scales, work, work_elems, scratch, scratch_bytes, None)

    bad = [dict(ids=None), dict(d=None), dict(out=None), dict(out=72), dict(with_table=False), dict(rows=4),
           dict(B=34, rows=2, L=1, rs=3), dict(rows=0), dict(nlayers=-1), dict(V=0), dict(dim=0), dict(L=0),
           dict(B=2048, rows=128), dict(rs=14), dict(ls=2), dict(ls=0, rs=2), dict(work=None), dict(work_elems=2),
           dict(scratch=None), dict(scratch=72), dict(scratch_bytes=15), dict(scales=None),
           dict(clip_mode=2, scales=None), dict(clip_mode=3), dict(mode=2), dict(div=0.0), dict(clip=0.0)]
    for kw in bad:
        assert call(**kw) == -3, kw
        assert lib.efl_last_error().decode()
    assert "8192 entries" in (call(B=2048, rows=128), lib.efl_last_error().decode())[1]
    assert call(nlayers=0, with_table=False) == 0               # no layers: a no-op
    assert lib.efl_dp_embed_work_elems(3, 5) == 15 and lib.efl_dp_embed_work_elems(3, 0) == -3
    # 30 sorted ids, 30 combined rows of 3 floats and one tile's range, each padded to 16 bytes
    assert lib.efl_dp_embed_scratch_bytes(table(), 1, 6) == 240 + 368 + 16
    assert lib.efl_dp_embed_scratch_bytes(table(), 1, 2048) == -3
    assert lib.efl_dp_embed_sqnorm(table(ids=None), 1, 6, 3, p, 0, 1, None) == -3
    assert lib.efl_dp_embed_sqnorm(table(), 1, 6, 3, p, 1, 1, None) == -3
