"""GPU: efl_dp_seq_clip_sum (csrc/dpseq.hip) through efl.privacy.dp_dense_clip_sum_noise and the DP
optimisers' microbatch_gradients="factored" for a Linear over [B, T, in], against float64 numpy that
materialises every microbatch's G_i = D_i^T X_i. The kernel's position tile and K-chunk are both 64."""
import functools

import numpy as np
import pytest
import torch

from oracle import mask
from test_dp_gpu import dp, kernel_normals  # noqa: F401  (dp is a fixture)

pytestmark = pytest.mark.gpu

SEED, CTR = 21, 5
# (B, rows, T, in, out, bias, columns of row padding); P = B / rows * T rows per microbatch
CASES = [(2, 2, 1, 5, 3, True, 0),        # P = 1; K tails 5 / 3
         (2, 2, 7, 36, 10, False, 0),     # P below one MFMA tile; 36 / 10; no bias
         (2, 2, 17, 5, 3, True, 0),       # P = 17, one past a 16-row MFMA tile
         (4, 4, 64, 8, 4, True, 0),       # P = the position tile, 16-byte loads
         (2, 2, 65, 65, 3, True, 0),      # P = tile + 1: a ragged second tile, the off-diagonal pair; in = K-chunk + 1
         (4, 2, 33, 36, 10, True, 4),     # r = 2, T = tile / 2 + 1: a microbatch spanning examples; row stride above the width
         (17, 17, 3, 5, 3, True, 3)]      # rows = 17: a ragged last split group; padded rows read by dwords


def stream():
    from efl.privacy.secret_sharing import NoiseStream
    return NoiseStream(SEED, CTR)


@functools.lru_cache(maxsize=None)
def seq_case(B, rows, T, nin, nout, bias, pad):
    """Seeded normals [B, T, width + pad], microbatch 0 scaled by 1e-3 (unclipped) and the last by 1e3
    (clipped), with the float64 reference: S [rows] and its bound dS from the materialised gradients."""
    rng, r = np.random.default_rng(1000 * B + 10 * T + nin), B // rows
    x, d = (rng.standard_normal((B, T, w + pad)).astype(np.float32) for w in (nin, nout))
    for t in (x, d):
        t[:r] *= np.float32(1e-3)
        t[-r:] *= np.float32(1e3)
    X, D = x[..., :nin].astype(np.float64).reshape(rows, r * T, nin), d[..., :nout].astype(np.float64).reshape(rows, r * T, nout)
    G, beta = np.einsum("ipo,ipn->ion", D, X), float(bias)
    S = (G ** 2).sum(axis=(1, 2)) + beta * (D.sum(axis=1) ** 2).sum(axis=1)
    ax, ad = (np.einsum("ipk,iqk->ipq", np.abs(M), np.abs(M)) for M in (X, D))
    dS = (nin + nout + (r * T) ** 2 + 8) * 2.0 ** -53 * (ad * (ax + beta)).sum(axis=(1, 2))
    return x, d, X, D, S, dS


def on_gpu(case):
    x, d = seq_case(*case)[:2]
    nin, nout, bias = case[3:6]
    return [(torch.from_numpy(x).cuda()[..., :nin], torch.from_numpy(d).cuda()[..., :nout], bias)]


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("clip", [0.5, 3.0])
def test_scales_against_materialised_float64(dp, case, clip):
    """scale = clip min(1 / sqrt(S), 1 / clip) decreases in S, and the kernel's S is the exact one within
    dS = gamma sum_{p,p'} (|x_p| . |x_p'| + beta)(|d_p| . |d_p'|), gamma = (in + out + P^2 + 8) 2^-53: the
    float scale lies between the float roundings of the formula at S + dS and at S - dS. Two runs give
    the same bytes."""
    rows, (S, dS) = case[1], seq_case(*case)[4:]
    runs = [dp.dp_dense_clip_sum_noise(on_gpu(case), rows, clip, 1, clip, float(rows), stream(), return_scales=True)
            for _ in range(2)]
    sc = runs[0][1].cpu().numpy()

    def scale(s):
        with np.errstate(divide="ignore"):
            return (clip * np.minimum(1.0 / np.sqrt(np.maximum(s, 0.0)), 1.0 / clip)).astype(np.float32)

    assert (scale(S + dS) <= sc).all() and (sc <= scale(S - dS)).all(), (sc, scale(S))
    assert sc[0] == 1.0 and sc[-1] < 1.0
    assert np.array_equal(sc.view(np.uint32), runs[1][1].cpu().numpy().view(np.uint32))
    for a, b in zip(runs[0][0][0], runs[1][0][0]):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("mode,div", [(0, 3.0), (1, 256.0)])
def test_sum_and_noise_given_scales(dp, case, mode, div):
    """Given scales and sigma = 0: |got - exact| <= (B T + splits + 3) 2^-24 sum_k |s d x| per element (the
    bias: sum |s d|). With noise: bit for bit efl_dp_noise's steps (oracle.mask.dp_noise) on those plain
    sums with the kernel's normals at the stream's positions, weight then bias."""
    B, rows, T, nin, nout, bias, _ = case
    X, D = (m.reshape(B * T, -1) for m in seq_case(*case)[2:4])
    s = np.random.default_rng(rows).uniform(0.1, 1.0, rows).astype(np.float32)
    st, sigma = stream(), 1.1
    sg = torch.from_numpy(s).cuda()
    got = dp.dp_dense_clip_sum_noise(on_gpu(case), rows, None, mode, sigma, div, st, scales=sg)[0]
    assert st.counter == CTR + (nin * nout + 3) // 4 + ((nout + 3) // 4 if bias else 0)
    plain = dp.dp_dense_clip_sum_noise(on_gpu(case), rows, None, 1, 0.0, 1.0, stream(), scales=sg)[0]
    sd = D * np.repeat(s.astype(np.float64), B // rows * T)[:, None]
    splits = -(-rows // -(-rows // min(rows, 16)))
    pairs = [(got[0], plain[0], sd.T @ X, np.abs(sd).T @ np.abs(X))]
    if bias:
        pairs.append((got[1], plain[1], sd.sum(axis=0), np.abs(sd).sum(axis=0)))
    else:
        assert got[1] is None
    ctr = CTR
    for g, v, total, mag in pairs:
        g, v = g.cpu().numpy(), v.cpu().numpy()
        assert g.shape == total.shape
        assert (np.abs(v.astype(np.float64) - total) <= (B * T + splits + 3) * 2.0 ** -24 * mag).all()
        z = kernel_normals(dp, SEED, ctr, g.size).reshape(g.shape)
        ctr += (g.size + 3) // 4
        assert np.array_equal(g.view(np.uint32), mask.dp_noise(v, SEED, 0, mode, sigma, div, z=z).view(np.uint32))


@pytest.mark.parametrize("nm", [8, 4])
def test_optimizer_factored_against_loop(dp, nm):
    """Linear(12 -> 8) over [8, 5, 12], mean over T, Linear(8 -> 3): compute_gradients under "factored"
    against "loop", same seed and stream position, within tests/test_dp_dense_gpu.py's bound with the B T
    (example, position) rows as the terms: ((B T + 2) 2^-24 (sum |terms| + |noise|) + 4 ulp of scale on
    sum |terms|) over the divisor, terms the rows' s_k d_k (x) x_k."""
    torch.manual_seed(3)
    B, T, clip = 8, 5, 1.0
    l1, l2 = torch.nn.Linear(12, 8).cuda(), torch.nn.Linear(8, 3).cuda()
    x = torch.randn(B, T, 12, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    y = torch.arange(B, device="cuda") % 3
    params, got = [*l1.parameters(), *l2.parameters()], {}
    for path in ("loop", "factored"):
        dp.set_noise_seed(77, 0)
        opt = dp.DPGradientDescentGaussianOptimizer(params, noise_multiplier=1.1, l2_norm_clip=clip, num_microbatches=nm,
                                                    learning_rate=0.5, microbatch_gradients=path, dense_layers=[l1, l2])
        h1 = l1(x)
        h2 = l2(torch.tanh(h1).mean(1))
        loss = torch.nn.functional.cross_entropy(h2, y, reduction="none")
        got[path] = [g.cpu().numpy().astype(np.float64) for g, _ in opt.compute_gradients(loss, params)]
        assert dp.noise_stream().counter == sum((p.numel() + 3) // 4 for p in params)
    rows = [torch.autograd.grad(r.sum(), params, retain_graph=True) for r in loss.reshape(nm, -1)]
    norm = np.array([np.sqrt(sum((g.double() ** 2).sum().item() for g in r)) for r in rows])
    s = clip * np.minimum(1.0 / norm, 1.0 / clip)
    d1, d2 = (t.double().cpu().numpy() for t in torch.autograd.grad(loss.sum(), [h1, h2]))
    x1, x2 = x.double().cpu().numpy().reshape(B * T, 12), torch.tanh(h1).mean(1).detach().double().cpu().numpy()
    d1, d2 = np.abs(d1.reshape(B * T, 8) * np.repeat(s, B // nm * T)[:, None]), np.abs(d2 * np.repeat(s, B // nm)[:, None])
    mags = [d1.T @ np.abs(x1), d1.sum(axis=0), d2.T @ np.abs(x2), d2.sum(axis=0)]
    ctr = 0
    for k, (p, mag) in enumerate(zip(params, mags)):
        z = np.abs(kernel_normals(dp, 77, ctr, p.numel()).astype(np.float64)) * np.float32(1.1 * clip)
        ctr += (p.numel() + 3) // 4
        bound = ((B * T + 2) * 2.0 ** -24 * (mag.reshape(-1) + z) + 4 * 2.0 ** -23 * mag.reshape(-1)) / nm
        assert (np.abs(got["loop"][k].reshape(-1) - got["factored"][k].reshape(-1)) <= bound).all(), k


def test_sequence_refusals(dp):
    x, d = torch.zeros(32, 513, 4, device="cuda"), torch.zeros(32, 513, 2, device="cuda")
    with pytest.raises(dp.errors.InvalidArgumentError, match="r T > 8192"):
        dp.dp_dense_clip_sum_noise([(x, d, True)], 2, 1.0, 1, 1.0)
    with pytest.raises(dp.errors.InvalidArgumentError, match="equal middle dimensions"):
        dp.dp_dense_clip_sum_noise([(x, d[:, :512], True)], 32, 1.0, 1, 1.0)
