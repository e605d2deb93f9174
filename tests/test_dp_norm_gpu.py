"""GPU: efl_dp_norm_clip_sum (csrc/dpnorm.hip) through efl.privacy.dp_norm_clip_sum_noise and the DP
optimisers' norm_layers= under microbatch_gradients="factored", against float64 numpy that materialises
every microbatch's ggamma = sum d xh and gbeta = sum d. The channel-last kernel's tile is 256 columns, 4 per
lane, its 4 waves take 4 rows each at a time (16 rows per pass); the channel-first one packs 4 channels into
a workgroup, a wave covering 64 dwords or 64 16-byte groups of a run per pass."""
import functools

import numpy as np
import pytest
import torch

from oracle import mask
from test_dp_gpu import dp, kernel_normals  # noqa: F401  (dp is a fixture)

pytestmark = pytest.mark.gpu

SEED, CTR, EPS = 21, 5, 1e-5
# (groups, B, rows, T or L, C, bias, columns of row padding, constant added to x); groups None: channel-last
CASES = [(None, 2, 2, 1, 1, True, 0, 0),      # var = 0: xh = 0
         (None, 2, 2, 1, 5, True, 0, 0),      # below one 16-byte load
         (None, 4, 2, 9, 36, True, 0, 100),   # r = 2, P = 18: a ragged second pass of the waves; |mu| / sigma = 2^7
         (None, 2, 2, 7, 256, True, 0, 0),    # exactly one tile
         (None, 2, 2, 5, 257, True, 0, 0),    # one past a tile, rows read by dwords
         (None, 4, 2, 3, 36, False, 0, 0),    # no bias
         (None, 2, 2, 5, 260, True, 4, 0),    # a padded row stride under 16-byte loads, a second tile of one lane
         (None, 2, 2, 5, 7, True, 3, 0),      # a padded row stride read by dwords
         (None, 17, 17, 2, 5, True, 0, 0),    # 17 rows
         (1, 2, 2, 1, 1, True, 0, 0),         # n = 1
         (3, 2, 2, 1, 6, True, 0, 0),         # L = 1; a second workgroup of 2 channels
         (2, 4, 2, 49, 6, True, 0, 100),      # r = 2; |mu| / sigma = 2^7
         (8, 2, 2, 5, 8, False, 0, 0),        # G = C; no bias
         (1, 2, 2, 65, 4, True, 0, 0),        # one past a wave
         (1, 2, 2, 260, 5, True, 0, 0),       # 16-byte loads, one group past a wave
         (2, 17, 17, 3, 4, True, 0, 0)]       # 17 rows


def stream():
    from efl.privacy.secret_sharing import NoiseStream
    return NoiseStream(SEED, CTR)


@functools.lru_cache(maxsize=None)
def norm_case(G, B, rows, TL, C, bias, pad, shift):
    """Seeded normals (x + shift), microbatch 0's d scaled by 1e-3 (unclipped) and the last one's by 1e3
    (clipped), with the float64 reference per microbatch: ggamma, gbeta, their sums of magnitudes, S and
    dS = 2^-32 sum_c [(sum |d| |xh|)^2 + beta (sum |d|)^2]."""
    rng, r = np.random.default_rng(1000 * B + 10 * TL + C), B // rows
    shape = (B, TL, C + pad) if G is None else (B, C, TL)
    x, d = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    x += np.float32(shift)
    d[:r] *= np.float32(1e-3)
    d[-r:] *= np.float32(1e3)
    X, D = (t[..., :t.shape[-1] - pad].astype(np.float64) for t in (x, d))
    Xg = X if G is None else X.reshape(B, G, -1)
    xh = ((Xg - Xg.mean(-1, keepdims=True)) / np.sqrt(Xg.var(-1, keepdims=True) + EPS)).reshape(X.shape)

    def per_microbatch(m):
        return m.reshape(rows, r * TL, C).sum(1) if G is None else m.reshape(rows, r, C, TL).sum((1, 3))

    gw, gb, aw, ab = (per_microbatch(m) for m in (D * xh, D, np.abs(D * xh), np.abs(D)))
    S, A = ((w ** 2).sum(1) + float(bias) * (b ** 2).sum(1) for w, b in ((gw, gb), (aw, ab)))
    return x, d, gw, gb, aw, ab, S, 2.0 ** -32 * A


def on_gpu(case):
    (x, d), w = norm_case(*case)[:2], case[3 if case[0] else 4]
    return [(torch.from_numpy(x).cuda()[..., :w], torch.from_numpy(d).cuda()[..., :w], case[5], case[0], EPS)]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_scales_against_materialised_float64(dp, case):
    """scale = clip min(1 / sqrt(S), 1 / clip) decreases in S, and the kernel's S is the exact one within dS:
    double arithmetic with fewer than 2^9 roundings per column at these shapes, amplified by
    1 + |mu| / sigma <= 2^8, stays below 2^-36, fp32 statistics or sums are off by 2^-24 or more, so 2^-32
    separates them. The float scale lies between the float roundings of the formula at S + dS and at S - dS.
    Two runs give the same bytes."""
    rows, clip, (S, dS) = case[2], 0.5, norm_case(*case)[6:]
    runs = [dp.dp_norm_clip_sum_noise(on_gpu(case), rows, clip, 1, clip, float(rows), stream(), return_scales=True)
            for _ in range(2)]
    sc = runs[0][1].cpu().numpy()

    def scale(s):
        with np.errstate(divide="ignore"):
            return (clip * np.minimum(1.0 / np.sqrt(np.maximum(s, 0.0)), 1.0 / clip)).astype(np.float32)

    print(case, sc, scale(S))
    assert (scale(S + dS) <= sc).all() and (sc <= scale(S - dS)).all(), (sc, scale(S))
    assert sc[0] == 1.0 and sc[-1] < 1.0
    assert np.array_equal(sc.view(np.uint32), runs[1][1].cpu().numpy().view(np.uint32))
    for a, b in zip(runs[0][0][0], runs[1][0][0]):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("mode,div", [(0, 3.0), (1, 256.0)])
def test_sum_and_noise_given_scales(dp, case, mode, div):
    """Given scales and sigma = 0: |got - exact| <= (rows + 4) 2^-24 sum_i s_i sum |d xh| per element (the
    bias: sum |d|), one rounding of each stacked row plus efl_dp_clip_sum's row-ordered fp32 sum. With noise:
    bit for bit efl_dp_noise's steps (oracle.mask.dp_noise) on those plain sums with the kernel's normals at
    the stream's positions, weight then bias."""
    rows, C, bias = case[2], case[4], case[5]
    gw, gb, aw, ab = norm_case(*case)[2:6]
    s = np.random.default_rng(rows).uniform(0.1, 1.0, rows).astype(np.float32)
    st, sigma, sg = stream(), 1.1, torch.from_numpy(s).cuda()
    got = dp.dp_norm_clip_sum_noise(on_gpu(case), rows, None, mode, sigma, div, st, scales=sg)[0]
    assert st.counter == CTR + (C + 3) // 4 * (2 if bias else 1)
    plain = dp.dp_norm_clip_sum_noise(on_gpu(case), rows, None, 1, 0.0, 1.0, stream(), scales=sg)[0]
    assert bias or got[1] is None
    ctr = CTR
    for g, v, total, mag in [(got[0], plain[0], gw, aw), (got[1], plain[1], gb, ab)][:2 if bias else 1]:
        g, v, s64 = g.cpu().numpy(), v.cpu().numpy(), s.astype(np.float64)
        assert g.shape == (C,)
        err, bound = np.abs(v.astype(np.float64) - s64 @ total), (rows + 4) * 2.0 ** -24 * (s64 @ mag)
        print(case, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        z = kernel_normals(dp, SEED, ctr, C)
        ctr += (C + 3) // 4
        assert np.array_equal(g.view(np.uint32), mask.dp_noise(v, SEED, 0, mode, sigma, div, z=z).view(np.uint32))


def cnn():
    x = torch.randn(8, 1, 6, 6, generator=torch.Generator().manual_seed(1))
    return [torch.nn.Conv2d(1, 4, 3), torch.nn.GroupNorm(2, 4), torch.nn.Linear(64, 3)], x, lambda h: torch.relu(h).flatten(1)


def tower():
    x = torch.randn(8, 5, 12, generator=torch.Generator().manual_seed(1))
    return [torch.nn.Linear(12, 8), torch.nn.LayerNorm(8), torch.nn.Linear(8, 3)], x, lambda h: torch.tanh(h).mean(1)


@pytest.mark.parametrize("nm", [8, 4])
@pytest.mark.parametrize("make", [cnn, tower])
def test_optimizer_factored_against_loop(dp, make, nm):
    """Conv2d(1, 4, 3) -> GroupNorm(2, 4) -> ReLU -> flatten -> Linear, and Linear(12, 8) over [8, 5, 12] ->
    LayerNorm(8) -> tanh -> mean over T -> Linear(8, 3): compute_gradients under "factored" against "loop",
    same seed and stream position, three families under one norm, within
    tests/test_dp_seq_gpu.py::test_optimizer_factored_against_loop's bound ((N + 2) 2^-24 (sum |terms| + |noise|)
    + 4 ulp of scale on sum |terms|) over the divisor, N the (example, position) terms of an element; a norm
    layer's terms are s d xh (the bias: s d)."""
    torch.manual_seed(3)
    layers, x, act = make()
    layers, x, (B, clip) = [m.cuda() for m in layers], x.cuda(), (8, 1.0)
    y = torch.arange(B, device="cuda") % 3
    params, got = [p for m in layers for p in m.parameters()], {}
    for path in ("loop", "factored"):
        dp.set_noise_seed(77, 0)
        opt = dp.DPGradientDescentGaussianOptimizer(
            params, noise_multiplier=1.1, l2_norm_clip=clip, num_microbatches=nm, learning_rate=0.5,
            microbatch_gradients=path, dense_layers=[m for m in layers if isinstance(m, torch.nn.Linear)],
            conv_layers=layers[:1] if make is cnn else [], norm_layers=layers[1:2])
        h0 = layers[0](x)
        h1 = layers[1](h0)
        ins, outs = [x, h0, act(h1)], [h0, h1, layers[2](act(h1))]
        loss = torch.nn.functional.cross_entropy(outs[-1], y, reduction="none")
        got[path] = [g.cpu().numpy().astype(np.float64) for g, _ in opt.compute_gradients(loss, params)]
        assert dp.noise_stream().counter == sum((p.numel() + 3) // 4 for p in params)
    per = [torch.autograd.grad(r.sum(), params, retain_graph=True) for r in loss.reshape(nm, -1)]
    norm = np.array([np.sqrt(sum((g.double() ** 2).sum().item() for g in r)) for r in per])
    s = torch.from_numpy(clip * np.minimum(1.0 / norm, 1.0 / clip)).repeat_interleave(B // nm)
    mags = []                                   # per parameter: (sum |terms|, N)
    for m, xin, d in zip(layers, ins, torch.autograd.grad(loss.sum(), outs, retain_graph=True)):
        xin, sd = xin.detach().double().cpu(), (d.double().cpu() * s.reshape(-1, *[1] * (d.dim() - 1))).abs()
        if isinstance(m, torch.nn.Linear):
            mags += [(sd.flatten(0, -2).T @ xin.abs().flatten(0, -2), sd[..., 0].numel()), (sd.flatten(0, -2).sum(0), sd[..., 0].numel())]
        elif isinstance(m, torch.nn.Conv2d):
            mags += [(torch.nn.grad.conv2d_weight(xin.abs(), m.weight.shape, sd), sd[:, 0].numel()), (sd.sum((0, 2, 3)), sd[:, 0].numel())]
        elif isinstance(m, torch.nn.GroupNorm):
            xh = torch.nn.functional.group_norm(xin, m.num_groups, eps=m.eps).abs()
            mags += [((sd * xh).sum((0, 2, 3)), sd[:, 0].numel()), (sd.sum((0, 2, 3)), sd[:, 0].numel())]
        else:
            xh = torch.nn.functional.layer_norm(xin, m.normalized_shape, eps=m.eps).abs()
            mags += [((sd * xh).sum((0, 1)), sd[..., 0].numel()), (sd.sum((0, 1)), sd[..., 0].numel())]
    ctr = 0
    for k, (p, (mag, N)) in enumerate(zip(params, mags)):
        mag = mag.reshape(-1).numpy()
        z = np.abs(kernel_normals(dp, 77, ctr, p.numel()).astype(np.float64)) * np.float32(1.1 * clip)
        ctr += (p.numel() + 3) // 4
        bound = ((N + 2) * 2.0 ** -24 * (mag + z) + 4 * 2.0 ** -23 * mag) / nm
        diff = np.abs(got["loop"][k].reshape(-1) - got["factored"][k].reshape(-1))
        print(make.__name__, nm, k, float((diff / bound).max()))
        assert (diff <= bound).all(), k


def test_norm_refusals(dp):
    make = dp.DPGradientDescentGaussianOptimizer
    lin, ln = torch.nn.Linear(4, 4).cuda(), torch.nn.LayerNorm(4).cuda()
    for bad in (torch.nn.BatchNorm1d(4), lin, torch.nn.LayerNorm(4, elementwise_affine=False),
                torch.nn.GroupNorm(2, 4, affine=False), torch.nn.LayerNorm((2, 4))):
        with pytest.raises(dp.errors.InvalidArgumentError, match="norm_layers takes"):
            make(list(lin.parameters()), noise_multiplier=1.0, l2_norm_clip=1.0, norm_layers=[bad])
    x = torch.zeros(4, 6, 3, device="cuda")
    with pytest.raises(dp.errors.InvalidArgumentError, match="groups"):
        dp.dp_norm_clip_sum_noise([(x, x, True, 4, EPS)], 4, 1.0, 1, 1.0)
    with pytest.raises(dp.errors.InvalidArgumentError, match="examples per microbatch"):
        dp.dp_norm_clip_sum_noise([(torch.zeros(34, 3, device="cuda"),) * 2 + (True, None, EPS)], 2, 1.0, 1, 1.0)
    params = [*lin.parameters(), *ln.parameters()]
    opt = make(params, noise_multiplier=1.0, l2_norm_clip=1.0, microbatch_gradients="factored", dense_layers=[lin])
    loss = ln(lin(torch.ones(2, 4, device="cuda"))).sum(1)
    with pytest.raises(dp.errors.InvalidArgumentError, match="not the weight or bias"):
        opt.compute_gradients(loss, params)
