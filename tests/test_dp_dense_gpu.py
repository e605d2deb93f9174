"""GPU: efl_dp_dense_clip_sum (csrc/dpdense.hip) through efl.privacy.dp_dense_clip_sum_noise and the DP
optimisers' microbatch_gradients="factored", against float64 numpy that materialises every microbatch's
G_i = D_i^T X_i (tests/test_dp_dense_host.py, which also shows on the CPU that the Gram identity the
kernel uses agrees with that reference on these inputs)."""
import numpy as np
import pytest
import torch

from oracle import mask
from test_dp_dense_host import CASES, dense_case, materialised, zero_microbatch
from test_dp_gpu import dp, kernel_normals, ulps  # noqa: F401  (dp is a fixture)

pytestmark = pytest.mark.gpu

SEED, CTR = 21, 5


def stream():
    from efl.privacy.secret_sharing import NoiseStream
    return NoiseStream(SEED, CTR)


def on_gpu(case):
    return [(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), bias) for x, d, bias in case]


@pytest.mark.parametrize("B,rows", CASES)
@pytest.mark.parametrize("clip", [0.5, 3.0])
def test_scales_against_materialised_float64(dp, B, rows, clip):
    case = dense_case(B, rows)
    _, sc = dp.dp_dense_clip_sum_noise(on_gpu(case), rows, clip, 1, clip, float(rows), stream(), return_scales=True)
    sc = sc.cpu().numpy()
    with np.errstate(divide="ignore"):
        want = (clip * np.minimum(1.0 / np.sqrt(materialised(case, rows)[1]), 1.0 / clip)).astype(np.float32)
    assert ulps(sc, want).max() <= 1
    assert sc[0] == 1.0 and sc[zero_microbatch(rows)] == 1.0 and (sc < 1.0).any()


@pytest.mark.parametrize("B,rows", CASES)
@pytest.mark.parametrize("mode,div", [(0, 256.0), (0, 3.0), (1, 256.0), (1, 3.0)])
def test_sum_and_noise_given_scales(dp, B, rows, mode, div):
    """|got - ref| <= (B + 3) 2^-24 (sum_k |s d x| + |noise|) / |div| per element: one rounding of s d,
    at most B of the accumulation in any order, one of the noise add, one of the divide. ref takes the
    float64 sum and the kernel's own normals; the noise is z sigma (mode 1) or z sigma sum (mode 0).
    The bias has sum_k |s d| for sum_k |s d x|. A second call at the same stream position gives the
    same bytes, and the output is bit for bit efl_dp_noise's steps (oracle.mask.dp_noise) on the plain
    sums (a call with sigma 0 and divisor 1), in the fused epilogue and in the unfused one alike."""
    case, sigma = dense_case(B, rows), 1.1
    s = np.random.default_rng(rows).uniform(0.1, 1.0, rows).astype(np.float32)
    calls = []
    for _ in range(2):
        st = stream()
        calls.append(dp.dp_dense_clip_sum_noise(on_gpu(case), rows, None, mode, sigma, div, st,
                                                scales=torch.from_numpy(s).cuda()))
        assert st.counter == CTR + sum((i * o + 3) // 4 + ((o + 3) // 4 if b else 0) for (x, d, b) in case
                                       for i, o in [(x.shape[1], d.shape[1])])
    plain = dp.dp_dense_clip_sum_noise(on_gpu(case), rows, None, 1, 0.0, 1.0, stream(), scales=torch.from_numpy(s).cuda())
    sk = np.repeat(s.astype(np.float64), B // rows)
    ctr = CTR
    for (x, d, bias), got, again, pl in zip(case, *calls, plain):
        x64, sd = x.astype(np.float64), d.astype(np.float64) * sk[:, None]
        pairs = [(got[0], again[0], pl[0], sd.T @ x64, np.abs(sd).T @ np.abs(x64))]
        if bias:
            pairs.append((got[1], again[1], pl[1], sd.sum(axis=0), np.abs(sd).sum(axis=0)))
        else:
            assert got[1] is None
        for g, g2, v, total, mag in pairs:
            g = g.cpu().numpy()
            assert g.shape == total.shape and np.array_equal(g.view(np.uint32), g2.cpu().numpy().view(np.uint32))
            z = kernel_normals(dp, SEED, ctr, g.size).reshape(g.shape)
            ctr += (g.size + 3) // 4
            assert np.array_equal(g.view(np.uint32), mask.dp_noise(v.cpu().numpy(), SEED, 0, mode, sigma, div, z=z).view(np.uint32))
            z = z.astype(np.float64)
            noise = z * np.float32(sigma).astype(np.float64) * (total if mode == 0 else 1.0)
            bound = (B + 3) * 2.0 ** -24 * (mag + np.abs(noise)) / abs(div)
            err = np.abs(g.astype(np.float64) - (total + noise) / div)
            assert (err <= bound).all()


def mlp():
    torch.manual_seed(3)
    nn = torch.nn
    return nn.Sequential(nn.Linear(36, 33), nn.ReLU(), nn.Linear(33, 8), nn.ReLU(), nn.Linear(8, 5)).cuda()


def optimizer(dp, model, path, nm, clip=1.0, **kw):
    return dp.DPGradientDescentGaussianOptimizer(list(model.parameters()), noise_multiplier=1.1, l2_norm_clip=clip,
                                                 num_microbatches=nm, learning_rate=0.5, microbatch_gradients=path,
                                                 dense_layers=[m for m in model if isinstance(m, torch.nn.Linear)], **kw)


@pytest.mark.parametrize("nm", [12, 4])
@pytest.mark.parametrize("clip", [None, 1.0])
def test_optimizer_factored_against_loop(dp, nm, clip):
    """compute_gradients under "factored" against "loop", same seed and stream position, within
    test_optimizer_step_batched_against_loop's bound: (rows + 2) 2^-24 (sum |terms| + |noise|) plus
    4 ulp of scale on sum |terms| (the loop rounds the norm, the reciprocal and the product in fp32),
    over the divisor, rows the number of microbatches; without a clip the noise is z sigma times the
    sum."""
    model, B = mlp(), 12
    x = torch.randn(B, 36, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    y = torch.arange(B, device="cuda") % 5
    params, got = list(model.parameters()), {}
    for path in ("loop", "factored"):
        dp.set_noise_seed(77, 0)
        opt = optimizer(dp, model, path, nm, clip)
        loss = torch.nn.functional.cross_entropy(model(x), y, reduction="none")
        got[path] = [g.cpu().numpy().astype(np.float64) for g, _ in opt.compute_gradients(loss, params)]
        assert dp.noise_stream().counter == sum((p.numel() + 3) // 4 for p in params)
    rows = [torch.autograd.grad(r.sum(), params, retain_graph=True) for r in loss.reshape(nm, -1)]
    norm = np.array([np.sqrt(sum((g.double() ** 2).sum().item() for g in r)) for r in rows])
    s = np.ones(nm) if clip is None else clip * np.minimum(1.0 / norm, 1.0 / clip)
    ctr = 0
    for k, p in enumerate(params):
        terms = np.stack([r[k].double().cpu().numpy().reshape(-1) * si for r, si in zip(rows, s)])
        z = np.abs(kernel_normals(dp, 77, ctr, p.numel()).astype(np.float64)) * np.float32(1.1 * (clip or 1.0))
        ctr += (p.numel() + 3) // 4
        mag = np.abs(terms).sum(axis=0)
        zs = z * mag if clip is None else z
        bound = ((nm + 2) * 2.0 ** -24 * (mag + zs) + 4 * 2.0 ** -23 * mag) / nm
        assert (np.abs(got["loop"][k].reshape(-1) - got["factored"][k].reshape(-1)) <= bound).all(), k


def test_factored_refusals(dp):
    model = mlp()
    x = torch.randn(64, 36, device="cuda")
    conv = torch.nn.Conv2d(1, 1, 3).cuda()

    def loss():
        return model(x).sum(1)

    with pytest.raises(dp.errors.InvalidArgumentError, match="not the weight or bias"):
        optimizer(dp, model, "factored", 64).compute_gradients(loss(), list(model.parameters()) + [conv.weight])
    with pytest.raises(dp.errors.InvalidArgumentError, match="r > 16"):
        optimizer(dp, model, "factored", 2).compute_gradients(loss(), list(model.parameters()))      # r = 32
    opt = optimizer(dp, model, "factored", 64)
    model(x)
    with pytest.raises(dp.errors.InvalidArgumentError, match="ran 2 times"):
        opt.compute_gradients(loss(), list(model.parameters()))
