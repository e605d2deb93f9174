"""GPU: efl_dp_conv_clip_sum (csrc/dpconv.hip) through efl.privacy.dp_conv_clip_sum_noise,
dp_factored_clip_sum_noise and the DP optimisers' conv_layers=, against the float64 reference of
tests/test_dp_conv_host.py (unfold and an einsum that materialise every microbatch's gradient)."""
import numpy as np
import pytest
import torch

from oracle import mask
from test_dp_conv_host import CASES, LAYERS, conv_case, materialised, unfolded
from test_dp_dense_gpu import SEED, CTR, stream
from test_dp_dense_host import dense_case, zero_microbatch
from test_dp_dense_host import materialised as dense_materialised
from test_dp_gpu import dp, kernel_normals, ulps  # noqa: F401  (dp is a fixture)

pytestmark = pytest.mark.gpu


def on_gpu(case):
    return [(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), *rest) for x, d, *rest in case]


def want_scales(S, clip):
    with np.errstate(divide="ignore"):
        return (clip * np.minimum(1.0 / np.sqrt(S), 1.0 / clip)).astype(np.float32)


@pytest.mark.parametrize("B,rows", CASES)
@pytest.mark.parametrize("clip", [0.5, 3.0])
def test_scales_against_materialised_float64(dp, B, rows, clip):
    _, sc = dp.dp_conv_clip_sum_noise(on_gpu(conv_case(B, rows)), rows, clip, 1, clip, float(rows), stream(),
                                      return_scales=True)
    sc = sc.cpu().numpy()
    assert ulps(sc, want_scales(materialised(B, rows), clip)).max() <= 1
    assert sc[0] == 1.0 and sc[zero_microbatch(rows)] == 1.0 and (sc < 1.0).any()


@pytest.mark.parametrize("B,rows", CASES)
@pytest.mark.parametrize("mode,div", [(0, 256.0), (0, 3.0), (1, 256.0), (1, 3.0)])
def test_sum_and_noise_given_scales(dp, B, rows, mode, div):
    """|got - ref| <= (B T + 3) 2^-24 (sum_{b,t} |s d u| + |noise|) / |div| per element: one rounding of
    s d, at most B T of the accumulation in any order (the splits included), one of the noise add, one
    of the divide. ref takes the float64 sum and the kernel's own normals; the noise is z sigma (mode 1)
    or z sigma sum (mode 0). The bias has sum |s d| for sum |s d u|. A second call at the same stream
    position gives the same bytes, and the output is bit for bit efl_dp_noise's steps
    (oracle.mask.dp_noise) on the plain sums (a call with sigma 0 and divisor 1)."""
    case, sigma = conv_case(B, rows), 1.1
    s = np.random.default_rng(rows).uniform(0.1, 1.0, rows).astype(np.float32)
    sg = torch.from_numpy(s).cuda()
    numels = [n for x, d, b, k, *_ in case for n in [d.shape[1] * x.shape[1] * k[0] * k[1]] + ([d.shape[1]] if b else [])]
    calls = []
    for _ in range(2):
        st = stream()
        calls.append(dp.dp_conv_clip_sum_noise(on_gpu(case), rows, None, mode, sigma, div, st, scales=sg))
        assert st.counter == CTR + sum((n + 3) // 4 for n in numels)
    plain = dp.dp_conv_clip_sum_noise(on_gpu(case), rows, None, 1, 0.0, 1.0, stream(), scales=sg)
    sk = np.repeat(s.astype(np.float64), B // rows)
    ctr = CTR
    for (x, d, bias, k, st_, p, dil), got, again, pl in zip(case, *calls, plain):
        U, D = unfolded(x, d, k, st_, p, dil, sk)
        T = U.shape[2]
        pairs = [(got[0], again[0], pl[0], np.einsum("bot,bkt->ok", D, U), np.einsum("bot,bkt->ok", np.abs(D), np.abs(U)))]
        if bias:
            pairs.append((got[1], again[1], pl[1], D.sum(axis=(0, 2)), np.abs(D).sum(axis=(0, 2))))
        else:
            assert got[1] is None
        for g, g2, v, total, mag in pairs:
            g = g.cpu().numpy()
            assert g.shape[0] == d.shape[1] and g.shape[1:] == (() if g.ndim == 1 else (x.shape[1], *k))
            assert np.array_equal(g.view(np.uint32), g2.cpu().numpy().view(np.uint32))
            z = kernel_normals(dp, SEED, ctr, g.size).reshape(g.shape)
            ctr += (g.size + 3) // 4
            assert np.array_equal(g.view(np.uint32), mask.dp_noise(v.cpu().numpy(), SEED, 0, mode, sigma, div, z=z).view(np.uint32))
            total, mag, z = total.reshape(g.shape), mag.reshape(g.shape), z.astype(np.float64)
            noise = z * np.float32(sigma).astype(np.float64) * (total if mode == 0 else 1.0)
            bound = (B * T + 3) * 2.0 ** -24 * (mag + np.abs(noise)) / abs(div)
            assert (np.abs(g.astype(np.float64) - (total + noise) / div) <= bound).all()


@pytest.mark.parametrize("B,rows", [(6, 6), (6, 2)])
@pytest.mark.parametrize("clip", [0.5, 3.0])
def test_shared_norm_of_dense_and_conv_layers(dp, B, rows, clip):
    layers = (LAYERS[1], LAYERS[3])
    dense, conv = dense_case(B, rows)[:1], conv_case(B, rows, layers)
    dn = [(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), b) for x, d, b in dense]
    _, _, sc = dp.dp_factored_clip_sum_noise(dn, on_gpu(conv), rows, clip, 1, clip, float(rows), stream(),
                                             return_scales=True)
    S = dense_materialised(dense, rows)[1] + materialised(B, rows, layers)
    sc = sc.cpu().numpy()
    assert ulps(sc, want_scales(S, clip)).max() <= 1
    assert sc[zero_microbatch(rows)] == 1.0 and (sc < 1.0).any()


def cnn(first=None):
    torch.manual_seed(3)
    nn = torch.nn
    return nn.Sequential(first or nn.Conv2d(1, 4, 3, stride=2, padding=1), nn.ReLU(), nn.MaxPool2d(2, 1), nn.Conv2d(4, 6, 2),
                         nn.ReLU(), nn.Flatten(), nn.Linear(96, 8), nn.ReLU(), nn.Linear(8, 5)).cuda()


def optimizer(dp, model, path, nm, clip=1.0):
    return dp.DPGradientDescentGaussianOptimizer(
        list(model.parameters()), noise_multiplier=1.1, l2_norm_clip=clip, num_microbatches=nm, learning_rate=0.5,
        microbatch_gradients=path, dense_layers=[m for m in model if isinstance(m, torch.nn.Linear)],
        conv_layers=[m for m in model if isinstance(m, torch.nn.Conv2d)])


@pytest.mark.parametrize("nm", [12, 4])
@pytest.mark.parametrize("clip", [None, 1.0])
def test_optimizer_factored_against_loop(dp, nm, clip):
    """compute_gradients under "factored" against "loop" for a CNN, same seed and stream position, within
    test_dp_dense_gpu's bound with nm r T_max accumulation roundings in place of nm (T_max = 36, the
    first convolution's output positions): (nm r T_max + 2) 2^-24 (sum |terms| + |noise|) plus 4 ulp of
    scale on sum |terms|, over the divisor."""
    model, B, t_max = cnn(), 12, 36
    x = torch.randn(B, 1, 12, 12, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
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
        bound = ((B * t_max + 2) * 2.0 ** -24 * (mag + zs) + 4 * 2.0 ** -23 * mag) / nm
        assert got["factored"][k].shape == tuple(p.shape)
        assert (np.abs(got["loop"][k].reshape(-1) - got["factored"][k].reshape(-1)) <= bound).all(), k


def test_conv_refusals(dp):
    nn = torch.nn
    for bad in (nn.Conv2d(2, 4, 3, groups=2), nn.Conv2d(1, 4, 3, padding=1, padding_mode="reflect")):
        with pytest.raises(dp.errors.InvalidArgumentError, match="groups = 1 and padding_mode"):
            optimizer(dp, cnn(bad.cuda()), "factored", 12)
    model = cnn()
    x = torch.randn(12, 1, 12, 12, device="cuda")
    opt = optimizer(dp, model, "factored", 12)
    model(x)
    with pytest.raises(dp.errors.InvalidArgumentError, match="ran 2 times"):
        opt.compute_gradients(model(x).sum(1), list(model.parameters()))
