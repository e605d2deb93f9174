"""GPU: efl_dp_embed_clip_sum (csrc/dpembed.hip) through efl.privacy.dp_embed_clip_sum_noise,
dp_factored_clip_sum_noise and the DP optimisers' embedding_layers=, against the float64 reference of
tests/test_dp_embed_host.py (np.add.at of every microbatch's rows into a dense array)."""
import numpy as np
import pytest
import torch

from oracle import mask
from test_dp_dense_gpu import SEED, CTR, stream
from test_dp_dense_host import dense_case, zero_microbatch
from test_dp_dense_host import materialised as dense_materialised
from test_dp_embed_host import CASES, embed_case, materialised
from test_dp_gpu import dp, kernel_normals, ulps  # noqa: F401  (dp is a fixture)

pytestmark = pytest.mark.gpu


def on_gpu(case):
    return [(torch.from_numpy(ids).cuda(), torch.from_numpy(d).cuda(), V, w) for ids, d, V, w in case]


def want_scales(S, clip):
    with np.errstate(divide="ignore"):
        return (clip * np.minimum(1.0 / np.sqrt(S), 1.0 / clip)).astype(np.float32)


@pytest.mark.parametrize("B,rows,layers", CASES)
@pytest.mark.parametrize("clip", [0.5, 3.0])
def test_scales_against_materialised_float64(dp, B, rows, layers, clip):
    case = embed_case(B, rows, layers)
    _, sc = dp.dp_embed_clip_sum_noise(on_gpu(case), rows, clip, 1, clip, float(rows), stream(), return_scales=True)
    sc = sc.cpu().numpy()
    assert ulps(sc, want_scales(materialised(case, rows)[1], clip)).max() <= 1
    assert sc[0] == 1.0 and sc[zero_microbatch(rows)] == 1.0 and (sc < 1.0).any()


@pytest.mark.parametrize("B,rows,layers", CASES)
@pytest.mark.parametrize("mode,div", [(0, 256.0), (0, 3.0), (1, 256.0), (1, 3.0)])
def test_sum_and_noise_given_scales(dp, B, rows, layers, mode, div):
    """|got - ref| <= (n_v + 3) 2^-24 (sum |t d| + |noise|) / |div| per element of row v, n_v the entries
    that hit it: one rounding of t = s w, one of each product, at most n_v - 1 of the accumulation, one of
    the noise add, one of the divide. ref takes the float64 sum and the kernel's own normals; the noise is
    z sigma (mode 1) or z sigma sum (mode 0). A second call at the same stream position gives the same
    bytes, and the output is bit for bit efl_dp_noise's steps (oracle.mask.dp_noise) on the plain sums (a
    call with sigma 0 and divisor 1), zeros in the rows that are not hit."""
    case, sigma = embed_case(B, rows, layers), 1.1
    s = np.random.default_rng(rows).uniform(0.1, 1.0, rows).astype(np.float32)
    sg = torch.from_numpy(s).cuda()
    calls = []
    for _ in range(2):
        st = stream()
        calls.append(dp.dp_embed_clip_sum_noise(on_gpu(case), rows, None, mode, sigma, div, st, scales=sg))
        assert st.counter == CTR + sum((V * d.shape[-1] + 3) // 4 for _, d, V, _ in case)
    plain = dp.dp_embed_clip_sum_noise(on_gpu(case), rows, None, 1, 0.0, 1.0, stream(), scales=sg)
    ctr = CTR
    for (total, mag, hits), g, g2, v in zip(materialised(case, rows, s.astype(np.float64))[0], *calls, plain):
        g, v = g.cpu().numpy(), v.cpu().numpy()
        assert g.shape == total.shape and np.array_equal(g.view(np.uint32), g2.cpu().numpy().view(np.uint32))
        assert not v[hits == 0].any()
        z = kernel_normals(dp, SEED, ctr, g.size).reshape(g.shape)
        ctr += (g.size + 3) // 4
        assert np.array_equal(g.view(np.uint32), mask.dp_noise(v, SEED, 0, mode, sigma, div, z=z).view(np.uint32))
        noise = z.astype(np.float64) * np.float32(sigma).astype(np.float64) * (total if mode == 0 else 1.0)
        bound = (hits[:, None] + 3) * 2.0 ** -24 * (mag + np.abs(noise)) / abs(div)
        assert (np.abs(g.astype(np.float64) - (total + noise) / div) <= bound).all()


@pytest.mark.parametrize("B,rows,layers", CASES[:2])
@pytest.mark.parametrize("clip", [0.5, 3.0])
def test_shared_norm_of_dense_and_embedding_layers(dp, B, rows, layers, clip):
    dense, embed = dense_case(B, rows)[:1], embed_case(B, rows, layers)[:1]
    dn = [(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), b) for x, d, b in dense]
    douts, couts, eouts, sc = dp.dp_factored_clip_sum_noise(dn, [], rows, clip, 1, clip, float(rows), stream(),
                                                            return_scales=True, embedding_layers=on_gpu(embed))
    assert len(douts) == 1 and couts == [] and eouts[0].shape == (embed[0][2], embed[0][1].shape[-1])
    S = dense_materialised(dense, rows)[1] + materialised(embed, rows)[1]
    sc = sc.cpu().numpy()
    assert ulps(sc, want_scales(S, clip)).max() <= 1
    assert sc[zero_microbatch(rows)] == 1.0 and (sc < 1.0).any()


class Recommender(torch.nn.Module):
    def __init__(self, bag=None):
        super().__init__()
        torch.manual_seed(3)
        self.bag = bag or torch.nn.EmbeddingBag(20, 4, mode="mean")
        self.emb, self.top = torch.nn.Embedding(15, 3), torch.nn.Linear(10, 5)

    def forward(self, a, b, **kw):
        return self.top(torch.cat([self.bag(input=a, **kw), self.emb(b).flatten(1)], 1))


def optimizer(dp, model, path, nm, clip=1.0):
    return dp.DPGradientDescentGaussianOptimizer(
        list(model.parameters()), noise_multiplier=1.1, l2_norm_clip=clip, num_microbatches=nm, learning_rate=0.5,
        microbatch_gradients=path, dense_layers=[model.top], embedding_layers=[model.bag, model.emb])


@pytest.mark.parametrize("nm", [12, 4])
@pytest.mark.parametrize("clip", [None, 1.0])
def test_optimizer_factored_against_loop(dp, nm, clip):
    """compute_gradients under "factored" against "loop" for tables under a dense layer, same seed and
    stream position, within test_dp_dense_gpu's bound for every variable, the tables included:
    (nm + 2) 2^-24 (sum |terms| + |noise|) plus 4 ulp of scale on sum |terms|, over the divisor. The ids go
    in by keyword for the bag."""
    model, B = Recommender().cuda(), 12
    gen = torch.Generator(device="cuda").manual_seed(1)
    a, b = torch.randint(0, 20, (B, 3), device="cuda", generator=gen), torch.randint(0, 15, (B, 2), device="cuda", generator=gen)
    y = torch.arange(B, device="cuda") % 5
    params, got = list(model.parameters()), {}
    for path in ("loop", "factored"):
        dp.set_noise_seed(77, 0)
        opt = optimizer(dp, model, path, nm, clip)
        loss = torch.nn.functional.cross_entropy(model(a, b), y, reduction="none")
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
        assert got["factored"][k].shape == tuple(p.shape)
        assert (np.abs(got["loop"][k].reshape(-1) - got["factored"][k].reshape(-1)) <= bound).all(), k


@pytest.mark.parametrize("make,match", [
    (lambda nn: nn.Embedding(20, 4, padding_idx=0), "padding_idx"), (lambda nn: nn.EmbeddingBag(20, 4, max_norm=1.0), "max_norm"),
    (lambda nn: nn.EmbeddingBag(20, 4, scale_grad_by_freq=True), "scale_grad_by_freq"),
    (lambda nn: nn.EmbeddingBag(20, 4, sparse=True), "sparse"), (lambda nn: nn.EmbeddingBag(20, 4, mode="max"), 'mode "sum" or "mean"')])
def test_refused_modules(dp, make, match):
    with pytest.raises(dp.errors.InvalidArgumentError, match=match):
        optimizer(dp, Recommender(make(torch.nn)), "factored", 12)


def test_refused_calls(dp):
    a, b = torch.zeros(12, 3, dtype=torch.long, device="cuda"), torch.zeros(12, 2, dtype=torch.long, device="cuda")
    for model, first, kw in ((Recommender(torch.nn.EmbeddingBag(20, 4, mode="sum")), a, dict(per_sample_weights=torch.ones(12, 3, device="cuda"))),
                             (Recommender(), a.flatten(), dict(offsets=torch.arange(0, 36, 3, device="cuda")))):
        opt = optimizer(dp, model.cuda(), "factored", 12)
        with pytest.raises(dp.errors.InvalidArgumentError, match="offsets .* and per_sample_weights are not supported"):
            opt.compute_gradients(model(first, b, **kw).sum(1), list(model.parameters()))
    d = torch.zeros(12, 4, device="cuda")
    with pytest.raises(dp.errors.InvalidArgumentError, match="integer dtype"):
        dp.dp_embed_clip_sum_noise([(a.float(), d, 20, 1.0)], 12, 1.0, 1, 1.0)
    with pytest.raises(dp.errors.InvalidArgumentError, match="more than 8192 entries"):
        dp.dp_embed_clip_sum_noise([(torch.zeros(12, 683, dtype=torch.long, device="cuda"), d, 20, 1.0)], 12, 1.0, 1, 1.0)
    model = Recommender().cuda()
    with pytest.raises(dp.errors.InvalidArgumentError, match="not the weight or bias"):
        optimizer(dp, model, "factored", 12).compute_gradients(model(a, b).sum(1), [torch.nn.Linear(2, 2).cuda().weight])
