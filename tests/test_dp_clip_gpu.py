"""GPU: efl_dp_clip_sum (csrc/dpclip.hip) through efl.privacy.dp_clip_sum_noise and the DP optimisers'
microbatch_gradients="batched".

The kernel's sum is the reference loop's: fp32 `acc = acc + g * s` in row order from 0, every
product and addition rounded on its own, then efl_dp_noise's steps. Given the scales and the kernel's
own normals (read back as tests/test_dp_gpu.py does) the output equals numpy's bit for bit. The
scales come from a double accumulation, so they are the float64 formula rounded once, give or take
a tie."""
import numpy as np
import pytest
import torch

from oracle import mask
from test_dp_gpu import dp, kernel_normals, ulps  # noqa: F401  (dp is a fixture)

pytestmark = pytest.mark.gpu

SEED, CTR = 21, 5
ROWS = [1, 5, 9, 1027]          # the unroll's remainders and the 1,024-row LDS chunk


NUMELS = (3, 10, 1024, 4100, 4099)


def record(rows, numels=NUMELS, edit=None):
    """One record: [rows, numel] float32 per variable; the 4100 and 4099 ones views of a [rows, 4104]
    buffer (16-byte loads, the last workgroup ragged; 4099 also ends in a ragged group, which falls
    back to dwords), the 3 and 10 ones on dword loads with a tail."""
    rng = np.random.default_rng(rows)
    host = [rng.standard_normal((rows, n)).astype(np.float32) for n in numels]
    for h in host if edit else ():
        edit(h)
    devs = []
    for h in host:
        if h.shape[1] >= 4099:
            buf = torch.zeros(rows, 4104, device="cuda")
            buf[:, :h.shape[1]] = torch.from_numpy(h).cuda()
            devs.append(buf[:, :h.shape[1]])
        else:
            devs.append(torch.from_numpy(h).cuda())
    return host, devs


def normals(dp, host):
    """The kernel's normals at the stream positions dp_clip_sum_noise takes, per variable."""
    zs, ctr = [], CTR
    for h in host:
        zs.append(kernel_normals(dp, SEED, ctr, h.shape[1]))
        ctr += (h.shape[1] + 3) // 4
    return zs


def loop_sum(h, s):
    acc = np.zeros(h.shape[1], np.float32)
    for g, si in zip(h, s):
        acc = acc + g * si                      # float32 product, float32 addition
    return acc


def stream(dp):
    from efl.privacy.secret_sharing import NoiseStream
    return NoiseStream(SEED, CTR)


@pytest.mark.parametrize("rows,numels", [(r, NUMELS) for r in ROWS] + [(3, (5,) * 70)])
@pytest.mark.parametrize("mode,div", [(0, 256.0), (0, 3.0), (1, 256.0), (1, 3.0)])
def test_sum_is_exact_given_scales(dp, rows, numels, mode, div):
    host, devs = record(rows, numels)
    s = np.random.default_rng(rows).uniform(0.1, 1.0, rows).astype(np.float32)
    st = stream(dp)
    got = dp.dp_clip_sum_noise(devs, None, mode, 1.0, div, st, scales=torch.from_numpy(s).cuda())
    assert st.counter == CTR + sum((n + 3) // 4 for n in numels)
    for h, g, z in zip(host, got, normals(dp, host)):
        want = mask.dp_noise(loop_sum(h, s), SEED, 0, mode, 1.0, div, z=z)
        assert np.array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_no_clip_is_the_plain_sum(dp):
    host, devs = record(9)
    got = dp.dp_clip_sum_noise(devs, None, 0, 1.0, 9.0, stream(dp))
    for h, g, z in zip(host, got, normals(dp, host)):
        want = mask.dp_noise(loop_sum(h, np.ones(9, np.float32)), SEED, 0, 0, 1.0, 9.0, z=z)
        assert np.array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("clip", [0.5, 1.0, 3.0])
def test_scales_and_result_against_float64(dp, rows, clip):
    def edit(h):                                # row 0 unclipped; one all-zero row
        h[0] *= np.float32(1e-3)
        h[2:3] = 0
    host, devs = record(rows, edit=edit)
    sigma, div = clip * 1.1, float(rows)
    got, sc = dp.dp_clip_sum_noise(devs, clip, 1, sigma, div, stream(dp), return_scales=True)
    sc = sc.cpu().numpy()
    norm = np.sqrt(sum((h.astype(np.float64) ** 2).sum(axis=1) for h in host))
    with np.errstate(divide="ignore"):
        want = (clip * np.minimum(1.0 / norm, 1.0 / clip)).astype(np.float32)
    assert ulps(sc, want).max() <= 1
    assert sc[0] == 1.0 and (rows <= 2 or sc[2] == 1.0) and (rows < 2 or sc[1] < 1.0)
    for h, g, z in zip(host, got, normals(dp, host)):
        terms = h.astype(np.float64) * sc.astype(np.float64)[:, None]
        zs = z.astype(np.float64) * np.float32(sigma).astype(np.float64)
        ref = (terms.sum(axis=0) + zs) / div
        bound = (rows + 2) * 2.0 ** -24 * (np.abs(terms).sum(axis=0) + np.abs(zs)) / abs(div)
        assert (np.abs(g.cpu().numpy().astype(np.float64) - ref) <= bound).all()


@pytest.mark.parametrize("clip", [None, 2.0 ** 10, 1.0])
def test_optimizer_step_batched_against_loop(dp, clip):
    """test_dp_gpu.py's 6 x 4 model, four microbatches: equal updates where both paths' scales are
    exactly 1; with clip = 1 within the float64 bound above plus 4 ulp of scale (the loop rounds the
    norm, the reciprocal and the product in fp32). The batched gradients are efl_dp_clip_sum's: equal
    to a direct dp_clip_sum_noise over the stacked per-microbatch gradients."""
    import efl
    x = torch.randn(16, 6, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    out = {}
    for path in ("loop", "batched"):
        w = torch.linspace(-1, 1, 24, device="cuda").reshape(6, 4).requires_grad_()
        b = torch.zeros(4, device="cuda", requires_grad=True)
        efl.privacy.set_noise_seed(77, 0)
        opt = efl.privacy.DPGradientDescentGaussianOptimizer(noise_multiplier=1.1, l2_norm_clip=clip, num_microbatches=4,
                                                             learning_rate=0.5, microbatch_gradients=path)
        loss = torch.nn.functional.cross_entropy(x @ w + b, torch.arange(16, device="cuda") % 4, reduction="none")
        gv = opt.compute_gradients(loss, [w, b])
        rows = [torch.autograd.grad(r.sum(), [w, b], retain_graph=True) for r in loss.reshape(4, -1)]
        opt.apply_gradients(gv)
        out[path] = ([g.cpu().numpy().astype(np.float64) for g, _ in gv], [w.detach().cpu(), b.detach().cpu()],
                     dp.noise_stream().counter, rows)
    assert out["loop"][2] == out["batched"][2] == 6 + 1
    from efl.privacy.secret_sharing import NoiseStream
    stacked = [torch.stack([r[k] for r in out["batched"][3]]) for k in (0, 1)]
    mode, sigma = (0, 1.1) if clip is None else (1, clip * 1.1)
    direct = dp.dp_clip_sum_noise(stacked, clip, mode, sigma, 4.0, NoiseStream(77, 0))
    assert all(np.array_equal(d.cpu().numpy().astype(np.float64), g) for d, g in zip(direct, out["batched"][0]))
    if clip != 1.0:
        assert all(torch.equal(a, c) for a, c in zip(out["loop"][1], out["batched"][1]))
        return
    rows = out["loop"][3]
    norm = np.array([np.sqrt(sum((g.double() ** 2).sum().item() for g in r)) for r in rows])
    s = clip * np.minimum(1.0 / norm, 1.0 / clip)
    for k, ctr in ((0, 0), (1, 6)):
        terms = np.stack([r[k].double().cpu().numpy().reshape(-1) * si for r, si in zip(rows, s)])
        zs = np.abs(kernel_normals(dp, 77, ctr, terms.shape[1]).astype(np.float64)) * np.float32(clip * 1.1)
        mag = np.abs(terms).sum(axis=0)
        bound = ((4 + 2) * 2.0 ** -24 * (mag + zs) + 4 * 2.0 ** -23 * mag) / 4.0
        assert (np.abs(out["loop"][0][k].reshape(-1) - out["batched"][0][k].reshape(-1)) <= bound).all()


def test_custom_query_keeps_its_overrides(dp):
    """A subclass of a stock query (here a noise-free get_noised_result) is not fused: "batched"
    honours the override as "loop" does, and draws no noise."""
    class NoNoise(dp.GaussianSumQuery):
        def get_noised_result(self, sample_state, global_state, divisor=1.0):
            return [v / divisor for v in sample_state], global_state

    x = torch.randn(16, 6, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    dp.set_noise_seed(77, 0)
    got = {}
    for path in ("loop", "batched"):
        w = torch.linspace(-1, 1, 24, device="cuda").reshape(6, 4).requires_grad_()
        b = torch.zeros(4, device="cuda", requires_grad=True)
        opt = dp.DPGradientDescentOptimizer(NoNoise(1.0, 5.0), 4, params=[w, b], lr=0.5, microbatch_gradients=path)
        loss = torch.nn.functional.cross_entropy(x @ w + b, torch.arange(16, device="cuda") % 4, reduction="none")
        got[path] = [g for g, _ in opt.compute_gradients(loss, [w, b])]
    assert all(torch.equal(a, c) for a, c in zip(got["loop"], got["batched"]))
    assert dp.noise_stream().counter == 0
