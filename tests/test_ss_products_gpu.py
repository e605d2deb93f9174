"""GPU: efl_ss_products (csrc/ssgemm.hip), the fp32-MFMA kernel behind efl.secret_sharing.fused_products
and `product="fused"`.

(a) fused_products against float64 torch on the same N(0, 1) operands, on both workgroup tiles.
The bound is derived, not measured: n = sum K_t + count roundings of u = 2^-24 per output, doubled
for the MFMA's unspecified rounding inside its 2-long dot:
    |z^ - z| <= 2 n u / (1 - n u) * sum_t |A_t| @ |B_t|   elementwise, right-hand side in float64.
(b) the refusals. (c) the protocol through matmul / Dense with a party playing against itself
(its own masked tensors come back as the peer's), where mode C gives 2 a @ b, da = 2 dy @ b^T and
db = 2 a^T @ dy; the tolerance of tests/test_secret_sharing_gpu.py for the same shapes."""
import pytest
import torch

import efl

pytestmark = pytest.mark.gpu
ss = efl.secret_sharing
ONE = [(1, (1,), 1), (1, (2,), 1), (31, (3,), 33), (33, (17,), 65), (64, (16,), 64), (65, (35,), 31),
       (256, (392,), 10)]
MANY = [(33, (17, 0), 65), (65, (3, 16), 31), (33, (35, 0, 3, 17, 1), 65), (65, (35, 0, 3, 17, 1), 31)]


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("first", range(4))
@pytest.mark.parametrize("R,ks,N", ONE + MANY)
def test_fused_products(R, ks, N, first, tile):
    """Term i takes layout (first + i) % 4: plain, both operands transposed views, both column
    slices of wider tensors, B a row slice from an odd row. The last of several terms is negative.
    The result goes into a view with a wider row stride, twice, compared byte for byte."""
    g = torch.Generator().manual_seed(1000 * R + N)
    rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()
    terms = []
    for i, K in enumerate(ks):
        layout = (first + i) % 4
        if layout == 0:
            A, B = rnd(R, K), rnd(K, N)
        elif layout == 1:
            A, B = rnd(K, R).t(), rnd(N, K).t()
        elif layout == 2:
            A, B = rnd(R, K + 5)[:, 3:3 + K], rnd(K, N + 7)[:, 2:2 + N]
        else:
            A, B = rnd(R, K), rnd(K + 4, N)[3:3 + K]
        terms.append((A, B, -1 if 0 < i == len(ks) - 1 else 1))
    wide = torch.full((2, R, N + 3), 7.0, device="cuda")
    got = ss.fused_products(terms, out=wide[0, :, 1:1 + N], tile=tile)
    ss.fused_products(terms, out=wide[1, :, 1:1 + N], tile=tile)
    assert got.data_ptr() == wide[0, :, 1:].data_ptr() and torch.equal(wide[0], wide[1])
    assert bool((wide[:, :, 0] == 7).all()) and bool((wide[:, :, 1 + N:] == 7).all())   # the sentinel stays
    ref = sum(s * (A.double() @ B.double()) for A, B, s in terms)
    mag = sum(A.double().abs() @ B.double().abs() for A, B, s in terms)
    nu = (sum(ks) + len(ks)) * 2.0 ** -24
    err, bound = (got.double() - ref).abs(), 2 * nu / (1 - nu) * mag
    print("max |err| / bound:", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())


def test_refusals_and_empty():
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(4, 6, generator=g).cuda(), torch.randn(6, 5, generator=g).cuda()
    bad = efl.errors.InvalidArgumentError
    with pytest.raises(bad, match="at most 8"):
        ss.fused_products([(a, b)] * 9)
    with pytest.raises(bad, match="inner dimensions"):
        ss.fused_products([(a, b[:5])])
    with pytest.raises(bad, match="the result is"):
        ss.fused_products([(a, b), (a[:3], b)])
    with pytest.raises(bad, match="the result is"):
        ss.fused_products([(a, b), (a, b[:, :4])])
    with pytest.raises(bad, match="float32"):
        ss.fused_products([(a.double(), b.double())])
    with pytest.raises(bad, match="overlaps"):
        ss.fused_products([(a, b)], out=a[:, :5])
    with pytest.raises(ValueError, match="product"):
        ss.matmul(a, b, None, "m", ss.matmul.Mode.C, product="blas")
    assert ss.fused_products([(a[:0], b)]).shape == (0, 5)
    out = torch.full((4, 5), 7.0, device="cuda")
    assert not ss.fused_products([], out=out).any()                    # no terms: zeros
    out.fill_(7.0)
    assert not ss.fused_products([(a[:, :0], b[:0])], out=out).any()   # K = 0 alone: zeros


class Loopback:
    """A communicator whose peer is the caller: recv returns the tensor last sent under the name."""
    def __init__(self): self.sent = {}
    def result(self): return None
    def recv(self, name, shape=None, dtype=None): return self.sent[name]
    def send(self, name, t):
        self.sent[name] = t.detach().clone()
        return self


@pytest.mark.parametrize("product", ["fused", "library"])
@pytest.mark.parametrize("combine", [False, True])
def test_mode_c_against_itself(combine, product):
    g = torch.Generator().manual_seed(1)
    a, b, dy = (torch.randn(s, generator=g).cuda() for s in ((8, 6), (6, 4), (8, 4)))
    a.requires_grad_(), b.requires_grad_()
    z = ss.matmul(a, b, Loopback(), "m", ss.matmul.Mode.C, combine_gradients=combine, product=product)
    z.backward(dy)
    ad, bd, dyd = a.detach().double(), b.detach().double(), dy.double()
    tol = dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(z.detach().double(), 2 * ad @ bd, **tol)
    torch.testing.assert_close(a.grad.double(), 2 * dyd @ bd.t(), **tol)
    torch.testing.assert_close(b.grad.double(), 2 * ad.t() @ dyd, **tol)


@pytest.mark.parametrize("product", ["fused", "library"])
def test_dense_against_itself(product):
    g = torch.Generator().manual_seed(2)
    x, w, dy = (torch.randn(s, generator=g).cuda() for s in ((8, 6), (6, 4), (8, 4)))
    x.requires_grad_()
    layer = ss.Dense(Loopback(), "d", 4, kernel_initializer=lambda t: t.copy_(w), product=product)
    y = layer(x)
    y.backward(dy)
    tol = dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(y.detach().double(), 2 * x.detach().double() @ w.double(), **tol)
    torch.testing.assert_close(x.grad.double(), 2 * dy.double() @ w.double().t(), **tol)
    torch.testing.assert_close(layer.kernel.grad.double(), 2 * x.detach().double().t() @ dy.double(), **tol)
