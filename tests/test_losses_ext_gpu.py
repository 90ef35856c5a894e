"""The loss family of modules/losses.py on the GPU (csrc/loss_ext.hip) against the genuine reference's float64 fixtures
(tests/golden/losses_ext.npz) and, where the fixture has no case, the torch restatement tests/losses_ext_ref.py in float64.

Tolerances are the project's (test_stdk_gpu.py): values within 1e-4 and gradients within 1e-3 of the
expected array's max-abs.  The reference's own float32-vs-float64 distance on these cases is <= 2e-6 (values) and <= 3e-6
(gradients), and every fixture case passed a 1e-5 float32 / float64 gate, so none sits on a relu / abs / argmax kink.

The extra shock case is a 17 x 67 map: the kernel's tile is 32 wide and 8 tall, so the map spans 3 x 3 tiles and is a multiple of
neither extent (fixture case shock_loss/6)."""
import numpy as np
import pytest
import torch

import losses_ext_ref as R
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
GTOL = 1e-3

_G = np.load(f"{GOLDEN}/losses_ext.npz")
CASES = {tag: (name, kw, inputs) for tag, name, kw, inputs in R.golden_cases(_G)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import _hip
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from p2igan_bench.modules import losses
    return losses


def _run(fn, inputs, g, dev):
    out, grad = R.value_and_grad(fn, inputs, g, torch.float32, dev)
    return out.cpu(), grad.cpu()


def _check(tag, out, grad, want_out, want_grad):
    ev, eg = rel_err(out, want_out), rel_err(grad, want_grad)
    print(f"{tag}: value {ev:.2e} gradient {eg:.2e}")
    assert tuple(out.shape) == tuple(np.shape(want_out)), tag
    assert ev <= TOL, (tag, ev)
    assert eg <= GTOL, (tag, eg)


@pytest.mark.parametrize("tag", list(CASES))
def test_matches_the_reference_and_is_deterministic(dev, L, tag):
    name, kw, inputs = CASES[tag]
    fn = lambda *xs: getattr(L, name)(*xs, **kw)           # noqa: E731
    out, grad = _run(fn, inputs, _G[f"{tag}/g"], dev)
    _check(tag, out.numpy(), grad.numpy(), _G[f"{tag}/out"], _G[f"{tag}/grad"])
    out2, grad2 = _run(fn, inputs, _G[f"{tag}/g"], dev)
    assert torch.equal(out, out2) and torch.equal(grad, grad2), f"{tag}: two runs differ"


def test_two_by_two_map(dev, L):
    """A 2 x 2 map under reflect padding has gx = gy = 0 everywhere, so |s| <= sqrt(eps) = 1e-6 and the loss is a difference of
    two such numbers: only its range is checked, and that the gradient is finite."""
    gen = torch.Generator().manual_seed(3)
    for shape, pool in (((1, 1, 2, 2), 1), ((1, 2, 4, 5), 2)):
        p = torch.rand(shape, generator=gen).to(dev).requires_grad_(True)
        t = torch.rand(shape, generator=gen).to(dev)
        out = L.shock_map_loss(p, t, beta=30.0, pool=pool)
        assert tuple(out.shape) == (shape[0], shape[1], 2, 2)
        o = out.detach()
        assert bool(torch.isfinite(o).all()) and float(o.min()) >= 0.0 and float(o.max()) <= 1.0001e-6
        out.sum().backward()
        assert bool(torch.isfinite(p.grad).all())


def test_shock_input_checks(dev, L):
    x = torch.rand(1, 2, 3, 8, device=dev)
    with pytest.raises(RuntimeError):
        L.shock_map_loss(x, x, pool=2)                       # pooled height 1
    with pytest.raises(RuntimeError):
        L.shock_map(torch.rand(1, 2, 1, 8, device=dev))
    with pytest.raises(RuntimeError):
        L.shock_map(torch.rand(2, 3, 8, device=dev))         # 4-D only
    with pytest.raises(RuntimeError):
        L.shock_map_loss(torch.rand(1, 2, 1, 8, 8, device=dev), torch.rand(1, 2, 1, 8, 8, device=dev))
    y = torch.rand(1, 2, 6, 8, device=dev)
    with pytest.raises(ValueError):
        L.shock_map_loss(y, y, pool=1, border_ignore=3)      # 6 - 2*3 rows left
    with pytest.raises(ValueError):
        L.shock_map_loss(y, y, pool=2, border_ignore=2)      # pooled 3 x 4
    assert tuple(L.shock_map_loss(y, y, pool=2, border_ignore=1).shape) == (1, 2, 1, 2)
    with pytest.raises(RuntimeError, match="target side"):
        L.shock_map_loss(y, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        L.spatial_pool(torch.rand(8, 8, device=dev))         # 3-D or 4-D


def test_pool_ties_go_to_the_first_maximum(dev, L):
    x = torch.ones(1, 1, 5, 5, device=dev, requires_grad=True)
    y = L.spatial_pool(x)
    assert tuple(y.shape) == (1, 1, 2, 2) and bool((y == 1).all())
    y.sum().backward()
    want = torch.zeros(5, 5)
    for i, j in ((0, 0), (0, 2), (2, 0), (2, 2)):
        want[i, j] = 1.0
    assert torch.equal(x.grad[0, 0].cpu(), want)
    # the same rule through the fused matching loss: with P(true_diff) = 0 and base = 0 the gradient is 2 / 4 at those pixels
    pd = torch.ones(1, 1, 5, 5, device=dev, requires_grad=True)
    L.temporal_difference_matching_loss(pd, torch.zeros(1, 1, 5, 5, device=dev), torch.zeros(1, 2, 5, 5, device=dev), eps=0.0).backward()
    assert torch.equal(pd.grad[0, 0].cpu(), want * 0.5)
    # and through the shock loss's pool: windows of equal values pass their gradient to the top-left element only
    gen = torch.Generator().manual_seed(4)
    p = torch.rand(1, 1, 4, 5, generator=gen).repeat_interleave(2, 2).repeat_interleave(2, 3).to(dev).requires_grad_(True)
    t = torch.rand(1, 1, 8, 10, generator=gen).to(dev)
    L.shock_map_loss(p, t, beta=1.0, pool=2).sum().backward()
    g = p.grad.cpu()
    assert float(g[..., ::2, ::2].abs().max()) > 0
    assert float(g[..., 1::2, :].abs().max()) == 0 and float(g[..., :, 1::2].abs().max()) == 0


def test_spatial_pool_three_dims_and_negative_planes(dev, L):
    gen = torch.Generator().manual_seed(6)
    x = (torch.randn(3, 10, 7, generator=gen) - 3.0).to(dev)           # all negative: a zero-padded pool would return zeros
    want = R.spatial_pool(x.double())
    assert float(want.max()) < 0
    assert torch.equal(L.spatial_pool(x).double(), want)


@pytest.mark.parametrize("name,shapes", [
    ("transform", [(8, 16, 72, 64)]), ("weighted_l1_distance", [(8, 16, 72, 64)] * 2), ("compute_forward_difference", [(8, 16, 72, 64)]),
    ("compute_forward_difference", [(3, 5, 7, 4)]), ("kl_divergence", [(8, 15, 72, 64)] * 2), ("softmax_temperature", [(8, 15, 72, 64)]),
    ("spatial_pool", [(4, 5, 70, 66)]), ("temporal_difference_matching_loss", [(4, 5, 70, 66), (4, 5, 70, 66), (4, 6, 70, 66)])])
def test_larger_shapes_match_the_restatement(dev, L, name, shapes):
    """Sizes at which the vectorised path and more than one workgroup per reduction run; the expected values are the float64
    restatement on the same float32 inputs.  Only the reductions' loops, whose grids are sized for four trips, go round again
    here: the largest tensor has 589,824 floats and one trip of the element-wise kernels covers 4,194,304 (1,048,576 on the
    scalar path), of the pool kernels 2,097,152 and of tdm_fwd 131,072 positions.  test_loss_ext_edges_gpu.py has those sizes."""
    gen = torch.Generator().manual_seed(len(name))
    if name == "kl_divergence":
        inputs = [R.softmax_temperature(0.2 * torch.randn(s, generator=gen, dtype=torch.float64), R.TEMP).float().numpy() for s in shapes]
    elif name in ("transform", "weighted_l1_distance"):
        inputs = [torch.rand(s, generator=gen).numpy() for s in shapes]
    else:
        inputs = [(0.4 * torch.randn(s, generator=gen)).numpy() for s in shapes]
    kw = dict(temperature=R.TEMP) if name == "softmax_temperature" else {}
    probe = R.value_and_grad(lambda *xs: getattr(R, name)(*xs, **kw), inputs, np.float32(1.0), torch.float64, dev)[0]
    g = torch.randn(tuple(probe.shape), generator=gen).numpy()
    want_out, want_grad = R.value_and_grad(lambda *xs: getattr(R, name)(*xs, **kw), inputs, g, torch.float64, dev)
    out, grad = _run(lambda *xs: getattr(L, name)(*xs, **kw), inputs, g, dev)
    _check(name, out.numpy(), grad.numpy(), want_out.cpu().numpy(), want_grad.cpu().numpy())
    out2, grad2 = _run(lambda *xs: getattr(L, name)(*xs, **kw), inputs, g, dev)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)


def test_softmax_of_large_inputs_is_finite(dev, L):
    x = torch.as_tensor(_G["softmax/3/x"]).to(dev)
    assert float(x.abs().max()) / R.TEMP > 89.0                  # exp would overflow in float32 without the max subtraction
    y = L.softmax_temperature(x, R.TEMP)
    assert bool(torch.isfinite(y).all())
    assert rel_err(y.sum(dim=(2, 3, 4)).cpu().numpy(), np.ones((2, 3))) <= 1e-5


def test_pieces_compose_to_the_reconstruction_loss_reg(dev, L):
    gen = torch.Generator().manual_seed(8)
    pred = torch.rand(2, 4, 1, 8, 8, generator=gen).to(dev).requires_grad_(True)
    true = torch.rand(2, 4, 1, 8, 8, generator=gen).to(dev)
    reg = L.kl_divergence(L.softmax_temperature(L.compute_forward_difference(pred), 0.1),
                          L.softmax_temperature(L.compute_forward_difference(true), 0.1))
    _, parts = L.ReconstructionLoss(0.05)(pred.detach(), true)
    assert abs(float(reg) - float(parts["reg"])) <= 1e-4 * abs(float(parts["reg"]))
    reg.backward()
    p64 = pred.detach().double().requires_grad_(True)
    R.kl_divergence(R.softmax_temperature(R.compute_forward_difference(p64), 0.1),
                    R.softmax_temperature(R.compute_forward_difference(true.double()), 0.1)).backward()
    assert rel_err(pred.grad.cpu().numpy(), p64.grad.cpu().numpy()) <= GTOL


def test_k1_loss_identities(dev, L):
    gen = torch.Generator().manual_seed(9)
    p, t = torch.rand(2, 4, 1, 8, 8, generator=gen).to(dev), torch.rand(2, 4, 1, 8, 8, generator=gen).to(dev)
    assert torch.equal(L.k1_loss(p, t, 0.0, 0.05), L.ReconstructionLoss(0.05)(p, t)[0])
    assert torch.equal(L.k1_loss(p, t, 1.0, 0.0), L.weighted_l1_distance(p, t))
    assert torch.equal(L.k1_loss(p, t, 0.0, 0.0), L.weighted_l1_distance(p, t))
    q = p.clone().requires_grad_(True)
    L.k1_loss(q, t, 1.0, 0.05).backward()
    q64 = p.double().requires_grad_(True)
    R.k1_loss(q64, t.double(), 1.0, 0.05).backward()
    assert rel_err(q.grad.cpu().numpy(), q64.grad.cpu().numpy()) <= GTOL


def test_metric_classes(dev, L):
    gen = torch.Generator().manual_seed(10)
    a = [torch.rand(2, 3, 9, 11, generator=gen).to(dev) for _ in range(4)]
    for m, fn in ((L.WeightedL1Metric(), L.weighted_l1_distance), (L.K1LossMetric(1.0, 0.05), lambda p, t: L.k1_loss(p, t, 1.0, 0.05)),
                  (L.K1LossMetric(), lambda p, t: L.k1_loss(p, t, 1.0, 0.0)),
                  (L.ShockDifferenceMetric(), lambda p, t: L.shock_map_loss(p, t, beta=0.02, border_ignore=2, pool=1).mean())):
        assert m.to(dev) is m
        assert float(m.compute()) == 0.0
        m.update(a[0], a[1])
        m.update(a[2], a[3])
        got = m.compute()
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dim() == 0
        want = 0.5 * (float(fn(a[0], a[1])) + float(fn(a[2], a[3])))
        assert abs(float(got) - want) <= 1e-6 * abs(want), type(m).__name__
        m.reset()
        assert float(m.loss_sum) == 0.0 and float(m.n_obs) == 0.0 and float(m.compute()) == 0.0
    lazy = L.WeightedL1Metric()                                # no .to(): the state follows the first update
    lazy.update(a[0], a[1])
    assert torch.equal(lazy.compute(), L.weighted_l1_distance(a[0], a[1]))


def test_adversarial_loss_module(dev, L):
    gen = torch.Generator().manual_seed(11)
    x = torch.rand(2, 1, 4, 6, 6, generator=gen).to(dev)       # inside [0, 1]: valid for nsgan's BCELoss too
    for loss_type in ("nsgan", "lsgan", "hinge"):
        mod = L.AdversarialLoss(loss_type, 0.9, 0.1).to(dev)
        assert mod.real_label.is_cuda
        for is_real in (True, False):
            for is_disc in (True, False):
                want = L.gan_loss(x, is_real, loss_type=loss_type, is_disc=is_disc, target_real_label=0.9, target_fake_label=0.1)
                assert torch.equal(mod(x, is_real, is_disc), want)
    assert torch.equal(L.AdversarialLoss("lsgan")(x, True), L.gan_loss(x, True, loss_type="lsgan"))
    with pytest.raises(ValueError):
        L.AdversarialLoss("hinge")(x, True)
    with pytest.raises(ValueError):
        L.AdversarialLoss("wgan")
