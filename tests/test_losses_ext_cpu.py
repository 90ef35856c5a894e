"""The loss family of modules/losses.py without a GPU: the module's surface, the torch restatement (tests/losses_ext_ref.py)
against the genuine reference's float64 fixtures, the refusal of CPU tensors and k1_loss's identities."""
import inspect

import numpy as np
import pytest
import torch

import losses_ext_ref as R
from conftest import rel_err

REFERENCE_ALL = ["ReconstructionLoss", "gan_loss", "transform", "weighted_l1_distance", "softmax_temperature", "kl_divergence",
                 "compute_forward_difference", "spatial_pool", "temporal_difference_matching_loss", "shock_map", "shock_map_loss",
                 "k1_loss", "AdversarialLoss", "WeightedL1Metric", "K1LossMetric", "ShockDifferenceMetric"]


def test_all_is_the_references_name_list():
    from p2igan_bench.modules import losses
    assert losses.__all__ == REFERENCE_ALL
    for n in REFERENCE_ALL:
        assert hasattr(losses, n), n
    from p2igan_bench import modules
    assert modules.__all__ == ["ReconstructionLoss", "gan_loss"]


def test_signatures_and_defaults_are_the_references():
    from p2igan_bench.modules import losses as L

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != "self"]
    E = inspect.Parameter.empty
    assert sig(L.transform) == [("x", E)]
    assert sig(L.weighted_l1_distance) == [("x_pred", E), ("x_true", E)]
    assert sig(L.softmax_temperature) == [("tensor", E), ("temperature", E)]
    assert sig(L.kl_divergence) == [("p", E), ("q", E)]
    assert sig(L.compute_forward_difference) == [("series", E)]
    assert sig(L.spatial_pool) == [("x", E)]
    assert sig(L.temporal_difference_matching_loss) == [("pred_diff", E), ("true_diff", E), ("true", E), ("beta", 1.0), ("eps", 1e-6)]
    assert sig(L.shock_map) == [("x", E), ("beta", 30.0), ("eps", 1e-12)]
    assert sig(L.shock_map_loss) == [("pred", E), ("true", E), ("beta", 30.0), ("tau", 25.0), ("border_ignore", 0), ("pool", 2),
                                     ("eps", 1e-12)]
    assert sig(L.k1_loss) == [("pred", E), ("true", E), ("temp_alpha", E), ("k1_alpha", E)]
    assert sig(L.AdversarialLoss.__init__) == [("loss_type", "nsgan"), ("target_real_label", 1.0), ("target_fake_label", 0.0)]
    assert sig(L.AdversarialLoss.forward) == [("outputs", E), ("is_real", E), ("is_disc", None)]
    assert sig(L.WeightedL1Metric.__init__) == []
    assert sig(L.K1LossMetric.__init__) == [("temp_alpha", 1.0), ("k1_alpha", 0.0)]
    assert sig(L.ShockDifferenceMetric.__init__) == [("beta", 0.02), ("border_ignore", 2), ("pool", 1)]
    for cls in (L.WeightedL1Metric, L.K1LossMetric, L.ShockDifferenceMetric):
        for m in ("update", "compute", "reset", "to"):
            assert callable(getattr(cls, m))
    a = L.AdversarialLoss("hinge", 0.9, 0.1)
    assert sorted(n for n, _ in a.named_buffers()) == ["fake_label", "real_label"]
    assert float(a.real_label) == pytest.approx(0.9) and float(a.fake_label) == pytest.approx(0.1)
    with pytest.raises(ValueError):
        L.AdversarialLoss("wgan")
    with pytest.raises(ValueError):
        a(torch.zeros(2), True)


def test_restatement_equals_the_reference_in_float64(golden):
    g = golden("losses_ext.npz")
    cases = R.golden_cases(g)
    assert len(cases) == 7 + 2 + 8 + 4 + 3 + 3
    for tag, name, kw, inputs in cases:
        out, grad = R.value_and_grad(lambda *xs: getattr(R, name)(*xs, **kw), inputs, g[f"{tag}/g"], torch.float64)
        assert tuple(out.shape) == g[f"{tag}/out"].shape, tag
        assert rel_err(out.numpy(), g[f"{tag}/out"]) <= 1e-12, tag
        assert rel_err(grad.numpy(), g[f"{tag}/grad"]) <= 1e-12, tag


def test_fixture_is_small_and_holds_arrays_only(golden):
    import os
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "losses_ext.npz")) < 200 * 1024
    g = golden("losses_ext.npz")
    assert all(g[k].dtype in (np.float32, np.float64) for k in g.files)


def test_cpu_tensors_are_refused():
    from p2igan_bench.modules import losses as L
    x, y = torch.rand(1, 3, 6, 6), torch.rand(1, 3, 6, 6)
    calls = [lambda: L.transform(x), lambda: L.weighted_l1_distance(x, y), lambda: L.softmax_temperature(x, 0.1),
             lambda: L.kl_divergence(x, y), lambda: L.compute_forward_difference(x), lambda: L.spatial_pool(x),
             lambda: L.temporal_difference_matching_loss(x[:, :2], y[:, :2], y), lambda: L.shock_map(x),
             lambda: L.shock_map_loss(x, y), lambda: L.k1_loss(x, y, 1.0, 0.0), lambda: L.k1_loss(x, y, 0.0, 0.05),
             lambda: L.WeightedL1Metric().update(x, y), lambda: L.K1LossMetric().update(x, y),
             lambda: L.ShockDifferenceMetric().update(x, y)]
    for i, c in enumerate(calls):
        with pytest.raises(RuntimeError):
            c()
            pytest.fail(f"call {i} accepted CPU tensors")


def test_target_side_gradients_are_refused():
    from p2igan_bench.modules import losses as L
    x, y = torch.rand(1, 3, 6, 6), torch.rand(1, 3, 6, 6, requires_grad=True)
    for c in (lambda: L.weighted_l1_distance(x, y), lambda: L.kl_divergence(x, y), lambda: L.shock_map_loss(x, y),
              lambda: L.temporal_difference_matching_loss(x[:, :2], y[:, :2], x), lambda: L.temporal_difference_matching_loss(x[:, :2], x[:, :2], y),
              lambda: L.k1_loss(x, y, 1.0, 0.0)):
        with pytest.raises(RuntimeError, match="target side"):
            c()


def test_k1_loss_identities_on_the_restatement():
    """The reference's k1_loss never includes its shock term (it is computed only for temp_alpha == 0 and then multiplied by
    temp_alpha): k1_loss(p, t, 0, k) is ReconstructionLoss(k)'s loss and k1_loss(p, t, 1, 0) the weighted L1."""
    gen = torch.Generator().manual_seed(5)
    p, t = torch.rand(2, 4, 1, 8, 8, generator=gen, dtype=torch.float64), torch.rand(2, 4, 1, 8, 8, generator=gen, dtype=torch.float64)
    assert torch.equal(R.k1_loss(p, t, 0.0, 0.05), R.reconstruction_loss(p, t, 0.05))
    assert torch.equal(R.k1_loss(p, t, 1.0, 0.0), R.weighted_l1_distance(p, t))
    from p2igan_bench.modules import losses as L
    assert "shock" in L.k1_loss.__doc__
