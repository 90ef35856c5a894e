"""STDK baseline on CPU: construction API, state-dict surface, seed-for-seed initialisation and the host knot tables against
tests/golden/stdk_32.npz (captured from the reference by tests/golden/make_golden_stdk.py)."""
import numpy as np
import pytest
import torch

CFG = {"model": {"name": "stdk", "in_channels": 1}, "data": {"train": {"h": 32, "w": 32, "sample_length": 16}}}


def test_build_generator_returns_stdk_with_reference_keys(golden):
    from p2igan_bench.models import build_generator
    from p2igan_bench.models.stdk import STDKGenerator
    g = golden("stdk_32.npz")
    G = build_generator(CFG)
    assert isinstance(G, STDKGenerator)
    sd = G.state_dict()
    names = sorted(k[len("init/"):-len("/shape")] for k in g.files if k.startswith("init/") and k.endswith("/shape"))
    assert sorted(sd) == names
    for n in names:
        assert list(sd[n].shape) == list(g[f"init/{n}/shape"]), n
    assert tuple(sd["_mlp.net.0.weight"].shape) == (100, 139 + 44 + 79 * 16)
    # data_loader.sample_length wins over data.train (reference models/__init__.py:33-36)
    G8 = build_generator(dict(CFG, data_loader={"sample_length": 8}))
    assert tuple(G8.state_dict()["_mlp.net.0.weight"].shape) == (100, 139 + 28 + 79 * 8)


def test_init_matches_reference_seed_for_seed(golden):
    from p2igan_bench.models import build_generator
    g = golden("stdk_32.npz")
    torch.manual_seed(2024)
    sd = build_generator(CFG).state_dict()
    for n, v in sd.items():
        v = v.double()
        s, a = g[f"init/{n}/sums"]
        assert abs(float(v.sum()) - s) <= 1e-6 * max(1.0, a), n
        assert abs(float(v.abs().sum()) - a) <= 1e-6 * max(1.0, a), n
        head = v.reshape(-1)[:64].float().numpy()
        np.testing.assert_allclose(head, g[f"init/{n}/head"], rtol=1e-6, atol=1e-7, err_msg=n)


@pytest.mark.parametrize("hw", [(32, 32), (32, 48), (128, 128), (256, 256)])
def test_space_knot_tables_equal_reference(golden, hw):
    from p2igan_bench.models.stdk import space_knots
    g = golden("stdk_32.npz")
    kn, th = space_knots(*hw)
    key = f"{hw[0]}x{hw[1]}"
    assert np.array_equal(kn.numpy(), g[f"knots_s/{key}"]) and np.array_equal(th.numpy(), g[f"theta_s/{key}"])
    assert kn.shape[0] == 139


@pytest.mark.parametrize("t", [8, 16, 32])
def test_time_knot_tables_equal_reference(golden, t):
    from p2igan_bench.models.stdk import time_knots
    g = golden("stdk_32.npz")
    kn, th = time_knots(t)
    assert np.array_equal(kn[:, :1].numpy(), g[f"knots_t/{t}"]) and not kn[:, 1].any()
    assert np.array_equal(th.numpy(), g[f"theta_t/{t}"])
    assert kn.shape[0] == {8: 28, 16: 44, 32: 60}[t]


def test_seeded_state_loads_strictly():
    from p2igan_bench.models import build_generator
    from p2igan_bench.utils import seeded
    for t in (8, 16):
        G = build_generator(dict(CFG, data={"train": {"h": 32, "w": 32, "sample_length": t}}))
        G.load_state_dict(seeded.seeded_stdk_state(t), strict=True)


def test_frames_smaller_than_79_pixels_raise():
    from p2igan_bench.models import build_generator
    G = build_generator(dict(CFG, data={"train": {"h": 8, "w": 8, "sample_length": 16}}))
    x = torch.zeros(1, 16, 1, 8, 8)
    with pytest.raises(ValueError):
        G(x, x)


def test_dk_and_simple_stay_refused():
    from p2igan_bench.models import build_generator
    for name in ("dk", "simple"):
        with pytest.raises(NotImplementedError):
            build_generator({"model": {"name": name}, "data": {"train": {"h": 32, "w": 32}}})


def test_shipped_config_has_reference_keys():
    import json
    import os
    from conftest import ROOT
    cfg = json.load(open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "p2igan_bench", "config", "stdk_baseline.json")))
    assert cfg["model"]["name"] == "stdk" and cfg["loss"]["use_gan"] == 0 and cfg["loss"]["k1_weight"] == 0.0005
    assert cfg["data"]["train"]["data_root"].startswith("synthetic://")
