"""exp2 renders without a GPU: the colour table, the numpy restatement tests/exp2_ref.py against the reference's captured outputs
(tests/golden/exp2_cases.npz, made by tests/golden/make_golden_exp2.py), the ABI, and the command line's flags."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import exp2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_NAMES = [c["name"] for c in exp2_ref.CASES]
ERRORS = {"FileNotFoundError": FileNotFoundError, "ValueError": ValueError, "TypeError": TypeError}


def golden_case(z, name):
    pre = name + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def check_events(events, want, rgba_tab):
    """events: dicts in exp2_ref's layout, against one fixture case: labels, frame counts and suptitles, every image panel's
    bytes at every pixel, the point list and the points' bytes."""
    assert len(events) == int(want["n_events"])
    for e, ev in enumerate(events):
        assert f"comparison_{ev['key']}.gif" == str(want[f"{e}/file"])
        assert ev["labels"] == json.loads(str(want[f"{e}/labels"]))
        sup = json.loads(str(want[f"{e}/suptitles"]))
        assert ev["frames"] == len(sup)
        assert [f"{ev['title']} | Frame {t + 1}/{ev['frames']}" for t in range(ev["frames"])] == sup
        rgba = want[f"{e}/rgba"]                                   # [n, P, S, S, 4]
        assert rgba.shape[:2] == (ev["frames"], len(ev["labels"]))
        for p, gauge in enumerate(ev["gauge"]):
            if gauge:                                              # imshow(zeros, cmap="gray"): opaque black under the discs
                assert np.array_equal(rgba[:, p], np.broadcast_to(np.array([0, 0, 0, 255], np.uint8), rgba[:, p].shape))
            else:
                assert np.array_equal(rgba_tab[ev["panels"][p]], rgba[:, p]), (ev["key"], ev["labels"][p])
        pts = np.asarray(ev["points"]).reshape(-1, 2)
        if f"{e}/pt_xy" in want:
            assert np.array_equal(pts[:, ::-1], want[f"{e}/pt_xy"])        # scatter takes (column, row); np.argwhere order
            assert np.array_equal(rgba_tab[ev["point_idx"]], want[f"{e}/pt_rgba"])
        else:
            assert pts.shape[0] == 0                               # the reference does not call scatter without a point


def check_ranges(range_lines, want):
    if "ranges" in want:
        assert "".join(line + "\n" for line in range_lines) == str(want["ranges"])


def test_fixture_matches_the_recipes(golden):
    z = golden("exp2_cases.npz")
    for c in exp2_ref.CASES:
        assert str(z[c["name"] + "/recipe"]) == exp2_ref.recipe_json(c), c["name"]
    assert float(z["margin"]) >= 1e-9


def test_paper_cmap_equals_the_reference_bit_for_bit(golden):
    from p2igan_bench.evaluation import EXP2_IDX_BAD, exp2_palette, paper_cmap
    z = golden("exp2_cases.npz")
    bounds, colors = paper_cmap()
    assert bounds.dtype == np.float64 and bounds.shape == (142,) and colors.shape == (141, 4)
    assert bounds.tobytes() == z["bounds"].tobytes()
    assert colors.tobytes() == z["colors"].tobytes()
    # the quirks: the coarse bounds 0.5 ... 16 are not among the fine ones; 20 white colours pad the 121 of the gradient
    assert not np.isin([0.5, 1, 2, 4, 8, 16], bounds).any() and bounds[0] == 0 and bounds[-1] == 200
    assert np.all(colors[121:, :3] == 1.0) and np.all(np.diff(bounds) > 0)
    assert np.array_equal(exp2_palette()[:EXP2_IDX_BAD], z["color_bytes"][:, :3])
    rb, rc = exp2_ref.cmap_tables()
    assert rb.tobytes() == bounds.tobytes() and rc.tobytes() == colors.tobytes()


@pytest.mark.parametrize("case", CASE_NAMES)
def test_restatement_reproduces_the_reference(golden, case):
    c = next(c for c in exp2_ref.CASES if c["name"] == case)
    want = golden_case(golden("exp2_cases.npz"), case)
    preds, truth, obs, mask, kw = exp2_ref.build_case(c)
    tab = exp2_ref.rgba_table()
    if "error" in want:
        with pytest.raises(ERRORS[str(want["error"])]):
            exp2_ref.exp2(preds, truth, obs, mask, **kw)
        # the events before the failing one were rendered by the reference: they must match too
        first = list(sorted(truth))[:int(want["n_events"])]
        res = exp2_ref.exp2({n: {k: p[k] for k in first} for n, p in preds.items()}, {k: truth[k] for k in first},
                            {k: obs[k] for k in first}, mask, **kw)
        check_events(res["events"], want, tab)
        assert "event_ranges.txt" not in json.loads(str(want["files"]))
        return
    res = exp2_ref.exp2(preds, truth, obs, mask, **kw)
    check_events(res["events"], want, tab)
    check_ranges([e["range_line"] for e in res["events"]], want)
    assert res["per_event"] == ("ranges" in want)
    assert [f"comparison_{e['key']}.gif" for e in res["events"] if e["frames"] > 0] == \
        [f for f in json.loads(str(want["files"])) if f.endswith(".gif")]


def test_fixture_covers_the_edge_cases(golden):
    z = golden("exp2_cases.npz")
    w = golden_case(z, "path_order")
    assert [str(w["0/file"]), str(w["1/file"])] == ["comparison_event_10.gif", "comparison_event_2.gif"]       # lexicographic
    assert len(json.loads(str(golden_case(z, "path_cap")["0/suptitles"]))) == 30
    s = golden_case(z, "path_shorten")
    assert str(s["ranges"]) == "event_01: frames 1-3 (count=3)\n" and len(json.loads(str(s["0/suptitles"]))) == 2
    assert json.loads(str(s["0/labels"]))[:2] == ["Gauge", "Radar"] and "0/pt_xy" not in s
    assert str(golden_case(z, "path_missing")["error"]) == "FileNotFoundError"
    assert len(json.loads(str(golden_case(z, "array_long")["0/suptitles"]))) == 31
    # NaN (transparent), the last colour (values clipped to 200) and the first are all among the reference's bytes
    rg = w["0/rgba"].reshape(-1, 4)
    assert (rg[:, 3] == 0).any() and (rg[:, :3] == 255).all(1).any()


def test_disc_rule_at_zoom_one():
    """One point: its pixel is the face, the 8 around it the edge ring; at a corner the ring is clipped by the panel.  This pins
    the arbiter (exp2_ref.compose) to the disc rule as DESIGN.md states it; it runs no product code: the kernel is held to the
    arbiter in tests/test_exp2_gpu.py."""
    panels = np.full((1, 1, 5, 5), 7, np.uint8)
    chrome = np.full((7, 16), 99, np.uint8)
    out = exp2_ref.compose(panels, 1, 1, [[2, 2], [0, 0]], chrome, 1, 1, 6, 50, 60)[0]
    want = np.full((5, 5), 50, np.uint8)
    want[1:4, 1:4] = 60
    want[2, 2] = 7
    want[0:2, 0:2] = 60          # the later point's ring paints over the earlier one's
    want[0, 0] = 7
    assert np.array_equal(out[1:6, 1:6], want)
    assert (out[0] == 99).all() and (out[:, 0] == 99).all() and (out[:, 6:] == 99).all() and (out[6] == 99).all()


def test_symbols_declared_and_bound():
    from p2igan_bench import _hip
    hdr = open(os.path.join(ROOT, "include", "p2i_hip.h")).read()
    for name, nargs in (("p2i_exp2_index", 9), ("p2i_exp2_compose", 18)):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(_hip.SIGNATURES[name])
    import ctypes
    lib = ctypes.CDLL(_hip.lib_path())
    assert hasattr(lib, "p2i_exp2_index") and hasattr(lib, "p2i_exp2_compose")
    mk = open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc", "Makefile")).read()
    assert "eval_exp2.hip" in mk and re.search(r"eval_exp2\.o: FLAGS \+= -ffp-contract=off", mk)


def test_gif_writer_keeps_the_palette_exactly(tmp_path):
    """The GIF holds the canvases' indices under the given palette: no quantisation, the right duration and frame count."""
    from PIL import Image
    from p2igan_bench.evaluation import exp2_palette, write_exp2_gif
    rng = np.random.default_rng(3)
    canv = rng.integers(0, 160, size=(3, 21, 37), dtype=np.uint8)
    pal = exp2_palette()
    path = str(tmp_path / "a.gif")
    write_exp2_gif(canv, pal, path, 4)
    with Image.open(path) as im:
        assert im.n_frames == 3 and im.info["loop"] == 0
        for t in range(3):
            im.seek(t)
            assert im.info["duration"] == 250
            assert np.array_equal(np.asarray(im.convert("RGB")), pal[canv[t]])


def test_exp2_has_no_cpu_path(monkeypatch):
    import torch
    from p2igan_bench.evaluation import compute_exp2
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    preds, truth, obs, mask, kw = exp2_ref.build_case(exp2_ref.CASES[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_exp2(preds, truth, obs, mask, **kw)


def test_evaluate_help_lists_the_exp2_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts", "evaluate.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--exp2", "--observation", "--gif-fps", "--exp2-pdf", "--exp2-events"):
        assert flag in r.stdout, flag
