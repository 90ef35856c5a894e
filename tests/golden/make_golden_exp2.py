#!/usr/bin/env python3
"""Generate tests/golden/exp2_cases.npz by running the GENUINE reference's experiments.exp2.run_exp2 on CPU.

Run where a checkout of the reference is at hand:  python tests/golden/make_golden_exp2.py REFERENCE_ROOT
(needs matplotlib and PIL, which the reference's exp2 imports).  The inputs are rebuilt from the recipes in tests/exp2_ref.py
(numpy-only generators of p2igan_bench.utils.seeded), so the fixture holds recipe parameters and the reference's outputs only.
Two shims, both here: a stub ``zarr`` module over p2igan_bench.data.zarr_lite, so that the path form runs without the zarr
package, and ``FigureCanvasAgg.tostring_rgb`` restored from ``buffer_rgba`` (matplotlib 3.10 removed it).

While run_exp2 runs, these are observed: the bounds and colours of ``_build_paper_cmap``; the array given to every
``Axes.imshow`` and the offsets and ``c=`` of every ``Axes.scatter``, each stored as the bytes ``cmap(norm(a), bytes=True)`` of
the reference's own cmap / norm objects (NaN masked first, as imshow and scatter do themselves); the panel titles, the suptitle of
every frame and the frame count; event_ranges.txt and the file names.  Layout:
    bounds, colors, color_bytes
    <case>/recipe (JSON), <case>/files (JSON list), <case>/ranges (the text; path form), <case>/error (``Type``),
    <case>/n_events, <case>/<e>/labels (JSON), <case>/<e>/suptitles (JSON), <case>/<e>/rgba [n, P, S, S, 4],
    <case>/<e>/pt_xy [K, 2] (x, y), <case>/<e>/pt_rgba [n, K, 4]
margin: the smallest relative distance of an f32 / f64 input's transformed value, before the final clip to [0, 200], to a bound
(asserted >= 1e-9: the device pow is a few ulp from numpy's, so equal indices are only fair away from the bounds; a value the
clip puts on 0 or 200 is the same constant on both sides, and uint8 inputs go through numpy's own table on the device).
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) != 2:
    sys.exit("usage: make_golden_exp2.py REFERENCE_ROOT")
REF = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exp2_ref  # noqa: E402
from p2igan_bench.data import zarr_lite  # noqa: E402

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import matplotlib.axes  # noqa: E402
import matplotlib.figure  # noqa: E402
from matplotlib.backends.backend_agg import FigureCanvasAgg  # noqa: E402
from matplotlib.colors import Normalize  # noqa: E402

if not hasattr(FigureCanvasAgg, "tostring_rgb"):
    FigureCanvasAgg.tostring_rgb = lambda self: np.asarray(self.buffer_rgba())[..., :3].tobytes()


class _ZarrGroup:
    """What the reference asks of ``zarr.open(path, mode="r")``: group_keys (none: the events are arrays), keys, in, []."""

    def __init__(self, path):
        self.g = zarr_lite.Group(path, "r")

    def group_keys(self):
        return []

    def keys(self):
        return self.g.keys()

    def __contains__(self, k):
        return k in self.g.keys()

    def __getitem__(self, k):
        return self.g[k][:]


sys.modules["zarr"] = types.SimpleNamespace(open=lambda path, mode="r": _ZarrGroup(path))

sys.path.insert(0, REF)
import experiments.exp2 as ref_exp2  # noqa: E402

LOG = {}


def _bytes(a, k):
    a = np.ma.masked_invalid(np.asarray(a, dtype=np.float64))
    cmap, norm = k.get("cmap"), k.get("norm")
    if isinstance(cmap, str):
        return matplotlib.colormaps[cmap](Normalize(k["vmin"], k["vmax"])(a), bytes=True)
    return cmap(norm(a), bytes=True)


def _observe():
    ax = matplotlib.axes.Axes
    o_imshow, o_scatter, o_title, o_sup = ax.imshow, ax.scatter, ax.set_title, matplotlib.figure.Figure.suptitle
    o_save = ref_exp2._save_combo_gif

    def imshow(self, a, *args, **k):
        LOG["frame"].append(("im", _bytes(a, k)))
        return o_imshow(self, a, *args, **k)

    def scatter(self, x, y, *args, **k):
        LOG["frame"].append(("pt", np.stack([np.asarray(x), np.asarray(y)], 1).astype(np.int64), _bytes(k["c"], k)))
        return o_scatter(self, x, y, *args, **k)

    def set_title(self, label, *args, **k):
        LOG["titles"].append(label)
        return o_title(self, label, *args, **k)

    def suptitle(self, t, *args, **k):
        # the last call of a frame: close it
        ev = LOG["events"][-1]
        ev["suptitles"].append(t)
        ev["frames"].append(LOG["frame"])
        ev["labels"] = LOG["titles"]
        LOG["frame"], LOG["titles"] = [], []
        return o_sup(self, t, *args, **k)

    def save(frames_map, out_path, *args, **k):
        LOG["events"].append({"suptitles": [], "frames": [], "labels": [], "path": os.path.basename(out_path)})
        LOG["frame"], LOG["titles"] = [], []
        return o_save(frames_map, out_path, *args, **k)

    ax.imshow, ax.scatter, ax.set_title, matplotlib.figure.Figure.suptitle = imshow, scatter, set_title, suptitle
    ref_exp2._save_combo_gif = save


def margin(arrays):
    bounds = exp2_ref.cmap_tables()[0]
    worst = np.inf
    for a in arrays:
        a = np.asarray(a)
        if a.dtype == np.uint8:
            continue
        x = np.maximum(a.astype(np.float64), 0.001) / 3.0
        v = 10 ** np.minimum(x * 0.0625, 38.0) * 0.036          # before the clip to [0, 200]
        v = v[np.isfinite(v)]
        if v.size:
            worst = min(worst, float(np.min(np.abs(v[:, None] - bounds[None, :]) / np.maximum(bounds[None, :], v[:, None]))))
    return worst


def main():
    _observe()
    cmap, norm, fine = ref_exp2._build_paper_cmap()
    out = {"bounds": np.asarray(fine, np.float64), "colors": np.asarray(cmap(np.arange(cmap.N)), np.float64),
           "color_bytes": cmap(np.arange(cmap.N), bytes=True)}
    worst = np.inf
    for c in exp2_ref.CASES:
        name = c["name"]
        preds, truth, obs, mask, kw = exp2_ref.build_case(c)
        out[f"{name}/recipe"] = np.array(exp2_ref.recipe_json(c))
        flat = []
        for src in list(preds.values()) + [truth, obs]:
            flat += list(src.values()) if isinstance(src, dict) else [src]
        worst = min(worst, margin(flat))
        LOG.clear()
        LOG.update(events=[], frame=[], titles=[])
        with tempfile.TemporaryDirectory() as td:
            od = os.path.join(td, "out")
            os.makedirs(od)
            if c["form"] == "path":
                preds, truth, obs = exp2_ref.write_zarrs(td, preds, truth, obs)
            try:
                ref_exp2.run_exp2(preds, truth, obs, mask, od, kw["crop_size"], None, 0.0, 0.0, 4, True, kw["mode"])
            except Exception as e:          # recorded: the device path must raise the same type
                out[f"{name}/error"] = np.array(type(e).__name__)
                print(name, "raises", type(e).__name__, e)
            files = sorted(os.listdir(od))
            out[f"{name}/files"] = np.array(json.dumps(files))
            if "event_ranges.txt" in files:
                out[f"{name}/ranges"] = np.array(open(os.path.join(od, "event_ranges.txt")).read())
        out[f"{name}/n_events"] = np.int64(len(LOG["events"]))
        for e, ev in enumerate(LOG["events"]):
            n = len(ev["frames"])
            labels = ev["labels"]
            out[f"{name}/{e}/labels"] = np.array(json.dumps(labels))
            out[f"{name}/{e}/suptitles"] = np.array(json.dumps(ev["suptitles"]))
            out[f"{name}/{e}/file"] = np.array(ev["path"])
            ims = [[x[1] for x in fr if x[0] == "im"] for fr in ev["frames"]]
            assert all(len(i) == len(labels) for i in ims), (name, e)
            out[f"{name}/{e}/rgba"] = np.asarray(ims, np.uint8)
            pts = [[x for x in fr if x[0] == "pt"] for fr in ev["frames"]]
            if pts and pts[0]:
                assert all(len(p) == 1 and np.array_equal(p[0][1], pts[0][0][1]) for p in pts), (name, e)
                out[f"{name}/{e}/pt_xy"] = pts[0][0][1]
                out[f"{name}/{e}/pt_rgba"] = np.asarray([p[0][2] for p in pts], np.uint8)
            print(name, e, ev["path"], labels, "frames", n)
    assert worst >= 1e-9, f"an input sits {worst:.3e} (relative) from a colour bound: change the recipe"
    out["margin"] = np.float64(worst)
    path = os.path.join(ROOT, "tests", "golden", "exp2_cases.npz")
    np.savez_compressed(path, **out)
    print("margin", worst, "wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
