"""exp2 renders on the MI355X (csrc/eval_exp2.hip through p2igan_bench.evaluation): the reference's captured outputs from
tests/golden/exp2_cases.npz, the compose kernel against the numpy restatement tests/exp2_ref.py byte for byte, the GIF read back,
determinism, input forms, scripts/evaluate.py --exp2 end to end, and the paper grid."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exp2_ref
from test_exp2_cpu import CASE_NAMES, ERRORS, check_events, check_ranges, golden_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_ref_layout(res):
    return [{"key": e.key, "title": e.title, "labels": e.labels, "gauge": e.gauge, "panels": e.panels, "points": e.points,
             "point_idx": e.point_idx, "frames": e.frames, "total": e.total, "range_line": e.range_line} for e in res.events]


def same_events(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ("key", "title", "labels", "gauge", "frames", "total", "range_line"):
            assert x[k] == y[k], k
        for k in ("panels", "points", "point_idx"):
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k


@pytest.mark.parametrize("case", CASE_NAMES)
def test_golden_case_on_device(golden, case, tmp_path):
    from p2igan_bench.evaluation import Exp2Result, run_exp2
    c = next(c for c in exp2_ref.CASES if c["name"] == case)
    want = golden_case(golden("exp2_cases.npz"), case)
    preds, truth, obs, mask, kw = exp2_ref.build_case(c)
    if c["form"] == "path":
        preds, truth, obs = exp2_ref.write_zarrs(tmp_path, preds, truth, obs)
    out = tmp_path / "out"
    args = (preds, truth, obs, mask, str(out), kw["crop_size"], None, 0.0, 0.0, 4)
    files = json.loads(str(want["files"]))
    if "error" in want:
        with pytest.raises(ERRORS[str(want["error"])]):
            run_exp2(*args, mode=kw["mode"], zoom=2)
        assert sorted(os.listdir(out)) == files                 # the events before the failing one, no event_ranges.txt
        return
    run_exp2(*args, mode=kw["mode"], zoom=2)
    assert sorted(os.listdir(out)) == sorted(files + ["exp2_data.npz"])
    res = Exp2Result.load(str(out / "exp2_data.npz"))
    check_events(as_ref_layout(res), want, exp2_ref.rgba_table())
    check_ranges(res.range_lines, want)
    if "ranges" in want:
        assert (out / "event_ranges.txt").read_text() == str(want["ranges"])
    assert res.bounds.tobytes() == golden("exp2_cases.npz")["bounds"].tobytes()


def test_index_kernel_matches_restatement_at_128():
    """uint8 (exact through the table), f32 and f64 inputs with NaN, negatives and values past the scale, crop 128 of 160 x 144:
    equal indices wherever the restatement's value is at least 1e-9 (relative) from a bound (the device pow is a few ulp off)."""
    from p2igan_bench import ops
    from p2igan_bench.evaluation import crop_origin, paper_cmap, truth_lut
    from p2igan_bench.utils import seeded
    dev = torch.device("cuda")
    bounds = paper_cmap()[0]
    bd, lut = torch.from_numpy(bounds).to(dev), torch.from_numpy(truth_lut(True)).to(dev)
    base = seeded.exp1_truth(77, 5, 160, 144)
    tl = crop_origin(160, 144, 128)
    for kind in ("u8", "f32", "f64"):
        x = base[:, 0] if kind == "u8" else exp2_ref._floaty(78, base, kind)[:, 0]
        out = torch.empty(3, 128, 128, device=dev, dtype=torch.uint8)
        ops.exp2_index(torch.from_numpy(np.ascontiguousarray(x)).to(dev), tl, 128, 3, bd, lut, True, out)
        got = out.cpu().numpy()
        crop = x[:3, tl[0]:tl[0] + 128, tl[1]:tl[1] + 128]
        want = exp2_ref.index(crop)
        if kind == "u8":
            assert np.array_equal(got, want)
            continue
        v = exp2_ref.transform(crop)
        with np.errstate(invalid="ignore"):
            near = np.min(np.abs(v[..., None] - bounds) / np.maximum(bounds, 1e-300), axis=-1) < 1e-9
        near &= (v > 0.0) & (v < 200.0)                       # the clip's own constants are exact on both sides
        assert near.mean() < 1e-4
        assert np.array_equal(got[~near], want[~near])
        assert (got == exp2_ref.BAD).sum() == np.isnan(crop).sum() > 0


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_index_kernel_into_misaligned_output(shift):
    """The output may start anywhere: 3 frames of 13 x 13 (507 bytes, no multiple of 4) written 1, 2 and 3 bytes past a word
    boundary equal the aligned result, and the guard bytes before and after stay as they were."""
    from p2igan_bench import ops
    from p2igan_bench.evaluation import crop_origin, paper_cmap, truth_lut
    from p2igan_bench.utils import seeded
    dev = torch.device("cuda")
    bd, lut = torch.from_numpy(paper_cmap()[0]).to(dev), torch.from_numpy(truth_lut(True)).to(dev)
    x = seeded.exp1_truth(79, 3, 17, 15)[:, 0]
    tl = crop_origin(17, 15, 13)
    want = exp2_ref.index(x[:, tl[0]:tl[0] + 13, tl[1]:tl[1] + 13])
    n = 3 * 13 * 13
    buf = torch.full((n + 16,), 200, device=dev, dtype=torch.uint8)
    assert buf.data_ptr() % 4 == 0
    out = buf[shift:shift + n].view(3, 13, 13)
    ops.exp2_index(torch.from_numpy(np.ascontiguousarray(x)).to(dev), tl, 13, 3, bd, lut, True, out)
    got = buf.cpu().numpy()
    assert np.array_equal(got[shift:shift + n].reshape(3, 13, 13), want)
    assert (got[:shift] == 200).all() and (got[shift + n:] == 200).all()


ODD = [
    # crop 13 of 17 x 15, 5 frames: panel i of the event's [P, 5, 13, 13] tensor starts 845 i bytes in
    {"name": "odd_array", "form": "array", "mode": "radar", "crop": 13, "keys": ["event_01"], "events": [[5, 17, 15]], "truth": "u8",
     "mask_frac": 0.1, "methods": {"gan": {"seed": 71, "noise": 10.0, "over": 0.03, "nan": 0.03, "neg_every": 7},
                                   "stdk": {"seed": 72, "noise": 25.0, "dtype": "f64", "extra": 2}}},
    # two events of 5 and 3 frames; f32 truth and observation
    {"name": "odd_path", "form": "path", "mode": "gauge", "crop": 13, "keys": ["event_01", "event_02"], "events": [[5, 17, 15], [3, 13, 16]],
     "truth": "f32", "mask_frac": 0.1, "methods": {"gan": {"seed": 73, "noise": 10.0}, "idw": {"seed": 74, "noise": 20.0, "t": [7, 4]}}},
]


def _assert_far_from_bounds(arrays, size):
    """Equal indices are only fair where no f32 / f64 value is within 1e-9 (relative) of a bound: the device pow is a few ulp from
    numpy's.  The inputs are seeded, so this is a fixed property of the case; uint8 inputs are exact through the table."""
    bounds = exp2_ref.cmap_tables()[0]
    for a in arrays:
        if a.dtype == np.uint8:
            continue
        v = exp2_ref.transform(exp2_ref._crop(exp2_ref.thw(a), size))
        v = v[(v > 0.0) & (v < 200.0)]                         # NaN drops out; the clip's own constants are exact on both sides
        assert (np.abs(v[:, None] - bounds) / np.maximum(bounds, 1e-300)).min() >= 1e-9


@pytest.mark.parametrize("case", ODD, ids=lambda c: c["name"])
def test_odd_crop_and_frame_count(case, tmp_path):
    """An odd crop with an odd frame count: compute_exp2 and run_exp2 (GIF included) against the restatement."""
    from PIL import Image
    from p2igan_bench.evaluation import Exp2Result, compute_exp2, run_exp2
    preds, truth, obs, mask, kw = exp2_ref.build_case(case)
    flat = lambda d: list(d.values()) if isinstance(d, dict) else [d]            # noqa: E731
    _assert_far_from_bounds(flat(truth) + flat(obs) + [a for p in preds.values() for a in flat(p)], kw["crop_size"])
    want = exp2_ref.exp2(preds, truth, obs, mask, **kw)["events"]
    assert all(e["frames"] % 2 == 1 for e in want)
    same_events(as_ref_layout(compute_exp2(preds, truth, obs, mask, **kw)), want)
    run_exp2(preds, truth, obs, mask, str(tmp_path), kw["crop_size"], None, 0.0, 0.0, 4, mode=kw["mode"], zoom=1)
    same_events(as_ref_layout(Exp2Result.load(str(tmp_path / "exp2_data.npz"))), want)
    for e in want:
        with Image.open(tmp_path / f"comparison_{e['key']}.gif") as im:
            assert im.n_frames == e["frames"]


def _points(rng, S, K):
    """K distinct points in np.argwhere order: the four corners (discs clipped by the panel) and neighbours (overlaps) first."""
    if K == 0:
        return np.zeros((0, 2), np.int32)
    must = [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (S // 2, S // 2), (S // 2, S // 2 + 1), (S // 2 + 1, S // 2)][:K]
    chosen = set(must)
    while len(chosen) < K:
        chosen.add((int(rng.integers(S)), int(rng.integers(S))))
    return np.array(sorted(chosen), np.int32)


@pytest.mark.parametrize("S,zoom,P,K,bits", [(8, 1, 1, 0, 1), (8, 3, 2, 1, 1), (8, 3, 1, 7, 1), (13, 1, 3, 79, 1), (13, 3, 5, 79, 0b10001),
                                             (13, 3, 4, 0, 0), (128, 1, 3, 79, 1), (128, 3, 2, 79, 1), (128, 1, 5, 1, 0b100),
                                             (128, 1, 2, 600, 0b10), (128, 2, 1, 1100, 1)])
def test_compose_matches_restatement(S, zoom, P, K, bits):
    """600 and 1100 points take two and three LDS rounds of the point list (512 points a round): a later round's disc must win
    over an earlier round's, and its face colour is looked up by the point's number in the whole list."""
    from p2igan_bench import ops
    rng = np.random.default_rng(1000 * S + 10 * zoom + P)
    n = 3
    panels = rng.integers(0, 142, size=(P, n, S, S), dtype=np.uint8)          # BAD (141) included
    pts = _points(rng, S, K)
    side, gap, ox, oy = S * zoom, 5, 3, 7
    width = ox + P * side + (P - 1) * gap + 2
    width += width % 16 == 0                                # never a multiple of 16: the pitch pads every row
    pitch, Hc = ops.exp2_pitch(width), oy + side + 9
    assert width % 16 != 0
    chrome = rng.integers(144, 160, size=(Hc, pitch), dtype=np.uint8)
    dev = torch.device("cuda")
    out = torch.full((n, Hc, pitch), 255, device=dev, dtype=torch.uint8)
    ops.exp2_compose(torch.from_numpy(panels).to(dev), zoom, bits, torch.from_numpy(pts).to(dev) if K else None,
                     torch.from_numpy(chrome).to(dev), oy, ox, side + gap, 142, 143, out)
    want = exp2_ref.compose(panels, zoom, bits, pts, chrome, oy, ox, side + gap, 142, 143)
    assert np.array_equal(out.cpu().numpy(), want)


def _array_case():
    c = next(c for c in exp2_ref.CASES if c["name"] == "array_long")
    return exp2_ref.build_case(c)


def test_gif_reads_back_exactly(tmp_path, monkeypatch):
    """fps 7 asks the writer for int(1000 / 7) = 142 ms.  A GIF holds a frame's delay in hundredths of a second, so the file
    carries 14 of them and reads back as 140 ms: the test checks the 142 where it is handed over and the 140 in the file."""
    from PIL import Image
    from p2igan_bench.evaluation import Exp2Result, exp2_canvases, run_exp2
    preds, truth, obs, mask, kw = _array_case()
    asked, save = [], Image.Image.save
    monkeypatch.setattr(Image.Image, "save", lambda self, fp, *a, **k: (asked.append(k.get("duration")), save(self, fp, *a, **k))[1])
    run_exp2(preds, truth, obs, mask, str(tmp_path), kw["crop_size"], None, 0.0, 0.0, 7, mode=kw["mode"], zoom=3)
    monkeypatch.undo()
    assert asked == [int(1000 / 7)] == [142]
    res = Exp2Result.load(str(tmp_path / "exp2_data.npz"))
    ev = res.events[0]
    canv = exp2_canvases(ev, zoom=3)
    assert canv.shape[0] == ev.frames == 31
    # the kernel's part of the canvas (below the host's title strip) is the restatement's
    from p2igan_bench.evaluation import EXP2_IDX_BG, EXP2_IDX_EDGE, exp2_chrome, exp2_layout
    lay = exp2_layout(len(ev.labels), 8, 3)
    want = exp2_ref.compose(ev.panels, 3, 1, ev.points, exp2_chrome(ev.labels, 8, 3), lay["oy"], lay["ox"], lay["step"], EXP2_IDX_BG,
                            EXP2_IDX_EDGE)[:, :, :lay["width"]]
    assert np.array_equal(canv[:, lay["oy"]:], want[:, lay["oy"]:])
    with Image.open(tmp_path / "comparison_event_01.gif") as im:
        assert im.n_frames == 31 and im.info["loop"] == 0
        for t in range(im.n_frames):
            im.seek(t)
            assert im.info["duration"] == int(1000 / 7) // 10 * 10 == 140
            assert np.array_equal(np.asarray(im.convert("RGB")), res.palette[canv[t]]), t


def test_two_runs_are_byte_identical(tmp_path):
    from p2igan_bench.evaluation import run_exp2
    c = next(c for c in exp2_ref.CASES if c["name"] == "path_order")
    preds, truth, obs, mask, kw = exp2_ref.build_case(c)
    for d in ("a", "b"):
        run_exp2(preds, truth, obs, mask, str(tmp_path / d), kw["crop_size"], None, 0.0, 0.0, 4, mode=kw["mode"], zoom=2)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 4
    for f in names:
        if f.endswith(".npz"):              # a zip: its member timestamps differ; the members must not
            with np.load(tmp_path / "a" / f) as za, np.load(tmp_path / "b" / f) as zb:
                assert za.files == zb.files and all(za[k].tobytes() == zb[k].tobytes() for k in za.files)
        else:
            assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f


def test_host_device_and_zarr_inputs_give_the_same_data(tmp_path):
    from p2igan_bench.evaluation import Exp2Result, compute_exp2, run_exp2
    c = next(c for c in exp2_ref.CASES if c["name"] == "path_order")
    preds, truth, obs, mask, kw = exp2_ref.build_case(c)
    dev = torch.device("cuda")
    on = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}          # noqa: E731
    a = compute_exp2(preds, truth, obs, mask, **kw)
    b = compute_exp2({n: on(p) for n, p in preds.items()}, on(truth), on(obs), torch.from_numpy(mask).to(dev), **kw)
    pp, tp, op = exp2_ref.write_zarrs(tmp_path, preds, truth, obs)
    run_exp2(pp, tp, op, mask, str(tmp_path / "z"), kw["crop_size"], None, 0.0, 0.0, 4, mode=kw["mode"], zoom=1)
    z = Exp2Result.load(str(tmp_path / "z" / "exp2_data.npz"))
    a.save(str(tmp_path / "a.npz"))
    b.save(str(tmp_path / "b.npz"))
    with np.load(tmp_path / "a.npz") as za, np.load(tmp_path / "b.npz") as zb, np.load(tmp_path / "z" / "exp2_data.npz") as zz:
        assert za.files == zb.files == zz.files
        for k in za.files:
            assert za[k].tobytes() == zb[k].tobytes() == zz[k].tobytes(), k
    same_events(as_ref_layout(a), exp2_ref.exp2(preds, truth, obs, mask, **kw)["events"])
    same_events(as_ref_layout(z), as_ref_layout(a))


def _cli_inputs(tmp_path):
    from p2igan_bench.utils import seeded
    truths = {f"event_{i + 1:02d}": seeded.exp1_truth(910 + i, t, 48, 40) for i, t in enumerate((9, 14))}
    obss = {k: seeded.exp1_truth(930 + i, v.shape[0], 48, 40) for i, (k, v) in enumerate(truths.items())}
    preds = {name: {k: seeded.exp1_pred(960 + 10 * j + i, v, 12.0 + 10 * j) for i, (k, v) in enumerate(truths.items())}
             for j, name in enumerate(("p2igan", "idw"))}
    pp, tp, op = exp2_ref.write_zarrs(tmp_path, preds, truths, obss)
    full = seeded.exp1_mask(6, 48, 40, 0.05)
    np.savetxt(tmp_path / "mask.txt", full.astype(np.float64), fmt="%d")
    return preds, truths, obss, full, pp, tp, op


def test_cli_exp2_end_to_end(tmp_path):
    from p2igan_bench.evaluation import Exp2Result, crop_mask
    preds, truths, obss, full, pp, tp, op = _cli_inputs(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts", "evaluate.py"), "--truth", tp,
           "--method", f"p2igan={pp['p2igan']}", "--method", f"idw={pp['idw']}", "--mask", str(tmp_path / "mask.txt"),
           "--mode", "radar", "--crop-size", "32"]
    r = subprocess.run(cmd + ["--output", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(cmd + ["--output", str(tmp_path / "with"), "--exp2", str(tmp_path / "e2"), "--observation", op, "--gif-fps", "5",
                              "--exp2-zoom", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for f in ("metrics.json", "metrics.txt"):                   # exp1's outputs do not depend on the flag
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "with" / f).read_bytes(), f
    assert sorted(os.listdir(tmp_path / "plain")) == ["metrics.json", "metrics.txt"]
    e2 = tmp_path / "e2"
    assert sorted(os.listdir(e2)) == ["comparison_event_01.gif", "comparison_event_02.gif", "event_ranges.txt", "exp2_data.npz"]
    assert (e2 / "event_ranges.txt").read_text() == "event_01: frames 1-9 (count=9)\nevent_02: frames 1-14 (count=14)\n"
    res = Exp2Result.load(str(e2 / "exp2_data.npz"))
    same_events(as_ref_layout(res), exp2_ref.exp2(preds, truths, obss, crop_mask(full, 32), 32, "radar")["events"])
    from PIL import Image
    with Image.open(e2 / "comparison_event_02.gif") as im:
        assert im.n_frames == 14 and im.info["duration"] == 200


def test_paper_grid(tmp_path, monkeypatch):
    """The PDF exists, and the RGBA panels handed to matplotlib's Axes.imshow are the restatement's; crop_pdf is refused."""
    import matplotlib.axes
    from p2igan_bench.evaluation import crop_mask, run_exp2_paper_zarr
    preds, truths, obss, full, pp, tp, op = _cli_inputs(tmp_path)
    seen = []
    orig = matplotlib.axes.Axes.imshow

    def imshow(self, a, *args, **k):
        seen.append(np.array(a))
        return orig(self, a, *args, **k)
    monkeypatch.setattr(matplotlib.axes.Axes, "imshow", imshow)
    events = [{"event_id": 1, "select_idx": [0, 4, 12], "title": "first"}, {"event_id": 2, "select_idx": [1, 13, 2], "title": "second"}]
    methods = {"p2igan": pp["p2igan"], "none": "", "idw": pp["idw"]}
    run_exp2_paper_zarr(op, methods, events, str(tmp_path / "mask.txt"), 32, str(tmp_path / "paper"), "grid.pdf")
    assert (tmp_path / "paper" / "grid.pdf").stat().st_size > 1000
    tab = exp2_ref.rgba_table()
    tab[:exp2_ref.BAD, 3] = 255
    black = np.zeros((32, 32, 4), np.uint8)
    black[..., 3] = 255
    want = []
    for ev in events:
        key = f"event_{ev['event_id']:02d}"
        srcs = [None, obss[key], preds["p2igan"][key], None, preds["idw"][key]]       # RadarMasked, Nimrod, p2igan, none, idw
        for i in ev["select_idx"]:
            for m, src in enumerate(srcs):
                if m == 0:
                    want.append(black)
                elif src is None or i >= src.shape[0]:
                    want.append(tab[np.zeros((32, 32), np.uint8)])                    # a zero panel: the first colour
                else:
                    want.append(tab[exp2_ref.index(exp2_ref._crop(exp2_ref.thw(src), 32)[i])])
    assert len(seen) == len(want) == 30
    for a, b in zip(seen, want):
        assert np.array_equal(a, b)
    assert crop_mask(full, 32).sum() > 0
    with pytest.raises(NotImplementedError):
        run_exp2_paper_zarr(op, methods, events, str(tmp_path / "mask.txt"), 32, str(tmp_path / "paper"), "grid.pdf", crop_pdf=True)
