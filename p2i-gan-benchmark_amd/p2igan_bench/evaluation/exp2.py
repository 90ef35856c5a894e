"""exp2 comparison renders (reference experiments/exp2.py ``run_exp2`` / ``_save_combo_gif``) on csrc/eval_exp2.hip: the events' index
panels (``iter_exp2``, ``compute_exp2``), their GIF canvases (``exp2_canvases``), ``run_exp2`` and the paper's frame grid
(``run_exp2_paper_zarr``: the panels' colour indices from the device, laid out by matplotlib, which is imported only there).
DESIGN.md section 12."""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import ops
from ._common import _thw, _to_device, crop_mask, crop_origin, device_tables, eval_device
from .exp2_chrome import (EXP2_IDX_BAD, EXP2_IDX_BG, EXP2_IDX_EDGE, PAPER_BOUNDS, PAPER_SUB, _exp2_paste, _exp2_text, exp2_chrome,
                          exp2_layout, exp2_palette, paper_cmap, write_exp2_gif)

EXP2_MAX_EVENTS = 20        # the path form takes the first 20 events ...
EXP2_MAX_FRAMES = 30        # ... and 30 frames of each


@dataclass
class Exp2Event:
    """One event of exp2 as palette indices.  ``panels`` [P, frames, S, S] uint8 in label order; a panel whose ``gauge`` flag is set
    is drawn as discs at ``points`` [K, 2] (row, column; np.argwhere order) over black, and its array holds the source's own
    indices (for the first panel: the observation's, of which ``point_idx`` [frames, K] are the discs' colours).  ``total`` is the
    count event_ranges.txt and the title report; ``frames`` (<= total: the observation may be shorter) is what the GIF holds."""
    key: str
    title: str
    labels: List[str]
    gauge: List[bool]
    panels: np.ndarray
    points: np.ndarray
    point_idx: np.ndarray
    frames: int
    total: int
    dev_panels: Optional[torch.Tensor] = field(default=None, repr=False, compare=False)

    @property
    def range_line(self) -> str:
        return f"{self.key}: frames 1-{self.total} (count={self.total})"


@dataclass
class Exp2Result:
    """The numbers behind run_exp2's files: the events, the palette [256, 3] the indices refer to, the colour table's bounds, and
    ``per_event`` (the path form: event_ranges.txt exists)."""
    events: List[Exp2Event]
    palette: np.ndarray
    bounds: np.ndarray
    per_event: bool = True

    @property
    def range_lines(self) -> List[str]:
        return [e.range_line for e in self.events]

    def save(self, path: str) -> None:
        head = {"per_event": self.per_event,
                "events": [{"key": e.key, "title": e.title, "labels": e.labels, "gauge": e.gauge, "frames": e.frames, "total": e.total}
                           for e in self.events]}
        arrays = {"header": np.array(json.dumps(head)), "palette": self.palette, "bounds": self.bounds}
        for i, e in enumerate(self.events):
            arrays[f"panels/{i}"], arrays[f"points/{i}"], arrays[f"point_idx/{i}"] = e.panels, e.points, e.point_idx
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path: str) -> "Exp2Result":
        with np.load(path) as z:
            head = json.loads(str(z["header"]))
            events = [Exp2Event(key=h["key"], title=h["title"], labels=h["labels"], gauge=h["gauge"], panels=z[f"panels/{i}"],
                                points=z[f"points/{i}"], point_idx=z[f"point_idx/{i}"], frames=h["frames"], total=h["total"])
                      for i, h in enumerate(head["events"])]
            return cls(events=events, palette=z["palette"], bounds=z["bounds"], per_event=head["per_event"])


class _Exp2Source:
    """Where an event's array comes from: a zarr path (zarr_lite), a dict of event arrays, or one array used for every event."""

    def __init__(self, src):
        self.src, self.group = src, None
        if isinstance(src, (str, os.PathLike)):
            from ..data import zarr_lite
            self.group = zarr_lite.Group(os.fspath(src), "r")

    def keys(self) -> List[str]:
        return [k for k in (self.group.keys() if self.group is not None else self.src.keys()) if isinstance(k, str)]

    def get(self, key: str):
        if self.group is not None:
            try:
                node = self.group[key]
            except KeyError:
                raise FileNotFoundError(f"Missing event {key} in {self.src}") from None
            return np.asarray(node[:])
        if isinstance(self.src, dict):
            if self.src.get(key) is None:
                raise FileNotFoundError(f"Missing event {key} in the given events")
            return self.src[key]
        return self.src


class _Exp2Tables:
    def __init__(self, dev, divide_by_3):
        self.dev, self.divide_by_3 = dev, bool(divide_by_3)
        self.bounds = paper_cmap()[0]
        self.bounds_d = torch.from_numpy(self.bounds).to(dev)
        self.lut = device_tables(dev, self.divide_by_3)[0]

    def index(self, src, tl, size, n, out):
        ops.exp2_index(src, tl, size, n, self.bounds_d, self.lut, self.divide_by_3, out)


def _exp2_mask_points(mask, size: int) -> np.ndarray:
    mask = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    if mask.shape != (size, size):
        raise ValueError(f"operands could not be broadcast together with shapes ({size},{size}) {mask.shape}")
    return np.ascontiguousarray(np.argwhere(mask).astype(np.int32)).reshape(-1, 2)


def _exp2_event(tab: _Exp2Tables, key, title_of, truth, obs, preds, points, size, cap, input_label, truth_label) -> Exp2Event:
    """One event by the reference's rules: the truth and the observation are cropped and cut to ``cap`` frames; every prediction is
    aligned to the current truth (which it may shorten for the methods after it) before its crop; the common length ``total`` is
    applied to every panel, and the GIF holds min(total, observation frames) of them."""
    dev = tab.dev
    truth = _to_device(_thw(truth), dev)
    obs = _to_device(_thw(obs), dev)
    n_obs = obs.shape[0] if cap is None else min(obs.shape[0], cap)
    total = truth.shape[0] if cap is None else min(truth.shape[0], cap)
    panel_src = {input_label: (obs, crop_origin(obs.shape[1], obs.shape[2], size)),
                 truth_label: (truth, crop_origin(truth.shape[1], truth.shape[2], size))}
    for name, arr in preds:
        p = _to_device(_thw(arr), dev)
        total = min(p.shape[0], total)              # never grows: the last value is the common length
        panel_src[name] = (p, crop_origin(p.shape[1], p.shape[2], size))
    frames = max(min(total, n_obs), 0)
    labels = list(panel_src)
    gauge = [lb.lower() in ("input", "gauge") for lb in labels]
    panels = torch.empty(len(labels), frames, size, size, device=dev, dtype=torch.uint8)
    for i, lb in enumerate(labels):
        src, tl = panel_src[lb]
        tab.index(src, tl, size, frames, panels[i])
    host = panels.cpu().numpy()
    pidx = host[0][:, points[:, 0], points[:, 1]] if frames else np.zeros((0, points.shape[0]), np.uint8)
    return Exp2Event(key=key, title=title_of(total), labels=labels, gauge=gauge, panels=host, points=points,
                     point_idx=np.ascontiguousarray(pidx), frames=frames, total=total, dev_panels=panels)


def _exp2_is_events(x) -> bool:
    return isinstance(x, (str, os.PathLike, dict))


def iter_exp2(preds, truth, observation, mask_train, crop_size: int, divide_by_3: bool = True, mode: str = "radar", device=None):
    """Yields (per_event, Exp2Event) event by event; see compute_exp2."""
    dev = eval_device(device, "exp2 renders run")
    size = int(crop_size)
    input_label, truth_label = ("Gauge", "Radar") if mode == "gauge" else ("Input", "Truth")
    with torch.cuda.device(dev):
        tab = _Exp2Tables(dev, divide_by_3)
        if _exp2_is_events(truth) and _exp2_is_events(observation):
            tsrc, osrc = _Exp2Source(truth), _Exp2Source(observation)
            # the reference's numeric key never matches (its pattern is r"event[_-]?(\\d+)"): the order is (10**9, key), plain sorted
            keys = sorted(tsrc.keys())
            if not keys:
                raise FileNotFoundError(f"No event groups found in {truth if not isinstance(truth, dict) else 'the given events'}")
            psrc = [(name, _Exp2Source(src)) for name, src in preds.items()]
            points = None
            for key in keys[:EXP2_MAX_EVENTS]:
                t, o = tsrc.get(key), osrc.get(key)
                # the reference crops truth and observation (ValueError) and applies the mask before it opens the methods
                for a in (t, o):
                    shp = _thw(a).shape
                    crop_origin(shp[1], shp[2], size)
                if points is None:
                    points = _exp2_mask_points(mask_train, size)
                evp = [(name, s.get(key)) for name, s in psrc]
                yield True, _exp2_event(tab, key, lambda n, k=key: f"{k} | total frames {n}", t, o, evp, points, size, EXP2_MAX_FRAMES,
                                        input_label, truth_label)
            return
        for name, src in preds.items():
            if _exp2_is_events(src):
                raise TypeError(f"method {name!r}: per-event predictions need a per-event truth and observation")
        for a in (truth, observation):
            shp = _thw(a).shape
            crop_origin(shp[1], shp[2], size)
        points = _exp2_mask_points(mask_train, size)
        yield False, _exp2_event(tab, "event_01", lambda n: f"Event 01 | total frames {n}", truth, observation, list(preds.items()),
                                 points, size, None, input_label, truth_label)


def compute_exp2(preds, truth, observation, mask_train, crop_size: int, divide_by_3: bool = True, mode: str = "radar",
                 device=None) -> Exp2Result:
    """The index panels of the reference's run_exp2 (experiments/exp2.py) on the device, without writing anything.  *Path form*:
    ``truth`` and ``observation`` are zarr paths or dicts of event arrays; the event keys are taken in lexicographic order, the
    first 20 of them, 30 frames each; a method is a path, a dict, or one array used for every event; an event a source lacks
    raises FileNotFoundError.  *Array form*: whole arrays, no frame cap, one event ``event_01``."""
    events, per_event = [], True
    for per_event, ev in iter_exp2(preds, truth, observation, mask_train, crop_size, divide_by_3, mode, device):
        ev.dev_panels = None
        events.append(ev)
    return Exp2Result(events=events, palette=exp2_palette(), bounds=paper_cmap()[0], per_event=per_event)


def default_zoom(size: int) -> int:
    """The panels' magnification when none is asked for: the smallest that makes a panel at least 256 pixels wide."""
    return max(1, -(-256 // int(size)))


def exp2_canvases(ev: Exp2Event, zoom: Optional[int] = None, device=None, titles: bool = True) -> np.ndarray:
    """The event's GIF frames as palette indices [frames, height, width] uint8: the chrome and the panel row composed on the device
    (p2i_exp2_compose), then the per-frame title strip ``<title> | Frame t/n`` drawn on the host."""
    dev = eval_device(device, "exp2 renders run")
    S = ev.panels.shape[-1]
    zoom = default_zoom(S) if zoom is None else int(zoom)
    if zoom < 1:
        raise ValueError(f"zoom must be >= 1, got {zoom}")
    lay = exp2_layout(len(ev.labels), S, zoom)
    if ev.frames <= 0:
        return np.zeros((0, lay["height"], lay["width"]), np.uint8)
    pts = np.ascontiguousarray(ev.points, dtype=np.int32).reshape(-1, 2)
    if pts.size and (pts.min() < 0 or pts.max() >= S):
        raise ValueError("a mask point lies outside the panel")
    bits = sum(1 << i for i, g in enumerate(ev.gauge) if g)
    with torch.cuda.device(dev):
        panels = ev.dev_panels if ev.dev_panels is not None and ev.dev_panels.device == dev else torch.from_numpy(ev.panels).to(dev)
        chrome = torch.from_numpy(exp2_chrome(ev.labels, S, zoom)).to(dev)
        out = torch.empty(ev.frames, lay["height"], lay["pitch"], device=dev, dtype=torch.uint8)
        ops.exp2_compose(panels.contiguous(), zoom, bits, torch.from_numpy(pts).to(dev) if pts.size else None, chrome, lay["oy"], lay["ox"],
                         lay["step"], EXP2_IDX_BG, EXP2_IDX_EDGE, out)
        canv = np.ascontiguousarray(out.cpu().numpy()[:, :, :lay["width"]])
    if titles and ev.title:
        for t in range(ev.frames):
            _exp2_paste(canv[t], _exp2_text(f"{ev.title} | Frame {t + 1}/{ev.frames}", 12), 2, lay["width"] // 2, lay["width"])
    return canv


def run_exp2(preds, truth, observation, mask_train, out_dir: str, crop_size: int, frames=None, vmin: float = 0.0, vmax: float = 0.0,
             gif_fps: int = 4, divide_by_3: bool = True, mode: str = "radar", device=None, zoom: Optional[int] = None) -> None:
    """The reference's run_exp2: ``comparison_<event>.gif`` per event and ``event_ranges.txt`` (path form), or
    ``comparison_event_01.gif`` (array form), plus ``exp2_data.npz`` (Exp2Result.save).  ``frames``, ``vmin`` and ``vmax`` are
    accepted and unused, as in the reference.  The GIFs are written event by event: when an event fails, the ones before it exist
    and event_ranges.txt does not, as there."""
    os.makedirs(out_dir, exist_ok=True)
    palette = exp2_palette()
    events, per_event = [], True
    for per_event, ev in iter_exp2(preds, truth, observation, mask_train, crop_size, divide_by_3, mode, device):
        if ev.frames > 0:
            write_exp2_gif(exp2_canvases(ev, zoom, device), palette, os.path.join(out_dir, f"comparison_{ev.key}.gif"), gif_fps)
        ev.dev_panels = None
        events.append(ev)
    res = Exp2Result(events=events, palette=palette, bounds=paper_cmap()[0], per_event=per_event)
    if per_event:
        with open(os.path.join(out_dir, "event_ranges.txt"), "w", encoding="utf-8") as f:
            for line in res.range_lines:
                f.write(line.rstrip() + "\n")
    res.save(os.path.join(out_dir, "exp2_data.npz"))


def paper_panels(observation_path, methods: Dict[str, object], events, mask, crop_size: int, method_order=None, device=None):
    """The paper grid's panels: per event ``(labels, idx [columns, rows, S, S] uint8, points [K, 2])``.  Column order defaults to
    RadarMasked, Nimrod (both the observation), then the methods; a method without a source and a frame beyond a source's length
    give a zero panel (index 0, as the reference's np.zeros maps)."""
    dev = eval_device(device, "exp2 renders run")
    size = int(crop_size)
    if method_order is None:
        method_order = ["RadarMasked", "Nimrod"] + list(methods.keys())
    order = list(method_order)
    points = _exp2_mask_points(crop_mask(np.asarray(mask).astype(bool), size), size)
    out = []
    with torch.cuda.device(dev):
        tab = _Exp2Tables(dev, True)
        osrc = _Exp2Source(observation_path)
        msrc = {name: _Exp2Source(p) for name, p in methods.items() if p is not None and not (isinstance(p, str) and not p)}
        for event in events:
            key = f"event_{int(event['event_id']):02d}"
            select = [int(i) for i in event["select_idx"]]
            obs = _to_device(_thw(osrc.get(key)), dev)
            cache = {}                                      # source name -> its index frames [T, S, S] on the host

            def frames_of(sid, src):
                if sid not in cache:
                    idx = torch.empty(src.shape[0], size, size, device=dev, dtype=torch.uint8)
                    tab.index(src, crop_origin(src.shape[1], src.shape[2], size), size, src.shape[0], idx)
                    cache[sid] = idx.cpu().numpy()
                return cache[sid]
            cols = []
            for name in order:
                col = np.zeros((len(select), size, size), np.uint8)
                fr = None
                if name in ("RadarMasked", "Nimrod"):
                    fr = frames_of("", obs)
                elif name in msrc:
                    fr = frames_of("m:" + name, _to_device(_thw(msrc[name].get(key)), dev))
                if fr is not None:
                    for r, i in enumerate(select):
                        if i < fr.shape[0]:
                            col[r] = fr[i]                  # a negative index counts from the end, as source[idx] does there
                cols.append(col)
            out.append((list(order), np.stack(cols) if cols else np.zeros((0, len(select), size, size), np.uint8), points))
    return out


def run_exp2_paper_zarr(observation_path, methods: Dict[str, object], events, mask_path: str, crop_size: int, out_dir: str,
                        output_pdf: str, method_order=None, crop_pdf: bool = False, crop_output: str = "cropped_stitched.pdf",
                        crop_y_ranges=((0.019, 0.5), (0.58, 1.0)), crop_zoom: float = 3.0, crop_margin_left: float = 0.0,
                        crop_margin_right: float = 0.0, device=None) -> None:
    """The reference's run_exp2_paper_zarr: one PDF with, per event, a title row and one row per selected frame, one column per
    entry of the method order.  The panels' colour indices come from the device (paper_panels); matplotlib lays the RGBA panels
    out.  ``crop_pdf=True`` (the PyMuPDF branch) is not implemented."""
    if crop_pdf:
        raise NotImplementedError("crop_pdf needs PyMuPDF; experiments/main.py never asks for it")
    from matplotlib.cm import ScalarMappable
    from matplotlib.colors import BoundaryNorm, ListedColormap
    from matplotlib.figure import Figure
    from matplotlib.gridspec import GridSpec
    os.makedirs(out_dir, exist_ok=True)
    events = list(events)
    mask = np.loadtxt(mask_path).astype(bool)
    blocks = paper_panels(observation_path, methods, events, mask, crop_size, method_order, device)
    bounds, colors = paper_cmap()
    rgba = np.zeros((256, 4), np.uint8)
    rgba[:EXP2_IDX_BAD] = (colors * 255).astype(np.uint8)
    ncols = len(blocks[0][0]) if blocks else 0
    nrows_each = len(list(events[0]["select_idx"]))
    total_rows = (nrows_each + 1) * len(events)
    fig = Figure(figsize=(2.4 * ncols, 1.9 * total_rows))
    gs = GridSpec(nrows=total_rows, ncols=ncols, figure=fig, top=0.93, bottom=0.06, wspace=0.04, hspace=0.02)
    cmap = ListedColormap(colors[:, :3].tolist(), name=f"seg{PAPER_SUB}_smooth")
    sm = ScalarMappable(cmap=cmap, norm=BoundaryNorm(bounds, cmap.N, clip=True))
    sm.set_array([])
    cbar = fig.colorbar(sm, cax=fig.add_axes([0.20, 0.88, 0.60, 0.02]), orientation="horizontal", ticks=list(PAPER_BOUNDS))
    cbar.set_ticklabels([f"{b:g}" for b in PAPER_BOUNDS[:-1]] + [""])
    cbar.set_label("Rainfall (mm/h)", fontsize=13, labelpad=3)
    cbar.ax.tick_params(labelsize=11)

    def face_of(panel):                             # the discs' face colours: the panel's own colour at every mask point
        return (rgba[panel[points[:, 0], points[:, 1]]] / 255.0).reshape(-1, 4)
    row = 0
    for event, (labels, idx, points) in zip(events, blocks):
        ax_title = fig.add_subplot(gs[row, :])
        ax_title.axis("off")
        ax_title.text(-0.015, 0.2, event["title"], fontsize=14, fontweight="bold", ha="left", va="center", transform=ax_title.transAxes)
        row += 1
        for t in range(nrows_each):
            for m, label in enumerate(labels):
                ax = fig.add_subplot(gs[row + t, m])
                if label == "RadarMasked":
                    black = np.zeros(idx[m, t].shape + (4,), np.uint8)
                    black[..., 3] = 255
                    ax.imshow(black)
                    ax.scatter(points[:, 1], points[:, 0], c=face_of(idx[m, t]), s=24, edgecolors="#dddddd", linewidths=0.4, zorder=5)
                else:
                    ax.imshow(rgba[idx[m, t]])
                ax.set_xticks([])
                ax.set_yticks([])
                for s in ax.spines.values():
                    s.set_visible(False)
                if label == "Gauge":
                    ax.scatter(points[:, 1], points[:, 0], c=face_of(idx[m, t]), s=38, edgecolors="black", linewidths=0.7, zorder=5)
                if t == 0:
                    ax.set_title(label, fontsize=13)
                if m == 0:
                    ax.text(-0.12, 0.5, f"{t * 5} min", transform=ax.transAxes, ha="center", va="center", fontsize=12, rotation=90)
        row += nrows_each
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fig.tight_layout(rect=[0, 0, 1, 0.7])
    fig.savefig(os.path.join(out_dir, output_pdf), format="pdf", bbox_inches="tight")
