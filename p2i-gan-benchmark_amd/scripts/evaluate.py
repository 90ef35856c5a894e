#!/usr/bin/env python3
"""Score inference outputs with the benchmark's exp1 table (the exp1 half of the reference's experiments/main.py) on the GPU.

    python scripts/evaluate.py --truth truth.zarr --method p2igan=pred.zarr --method stdk=stdk.zarr \\
        --mask mask_train.txt --mode radar --crop-size 128 --output results/exp1

Every zarr is a group of per-event arrays (``event_01``, ``event_02``, ...) as scripts/infer.py writes them.  The truth's keys are
taken in sorted order, and every method must hold all of them: unlike run_exp1, which skips an event a method lacks and so shifts
its frames against the truth's, a missing event is refused here.  The mask is read with ``np.loadtxt(...).astype(bool)`` and
center-cropped to the crop size.  Writes DIR/metrics.json (indent 2, sorted keys) and DIR/metrics.txt in main.py's layout.

With ``--exp3 DIR3`` it also runs the benchmark's exp3 analysis (run_exp3) on the same inputs and writes DIR3/metrics.json,
DIR3/metrics.txt (``NSE_<name>: value`` lines, as main.py writes them), DIR3/exp3_data.npz and the figures (scatter_panels.pdf,
residual_panels.pdf, nse_boxplot.pdf, logfreq.pdf).  exp1's outputs do not depend on it.

With ``--exp2 DIR2 --observation OBS.zarr`` it also writes the benchmark's exp2 comparison animations (run_exp2 on the zarr paths:
the first 20 events in lexicographic key order, 30 frames each): DIR2/comparison_<event>.gif, DIR2/event_ranges.txt and
DIR2/exp2_data.npz.  ``--exp2-pdf FILE --exp2-events EVENTS.json`` writes the paper's frame grid (run_exp2_paper_zarr); the JSON is
a list of ``{"event_id": 3, "select_idx": [0, 2, 4], "title": "..."}``.  Neither changes exp1's or exp3's outputs.

With ``--scale DIRS [--scales N ...]`` it also runs the scale-aware verification (run_scale: the fractions skill score over
``--thresholds`` x the neighbourhood sizes, and the radially averaged power spectra) on the whole crop and writes DIRS/metrics.json,
DIRS/metrics.txt (``FSS_<name>_thr<q>_n<n>: value`` and ``LSD_<name>: value`` lines), DIRS/scale_data.npz and DIRS/scale_panels.pdf.
It needs ``--mode radar``; the other outputs do not depend on it.

With ``--prob DIRP [--variance NAME=V.zarr ...] [--levels L ...] [--no-censor]`` it also runs the probabilistic verification
(run_prob) on the mode's pixels: every method "dressed" with its own in-sample MSE as the variance, and every method named by a
``--variance`` (a zarr of sigma^2 x output_scale^2 under the prediction's event keys, as ``scripts/infer.py --variance-output``
writes it) with its variance map.  Writes DIRP/metrics.json, DIRP/metrics.txt (``CRPS_<name>_<kind>: value``, ``COV90_...``,
``BRIER_..._thr<q>`` ... lines), DIRP/prob_data.npz and DIRP/prob_panels.pdf.  The other outputs do not depend on it.

With ``--objects DIRO [--connectivity {4,8}] [--sal-factor F] [--sal-floor Q]`` it also runs the object-based verification
(run_objects: the connected rain objects at ``--thresholds`` and at the relative level R >= max(F Rmax, Q), their population and SAL)
on the whole crop and writes DIRO/metrics.json, DIRO/metrics.txt (``SAL_<name>_<level>: S=.. A=.. L=..`` and ``OBJ_<name>_<level>:
pred=.. truth=..`` lines), DIRO/objects_data.npz and DIRO/objects_panels.pdf.  It needs ``--mode radar``; the other outputs do not
depend on it.

With ``--ens DIRE --ensemble NAME=MEMBERDIR [--ensemble ...] [--box-sizes S ...]`` it also runs the ensemble verification
(run_ensemble) on the mode's pixels: MEMBERDIR holds the ``member_%03d.zarr`` groups that ``scripts/infer.py --ensemble-output``
writes, every one with all of the truth's events.  Per ensemble and box size (box means on the 0-255 scale, not areal rain rates):
CRPS and fair CRPS, the rank histogram, spread against skill and the exceedance reliability; per ensemble the energy and variogram
scores.  Writes DIRE/metrics.json, DIRE/metrics.txt (``CRPSFAIR_<name>_box<s>: value``, ``ES_<name>``, ``VS_<name>`` ... lines),
DIRE/ens_data.npz and DIRE/ens_panels.pdf.  ``--ensemble`` without ``--ens`` is an argument error; the other outputs do not depend
on it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, List

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from p2igan_bench.data import zarr_lite  # noqa: E402
from p2igan_bench.evaluation import (DEFAULT_SCALES, DEFAULT_THRESHOLDS, crop_mask, run_exp1, run_exp2, run_exp2_paper_zarr,  # noqa: E402
                                     run_exp3, run_scale, write_scale_outputs)
from p2igan_bench.evaluation.objects import (DEFAULT_SAL_FACTOR, DEFAULT_SAL_FLOOR, run_objects, write_objects_outputs)  # noqa: E402
from p2igan_bench.evaluation.ensemble import DEFAULT_BOX_SIZES, run_ensemble, write_ens_outputs  # noqa: E402
from p2igan_bench.evaluation.prob import DEFAULT_LEVELS, half_width, pixel_threshold, run_prob, write_prob_outputs  # noqa: E402


def _method(spec: str):
    name, sep, path = spec.partition("=")
    if not sep or not name or not path:
        raise argparse.ArgumentTypeError(f"expected NAME=ZARR, got {spec!r}")
    return name, path


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="exp1 scores (MAE, RMSE, PSS, SSIM, dTSSIM, NSE, POD/FAR/CSI/HSS) of inference outputs")
    p.add_argument("--truth", required=True, help="zarr group of the truth events (uint8 or float, 0-255 scale)")
    p.add_argument("--method", type=_method, action="append", required=True, metavar="NAME=ZARR",
                   help="a method's prediction zarr (repeatable)")
    p.add_argument("--mask", required=True, help="mask .txt of the full domain (np.loadtxt)")
    p.add_argument("--mode", choices=("radar", "gauge"), default="radar")
    p.add_argument("--crop-size", type=int, default=128)
    p.add_argument("--no-pool8", action="store_true", help="SSIM / dTSSIM on the full-resolution crop")
    p.add_argument("--thresholds", type=float, nargs="+", default=list(DEFAULT_THRESHOLDS))
    p.add_argument("--output", required=True, help="output directory")
    p.add_argument("--device", default=None, help="torch device (default: the current GPU)")
    p.add_argument("--exp3", default=None, metavar="DIR", help="also run exp3 (NSE, scatter / residual panels, NSE boxplot, "
                   "log-frequency) and write its outputs into DIR")
    p.add_argument("--exp2", default=None, metavar="DIR", help="also write exp2's comparison GIFs, event_ranges.txt and exp2_data.npz "
                   "into DIR (needs --observation)")
    p.add_argument("--observation", default=None, metavar="OBS.zarr", help="zarr group of the observed events (exp2's Input / Gauge "
                   "panel and the paper grid's first two columns)")
    p.add_argument("--gif-fps", type=int, default=4, help="frames per second of exp2's GIFs")
    p.add_argument("--exp2-zoom", type=int, default=None, help="magnification of exp2's panels (default: at least 256 pixels wide)")
    p.add_argument("--exp2-pdf", default=None, metavar="FILE", help="also write exp2's paper frame grid to FILE (needs --observation "
                   "and --exp2-events)")
    p.add_argument("--exp2-events", default=None, metavar="JSON", help="the paper grid's events: a JSON list of "
                   "{event_id, select_idx, title}")
    p.add_argument("--scale", default=None, metavar="DIR", help="also run the scale-aware verification (FSS over thresholds x "
                   "neighbourhood sizes, radial power spectra) and write its outputs into DIR")
    p.add_argument("--scales", type=int, nargs="+", default=list(DEFAULT_SCALES), metavar="N", help="FSS neighbourhood sizes in pixels "
                   "(at most 16)")
    p.add_argument("--prob", default=None, metavar="DIR", help="also run the probabilistic verification (CRPS, PIT, coverage, "
                   "spread-skill, Brier / reliability / ROC) and write its outputs into DIR")
    p.add_argument("--variance", type=_method, action="append", default=[], metavar="NAME=ZARR",
                   help="the variance zarr of method NAME (repeatable; needs --prob)")
    p.add_argument("--levels", type=float, nargs="+", default=list(DEFAULT_LEVELS), metavar="L", help="nominal levels of the central "
                   "intervals (at most 8, each in (0, 1))")
    p.add_argument("--no-censor", action="store_true", help="score the plain Gaussian instead of the one left-censored at 0")
    p.add_argument("--ens", default=None, metavar="DIR", help="also run the ensemble verification (fair CRPS, rank histograms, "
                   "spread-skill and exceedance reliability of pixels and box means, energy and variogram scores) of every --ensemble into DIR")
    p.add_argument("--ensemble", type=_method, action="append", default=[], metavar="NAME=MEMBERDIR",
                   help="the directory of ensemble NAME's member_%%03d.zarr files, as infer.py --ensemble-output writes them "
                        "(repeatable; needs --ens)")
    p.add_argument("--box-sizes", type=int, nargs="+", default=list(DEFAULT_BOX_SIZES), metavar="S",
                   help="box sizes in pixels of the ensemble scores' points (1: pixels; means on the 0-255 scale)")
    p.add_argument("--objects", default=None, metavar="DIR", help="also run the object-based verification (connected rain objects, "
                   "their population, SAL) and write its outputs into DIR")
    p.add_argument("--connectivity", type=int, choices=(4, 8), default=8, help="pixel connectivity of the objects")
    p.add_argument("--sal-factor", type=float, default=DEFAULT_SAL_FACTOR, metavar="F", help="the relative level's share of the "
                   "frame's maximum (default 1/15)")
    p.add_argument("--sal-floor", type=float, default=DEFAULT_SAL_FLOOR, metavar="Q", help="the relative level's floor in mm/h "
                   "(default 0.1)")
    args = p.parse_args(argv)
    if args.objects and args.mode != "radar":
        p.error("--objects labels the whole crop: it needs --mode radar")
    if args.objects and not 0 < len(args.thresholds) <= 8:
        p.error("--thresholds takes 1 to 8 thresholds")
    if args.objects and not (0.0 < args.sal_factor <= 1.0 and args.sal_floor >= 0.0):
        p.error("--sal-factor lies in (0, 1] and --sal-floor is >= 0")
    if args.variance and not args.prob:
        p.error("--variance needs --prob")
    if args.ensemble and not args.ens:
        p.error("--ensemble needs --ens")
    if args.ens:
        if not args.ensemble:
            p.error("--ens needs at least one --ensemble")
        if len({n for n, _ in args.ensemble}) != len(args.ensemble):
            p.error("--ensemble names repeat")
        if not 0 < len(args.thresholds) <= 8:
            p.error("--thresholds takes 1 to 8 thresholds")
        if len(set(args.box_sizes)) != len(args.box_sizes) or any(not 1 <= s <= args.crop_size for s in args.box_sizes):
            p.error("--box-sizes takes distinct sizes in 1 .. the crop size")
        try:
            for q in args.thresholds:
                pixel_threshold(q, True)
        except ValueError as e:
            p.error(str(e))
    if args.prob:
        unknown = [n for n, _ in args.variance if n not in [m for m, _ in args.method]]
        if unknown:
            p.error(f"--variance names a method that no --method gives: {unknown}")
        if len({n for n, _ in args.variance}) != len(args.variance):
            p.error("--variance names repeat")
        if not 0 < len(args.levels) <= 8:
            p.error("--levels takes 1 to 8 levels")
        if not 0 < len(args.thresholds) <= 8:
            p.error("--thresholds takes 1 to 8 thresholds")
        try:
            for v in args.levels:
                half_width(v)
            for q in args.thresholds:
                pixel_threshold(q, True)
        except ValueError as e:
            p.error(str(e))
    if args.scale and args.mode != "radar":
        p.error("--scale scores the whole crop: it needs --mode radar")
    if args.scale and not 0 < len(args.scales) <= 16:
        p.error("--scales takes 1 to 16 sizes")
    if (args.exp2 or args.exp2_pdf) and not args.observation:
        p.error("--exp2 / --exp2-pdf need --observation")
    if args.exp2_pdf and not args.exp2_events:
        p.error("--exp2-pdf needs --exp2-events")
    names = [n for n, _ in args.method]
    if len(set(names)) != len(names):
        p.error(f"method names repeat: {names}")
    return args


def load_events(path: str) -> Dict[str, np.ndarray]:
    g = zarr_lite.Group(path, "r")
    return {k: np.asarray(g[k][:]) for k in sorted(g.array_keys())}


def load_mask(path: str, crop_size: int) -> np.ndarray:
    return crop_mask(np.loadtxt(path).astype(bool), crop_size)


def check_events(truth_keys: List[str], method: str, keys) -> None:
    missing = [k for k in truth_keys if k not in keys]
    if missing:
        raise ValueError(f"method {method!r} lacks truth event {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))


def load_members(path: str, truth_keys: List[str]) -> Dict[str, List[np.ndarray]]:
    """{event: [member 0's array, member 1's, ...]} of the member_%03d.zarr groups under ``path`` (infer.py --ensemble-output)."""
    names = sorted(n for n in os.listdir(path) if n.startswith("member_") and n.endswith(".zarr"))
    if not names or names != [f"member_{k:03d}.zarr" for k in range(len(names))]:
        raise SystemExit(f"{path}: expected member_000.zarr .. member_<M-1>.zarr, found {names[:4]}")
    events = {k: [] for k in truth_keys}
    for n in names:
        g = zarr_lite.Group(os.path.join(path, n), "r")
        try:
            check_events(truth_keys, n, set(g.array_keys()))
        except ValueError as e:
            raise SystemExit(f"{os.path.join(path, n)}: {e}")
        for k in truth_keys:
            events[k].append(np.asarray(g[k][:]))
    return events


def check_output_scale(name: str, pred_attrs, var_attrs) -> None:
    """The variance is sigma^2 x output_scale^2 of the prediction's scale: where both zarrs record an output_scale they must agree."""
    a, b = pred_attrs.get("output_scale"), var_attrs.get("output_scale")
    if a is not None and b is not None and float(a) != float(b):
        raise ValueError(f"method {name!r}: the prediction was written with output_scale {a}, its variance with {b}")


def format_lines(metrics) -> List[str]:
    """main.py's metrics.txt layout: [method], `key: value` with 6 decimals, nested `key:` / `  sub: value`, a blank line."""
    lines = []
    for name, vals in metrics.items():
        lines.append(f"[{name}]")
        for k, v in vals.items():
            if isinstance(v, dict):
                lines.append(f"{k}:")
                for sk, sv in v.items():
                    lines.append(f"  {sk}: {sv:.6f}")
            else:
                lines.append(f"{k}: {v:.6f}")
        lines.append("")
    return lines


def write_outputs(out_dir: str, metrics) -> None:
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "metrics.json"), "w", encoding="utf-8") as f:
        json.dump(metrics, f, indent=2, sort_keys=True)
    with open(os.path.join(out_dir, "metrics.txt"), "w", encoding="utf-8") as f:
        for line in format_lines(metrics):
            f.write(line.rstrip() + "\n")


def write_exp3_outputs(out_dir: str, metrics) -> None:
    """main.py's exp3 files: metrics.json (indent 2, sorted keys) and metrics.txt (`key: value` with 6 decimals)."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "metrics.json"), "w", encoding="utf-8") as f:
        json.dump(metrics, f, indent=2, sort_keys=True)
    with open(os.path.join(out_dir, "metrics.txt"), "w", encoding="utf-8") as f:
        for k, v in metrics.items():
            f.write(f"{k}: {v:.6f}\n")


def main(argv=None):
    args = parse_args(argv)
    truth = load_events(args.truth)
    if not truth:
        raise SystemExit(f"{args.truth}: no events")
    preds = {}
    for name, path in args.method:
        g = zarr_lite.Group(path, "r")
        keys = set(g.array_keys())
        try:
            check_events(list(truth), name, keys)
        except ValueError as e:
            raise SystemExit(f"{path}: {e}")
        preds[name] = {k: np.asarray(g[k][:]) for k in truth}
    mask = load_mask(args.mask, args.crop_size)
    metrics = run_exp1(preds, truth, mask, args.mode, args.crop_size, thresholds=tuple(args.thresholds),
                       use_pool8=not args.no_pool8, divide_by_3=True, device=args.device)
    write_outputs(args.output, metrics)
    print(f"wrote {os.path.join(args.output, 'metrics.json')} ({len(metrics)} methods)")
    if args.exp3:
        m3 = run_exp3(preds, truth, mask, args.mode, args.crop_size, args.exp3, device=args.device)
        write_exp3_outputs(args.exp3, m3)
        print(f"wrote {os.path.join(args.exp3, 'metrics.json')} and the exp3 figures")
    if args.scale:
        ms = run_scale(preds, truth, args.crop_size, thresholds=tuple(args.thresholds), scales=tuple(args.scales), divide_by_3=True,
                       device=args.device, mode=args.mode)
        write_scale_outputs(args.scale, ms)
        print(f"wrote {os.path.join(args.scale, 'metrics.json')} and the scale figure")
    if args.objects:
        frames = {}
        mo = run_objects(preds, truth, args.crop_size, thresholds=tuple(args.thresholds), connectivity=args.connectivity,
                         sal_factor=args.sal_factor, sal_floor=args.sal_floor, divide_by_3=True, device=args.device, mode=args.mode,
                         frames_out=frames)
        write_objects_outputs(args.objects, mo, frames)
        print(f"wrote {os.path.join(args.objects, 'metrics.json')} and the SAL diagrams")
    paths = {name: path for name, path in args.method}
    if args.prob:
        variances = {}
        for name, path in args.variance:
            g = zarr_lite.Group(path, "r")
            try:
                check_events(list(truth), name, set(g.array_keys()))
                check_output_scale(name, zarr_lite.Group(paths[name], "r").attrs, g.attrs)
            except ValueError as e:
                raise SystemExit(f"{path}: {e}")
            variances[name] = {k: np.asarray(g[k][:]) for k in truth}
        mp = run_prob(preds, variances, truth, mask, args.mode, args.crop_size, thresholds=tuple(args.thresholds),
                      levels=tuple(args.levels), censor=not args.no_censor, divide_by_3=True, device=args.device)
        write_prob_outputs(args.prob, mp)
        print(f"wrote {os.path.join(args.prob, 'metrics.json')} and the probability figure")
    if args.ens:
        me = run_ensemble({name: load_members(path, list(truth)) for name, path in args.ensemble}, truth, mask, args.mode, args.crop_size,
                          box_sizes=tuple(args.box_sizes), thresholds=tuple(args.thresholds), divide_by_3=True, device=args.device)
        write_ens_outputs(args.ens, me)
        print(f"wrote {os.path.join(args.ens, 'metrics.json')} and the ensemble figure")
    if args.exp2:
        run_exp2(paths, args.truth, args.observation, mask, args.exp2, args.crop_size, None, 0.0, 0.0, args.gif_fps, divide_by_3=True,
                 mode=args.mode, device=args.device, zoom=args.exp2_zoom)
        print(f"wrote {os.path.join(args.exp2, 'event_ranges.txt')} and the exp2 GIFs")
    if args.exp2_pdf:
        with open(args.exp2_events, encoding="utf-8") as f:
            events = json.load(f)
        out_dir, name = os.path.split(os.path.abspath(args.exp2_pdf))
        run_exp2_paper_zarr(args.observation, paths, events, args.mask, args.crop_size, out_dir, name, device=args.device)
        print(f"wrote {args.exp2_pdf}")


if __name__ == "__main__":
    main()
