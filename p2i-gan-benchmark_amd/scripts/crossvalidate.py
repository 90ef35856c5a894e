#!/usr/bin/env python3
"""Leave-one-out gauge cross-validation of a classical baseline (model.name: kriging / idw) over the test events: every gauge is
predicted from the other gauges of its frame, which needs no gridded truth.  Writes loo.json, loo.txt and loo_data.npz
(p2igan_bench/evaluation/loo.py).  The space-time baselines `stkriging` and `lagkriging` are refused there:
their honest score is leave-one-site-out, --by-site: a site, a gauge pixel over all frames of a chunk of
--stride frames, is left out as a whole.  --by-site takes kriging, idw, stkriging and lagkriging (the last two in chunks of at
most 32 frames) and localkriging and locallagkriging (chunks of any length; they too are refused without --by-site) and writes loso.json, loso.txt and
loso_data.npz.  --prob additionally scores the columns' predictive distributions N(pred, var) (p2igan_bench/evaluation/prob.py, DESIGN.md
section 22) and writes prob.json, prob.txt and prob_data.npz; it needs a run that has a variance and is refused otherwise."""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from p2igan_bench.evaluation import loo_lines, loso_lines, run_loo, run_loso  # noqa: E402
from p2igan_bench.evaluation.loo import check_prob  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Leave-one-out cross-validation of the classical baselines")
    p.add_argument("--config", type=Path, required=True)
    p.add_argument("--data-root", type=Path, default=None)
    p.add_argument("--output", type=Path, required=True)
    p.add_argument("--stride", type=int, default=16)
    p.add_argument("--by-site", action="store_true", help="leave whole sites out (leave-one-site-out); the score of stkriging and lagkriging")
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--output-scale", type=float, default=255.0)
    p.add_argument("--prob", action="store_true", help="also write prob.json, prob.txt and prob_data.npz: the probabilistic "
                   "verification of the collected columns (runs with a variance only)")
    p.add_argument("--log-level", type=str, default="INFO")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper(), logging.INFO), format="%(asctime)s | %(levelname)s | %(message)s")
    with args.config.open() as f:
        cfg = json.load(f)
    torch.manual_seed(cfg.get("seed", 42))          # the masks are drawn from the global generators, as in infer.py
    np.random.seed(cfg.get("seed", 42))
    if args.data_root is not None:
        cfg.setdefault("data", {}).setdefault("test", {})["data_root"] = str(args.data_root)
    run, lines = (run_loso, loso_lines) if args.by_site else (run_loo, loo_lines)
    kw = {}
    if args.prob:
        check_prob(cfg, args.by_site)
        kw["prob"] = True
    result = run(cfg, str(args.output), device=args.device, output_scale=args.output_scale, stride=args.stride, **kw)
    for line in lines(result):
        logging.info("%s", line)
    return result


if __name__ == "__main__":
    main()
