#!/usr/bin/env python3
"""Sliding-window inference on the MI355X path; CLI flags, checkpoint resolution and the output
Zarr group follow the reference's scripts/infer.py:20-40,61-80,168-180,247-257."""
from __future__ import annotations

import argparse
import json
import logging
import os
import shutil
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from p2igan_bench.data import zarr_lite  # noqa: E402
from p2igan_bench.data.dataloader import P2IDataModule  # noqa: E402
from p2igan_bench.inference import infer_event, infer_event_chunks, infer_event_ensemble, infer_event_variance  # noqa: E402
from p2igan_bench.models import CLASSICAL, build_generator  # noqa: E402
from p2igan_bench.models.classical import LOCAL  # noqa: E402

VARIANCE_MODELS = ("kriging",) + LOCAL          # the models with a forward_uq
ENSEMBLE_MODELS = ("kriging", "stkriging")      # the models with a conditional simulation (forward_ensemble, forward_simulation)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Inference for P2I-GAN benchmark models")
    p.add_argument("--config", type=Path, default=Path("p2igan_bench/config/p2igan_baseline.json"))
    p.add_argument("--checkpoint", type=Path, default=None)
    p.add_argument("--model-dir", type=Path, default=None)
    p.add_argument("--data-root", type=Path, default=None)
    p.add_argument("--output", type=Path, default=None)
    p.add_argument("--passes", type=int, default=1)
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--log-every", type=int, default=50)
    p.add_argument("--stride", type=int, default=16)
    p.add_argument("--overlap", type=int, default=12)
    p.add_argument("--output-scale", type=float, default=255.0)
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--variance-output", type=Path, default=None,
                   help="kriging, localkriging and locallagkriging only: a second zarr with the kriging variance x output-scale^2 under the same event keys")
    p.add_argument("--ensemble-output", type=Path, default=None,
                   help="kriging and stkriging only: a directory of member_%%03d.zarr, the conditional-simulation members laid out as "
                        "--output is (stkriging: coherent in time within a chunk of --stride frames)")
    p.add_argument("--members", type=int, default=None, help="ensemble members per frame (1..64), with --ensemble-output")
    p.add_argument("--ensemble-seed", type=int, default=0)
    p.add_argument("--log-level", type=str, default="INFO")
    return p.parse_args(argv)


def resolve_checkpoint(cfg, args) -> Path:
    if args.checkpoint:
        return args.checkpoint
    base = Path(args.model_dir or cfg.get("save_dir", "weights"))
    if base.is_file():
        return base
    if (base / "latest.pt").exists():
        return base / "latest.pt"
    if base.exists():
        cands = sorted(base.glob("*.pt"), key=lambda p: p.stat().st_mtime, reverse=True)
        if cands:
            logging.warning("latest.pt not found, falling back to %s", cands[0])
            return cands[0]
    raise FileNotFoundError(f"Checkpoint not found under {base}")


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper(), logging.INFO), format="%(asctime)s | %(levelname)s | %(message)s")
    with args.config.open() as f:
        cfg = json.load(f)
    if args.ensemble_output is not None:         # refused before the device, the data or a checkpoint is touched
        asked = cfg.get("model", {}).get("name", "model")
        if str(asked).lower() not in ENSEMBLE_MODELS:
            raise RuntimeError(f"--ensemble-output needs model.name 'kriging' or 'stkriging', the models with a conditional simulation "
                               f"(got '{asked}')")
        if args.members is None or not 1 <= args.members <= 64:
            raise ValueError(f"--ensemble-output needs --members in 1..64 (got {args.members})")
    elif args.members is not None:
        raise ValueError("--members needs --ensemble-output")
    torch.manual_seed(cfg.get("seed", 42))
    np.random.seed(cfg.get("seed", 42))
    if args.data_root is not None:
        cfg.setdefault("data", {}).setdefault("test", {})["data_root"] = str(args.data_root)
    dev = torch.device(args.device or cfg.get("device", "cuda:0"))
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("the MI355X path needs a GPU: there is no CPU fallback")
    name = cfg.get("model", {}).get("name", "model")
    classical = str(name).lower() in CLASSICAL         # parameter-free: no checkpoint to resolve or load
    if args.variance_output is not None and str(name).lower() not in VARIANCE_MODELS:
        raise RuntimeError(f"--variance-output needs model.name 'kriging', 'localkriging' or 'locallagkriging', the models with a variance "
                           f"(got '{name}')")
    ckpt = None if classical else resolve_checkpoint(cfg, args)
    loader = P2IDataModule(cfg).test_dataloader()
    if loader is None or len(loader.dataset) == 0:
        raise RuntimeError("Test dataloader is not configured or empty.")
    out = Path(args.output or Path(args.model_dir or cfg.get("save_dir", "weights")) / f"test{name}.zarr")
    if out.exists():
        if not args.overwrite:
            raise FileExistsError(f"Output already exists: {out}")
        shutil.rmtree(out)
    if args.variance_output is not None and args.variance_output.exists():
        if not args.overwrite:
            raise FileExistsError(f"Output already exists: {args.variance_output}")
        shutil.rmtree(args.variance_output)
    if args.ensemble_output is not None and args.ensemble_output.exists():
        if not args.overwrite:
            raise FileExistsError(f"Output already exists: {args.ensemble_output}")
        shutil.rmtree(args.ensemble_output)
    group = zarr_lite.Group(str(out), "w")
    group.attrs.update({"config_path": str(args.config), "checkpoint": None if ckpt is None else str(ckpt), "model_name": name,
                        "data_root": cfg.get("data", {}).get("test", {}).get("data_root"), "passes": int(args.passes),
                        "output_scale": float(args.output_scale)})
    G = build_generator(cfg).to(dev)
    if not classical:
        state = torch.load(ckpt, map_location=dev, weights_only=True)
        G.load_state_dict(state["generator"] if isinstance(state, dict) and "generator" in state else state)
    G.eval()
    results, variances, ensembles, clip_max = {}, {}, {}, 0.0
    for p in range(max(1, args.passes)):
        t0 = time.time()
        for i, batch in enumerate(loader):
            _, masked, masks = [t.permute(0, 1, 4, 2, 3).contiguous().to(dev) for t in batch]
            if classical:       # consecutive chunks of --stride frames, no overlap: each chunk is one sample of the variogram fit
                comp = infer_event_chunks(G, masked, masks, max(1, args.stride), args.output_scale).cpu().numpy()
            else:
                comp = infer_event(G, masked, masks, max(1, args.stride), max(0, args.overlap), args.output_scale).cpu().numpy()
            key = f"event_{i + 1:02d}"
            if args.variance_output is not None and p == 0:       # a function of gauge positions and variogram: the same every pass
                variances[key] = infer_event_variance(G, masked, masks, max(1, args.stride), args.output_scale).cpu().numpy()
            if args.ensemble_output is not None and p == 0:       # a function of (seed, event, frame, member): the same every pass
                ens = infer_event_ensemble(G, masked, masks, args.members, args.ensemble_seed, i, max(1, args.stride), args.output_scale)
                ensembles[key] = ens.clamp(min=0.0).cpu().numpy()
                clip = G.last_ensemble["clip"]
                clip_max = max(clip_max, float(clip[~clip.isnan()].max()) if bool((~clip.isnan()).any()) else 0.0)
            results[key] = comp if p == 0 else results[key] + (comp - results[key]) / float(p + 1)
            if (i + 1) % max(1, args.log_every) == 0:
                logging.info("Pass %d | %d samples | %.2f samples/sec", p + 1, i + 1, (i + 1) / max(time.time() - t0, 1e-6))
    for key, comp in results.items():
        group.create_dataset(key, comp.astype(np.float32), chunks=comp.shape)
    if args.variance_output is not None:
        vgroup = zarr_lite.Group(str(args.variance_output), "w")
        vgroup.attrs.update({"config_path": str(args.config), "model_name": name, "quantity": "kriging_variance",
                             "data_root": cfg.get("data", {}).get("test", {}).get("data_root"), "output_scale": float(args.output_scale)})
        for key, v in variances.items():
            vgroup.create_dataset(key, v.astype(np.float32), chunks=v.shape)
        logging.info("Kriging variance saved to %s", args.variance_output)
    if args.ensemble_output is not None:
        for m in range(args.members):
            mgroup = zarr_lite.Group(str(args.ensemble_output / f"member_{m:03d}.zarr"), "w")
            extra = {"embed_time": int(G.embed_time)} if hasattr(G, "embed_time") else {}      # stkriging: the torus' temporal side
            mgroup.attrs.update(dict(group.attrs, member=m, members=int(args.members), seed=int(args.ensemble_seed), embed=int(G.embed),
                                     clip_share_max=clip_max, **extra))
            for key, ens in ensembles.items():
                comp = np.ascontiguousarray(ens[:, m:m + 1])
                mgroup.create_dataset(key, comp.astype(np.float32), chunks=comp.shape)
        logging.info("%d ensemble members saved to %s", args.members, args.ensemble_output)
    logging.info("Inference completed. Output saved to %s", out)


if __name__ == "__main__":
    main()
