"""Leave-one-out (LOO) gauge cross-validation of the classical baselines over the test events (no counterpart in
the reference): the one score that needs no gridded truth, so the one that also holds on gauge-only data.  Every gauge of a frame is
predicted from the frame's other gauges by the model's ``cross_validate`` (csrc/krig_uq.hip); the sums behind the scores are taken on
the device, chunk by chunk, and added per event and overall on the host.

Leave-one-site-out (LOSO; csrc/stkrig_loso.hip) is the same loop over the models' ``cross_validate_sites``: a
site (a gauge pixel in all frames of a chunk) is left out as a whole.  It is the score of the space-time baselines `stkriging` and
`lagkriging`, whose point-wise LOO would flatter them, and of `localkriging` and `locallagkriging`, which score it with their own kernel and take
chunks of any length; for `kriging` and `idw` it equals LOO and puts all in one table over the same targets."""
from __future__ import annotations

import json
import math
import os
from typing import Any, Dict, Optional

import numpy as np
import torch

from ._common import transform_mmhr

def _coded(sums, with_var: bool, scale: float) -> Dict[str, float]:
    from ..models.classical import loo_summary
    out = loo_summary(sums, with_var)
    for k in ("ME", "MAE", "RMSE"):
        out[k] *= scale
    return out


def _mmhr(z, pred, scale: float) -> Dict[str, float]:
    """ME / MAE / RMSE of the rain rates: the evaluation's transform on z and on the LOO prediction (coded units x scale), then e."""
    if len(z) == 0:
        return {"ME_mmhr": math.nan, "MAE_mmhr": math.nan, "RMSE_mmhr": math.nan}
    e = transform_mmhr(z.astype(np.float64) * scale) - transform_mmhr(pred.astype(np.float64) * scale)
    return {"ME_mmhr": float(e.mean()), "MAE_mmhr": float(np.abs(e).mean()), "RMSE_mmhr": float(np.sqrt((e * e).mean()))}


def loo_lines(result: Dict[str, Any], title: str = "leave-one-out"):
    """The text table of a run_loo result."""
    keys = ["n", "ME", "MAE", "RMSE"] + (["MSDR"] if "MSDR" in result["overall"] else []) + ["ME_mmhr", "MAE_mmhr", "RMSE_mmhr"]
    lines = [f"{title} cross-validation: {result['model_name']}  (coded units x {result['output_scale']:g}; *_mmhr in mm/h)",
             "event".ljust(12) + "".join(k.rjust(14) for k in keys)]
    for name, row in list(result["events"].items()) + [("overall", result["overall"])]:
        lines.append(name.ljust(12) + "".join((f"{row[k]:d}" if k == "n" else f"{row[k]:.6g}").rjust(14) for k in keys))
    return lines


def loso_lines(result: Dict[str, Any]):
    """The text table of a run_loso result."""
    return loo_lines(result, "leave-one-site-out")


def _has_variance(name: str, by_site: bool) -> bool:
    from ..models.classical import LOCAL, SPACE_TIME
    return name == "kriging" or (by_site and (name in SPACE_TIME or name in LOCAL))


def check_prob(cfg: Dict[str, Any], by_site: bool) -> None:
    """The probabilistic verification of a cross-validation scores N(pred, var): RuntimeError for a run without a variance."""
    name = str(cfg.get("model", {}).get("name", "model")).lower()
    if not _has_variance(name, by_site):
        raise RuntimeError(f"--prob scores the predictive distribution N(pred, var) of a cross-validation: model.name '{name}' "
                           f"{'leave-one-site-out' if by_site else 'leave-one-out'} has no variance")


def run_loo(cfg: Dict[str, Any], out_dir, device: Optional[str] = None, output_scale: float = 255.0, stride: int = 16,
            prob: bool = False) -> Dict[str, Any]:
    """Cross-validate cfg's classical model on every test event, in consecutive chunks of `stride` frames as infer_event_chunks forms
    them (each chunk is one sample of a fitted variogram).  Writes loo.json / loo.txt (scores per event and overall) and loo_data.npz
    (per gauge: event, frame, y, x, z, LOO prediction, LOO variance; coded units, unscaled) under out_dir; returns loo.json's content."""
    from ..models import CLASSICAL
    from ..models.classical import LOCAL, SPACE_TIME
    name = str(cfg.get("model", {}).get("name", "model")).lower()
    if name not in CLASSICAL:
        raise RuntimeError(f"leave-one-out cross-validation is defined for the classical baselines {sorted(set(CLASSICAL) - set(SPACE_TIME) - set(LOCAL))} only: "
                           f"model.name '{name}' is a learnt model and would need one training per gauge")
    if name in SPACE_TIME:
        from ..models.classical import LAG_NO_LOO, ST_NO_LOO
        raise RuntimeError(ST_NO_LOO if name == "stkriging" else LAG_NO_LOO)
    if name in LOCAL:
        from ..models.classical import LOCAL_LAG_NO_LOO, LOCAL_NO_LOO
        raise RuntimeError(LOCAL_NO_LOO if name == "localkriging" else LOCAL_LAG_NO_LOO)
    return _run(cfg, out_dir, device, output_scale, stride, name, False, prob)


def run_loso(cfg: Dict[str, Any], out_dir, device: Optional[str] = None, output_scale: float = 255.0, stride: int = 16,
             prob: bool = False) -> Dict[str, Any]:
    """run_loo with whole sites left out (the models' cross_validate_sites), for all classical baselines.  A chunk of `stride`
    frames is one sample, so a site is a gauge pixel over the chunk's frames; `stkriging` and `lagkriging` take chunks of at most 32 frames.  Writes
    loso.json / loso.txt and loso_data.npz (loo_data.npz's columns plus site, the site's index within its chunk) under out_dir."""
    from ..models import CLASSICAL
    from ..models.classical import SPACE_TIME
    from .. import ops
    name = str(cfg.get("model", {}).get("name", "model")).lower()
    if name not in CLASSICAL:
        raise RuntimeError(f"leave-one-site-out cross-validation is defined for the classical baselines {sorted(CLASSICAL)} only: "
                           f"model.name '{name}' is a learnt model and would need one training per site")
    if name in SPACE_TIME and int(stride) > ops.KRIG_TILE:
        raise ValueError(f"leave-one-site-out of '{name}' takes chunks of at most {ops.KRIG_TILE} frames: --stride {int(stride)} is too long")
    return _run(cfg, out_dir, device, output_scale, stride, name, True, prob)


def _run(cfg, out_dir, device, output_scale, stride, name, by_site, prob=False):
    from ..models import build_generator
    if prob:
        check_prob(cfg, by_site)
    dev = torch.device(device or cfg.get("device", "cuda:0"))
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("the MI355X path needs a GPU: there is no CPU fallback")
    from ..data.dataloader import P2IDataModule
    loader = P2IDataModule(cfg).test_dataloader()
    if loader is None or len(loader.dataset) == 0:
        raise RuntimeError("Test dataloader is not configured or empty.")
    G = build_generator(cfg).to(dev).eval()
    scale, stride = float(output_scale), max(1, int(stride))
    with_var = _has_variance(name, by_site)
    stem = "loso" if by_site else "loo"
    events, cols = {}, {k: [] for k in ("event", "frame", "y", "x", "z", "pred", "var") + (("site",) if by_site else ())}
    total = np.zeros(5)
    for ei, batch in enumerate(loader):
        _, masked, masks = [t.permute(0, 1, 4, 2, 3).contiguous().to(dev) for t in batch]
        sums, ez, ep = np.zeros(5), [], []
        for s in range(0, masked.shape[1], stride):
            res = (G.cross_validate_sites if by_site else G.cross_validate)(masked[:, s:s + stride].contiguous(),
                                                                            masks[:, s:s + stride].contiguous())
            site = res.site.cpu().numpy() if by_site else None
            sums += np.asarray(res.sums().cpu().tolist())
            counts = res.counts.cpu().numpy()
            pix, z, pred = res.pix.cpu().numpy(), res.z.cpu().numpy(), res.pred.cpu().numpy()
            var = res.var.cpu().numpy() if with_var else np.full(z.shape, np.nan, np.float32)
            for f, n in enumerate(counts):
                n = min(int(n), z.shape[1])
                cols["event"].append(np.full(n, ei + 1, np.int32))
                cols["frame"].append(np.full(n, s + f, np.int32))
                cols["y"].append((pix[f, :n] >> 16).astype(np.int32))
                cols["x"].append((pix[f, :n] & 0xffff).astype(np.int32))
                cols["z"].append(z[f, :n])
                cols["pred"].append(pred[f, :n])
                cols["var"].append(var[f, :n])
                if by_site:
                    cols["site"].append(site[f, :n])
                ok = ~np.isnan(pred[f, :n]) & (~np.isnan(var[f, :n]) if with_var else True)
                ez.append(z[f, :n][ok])
                ep.append(pred[f, :n][ok])
        ez, ep = np.concatenate(ez), np.concatenate(ep)
        events[f"event_{ei + 1:02d}"] = {**_coded(sums.tolist(), with_var, scale), **_mmhr(ez, ep, scale)}
        total += sums
    data = {k: np.concatenate(v) for k, v in cols.items()}
    ok = ~np.isnan(data["pred"]) & (~np.isnan(data["var"]) if with_var else True)
    result = {"model_name": name, "output_scale": scale, "stride": stride, "events": events,
              "overall": {**_coded(total.tolist(), with_var, scale), **_mmhr(data["z"][ok], data["pred"][ok], scale)}}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{stem}.json"), "w") as fh:
        json.dump(result, fh, indent=2)
    with open(os.path.join(out_dir, f"{stem}.txt"), "w") as fh:
        fh.write("\n".join(loso_lines(result) if by_site else loo_lines(result)) + "\n")
    np.savez(os.path.join(out_dir, f"{stem}_data.npz"), **data)
    if prob:
        # prob.json / prob.txt / prob_data.npz: the columns' N(pred, var) against z on the output scale (points without a prediction
        # or a variance carry NaN and are counted as skipped)
        from .prob import run_prob_points, write_prob_outputs
        write_prob_outputs(out_dir, run_prob_points(data["z"], data["pred"], data["var"], scale, name=name, device=dev), stem="prob",
                           figure=False)
    return result
