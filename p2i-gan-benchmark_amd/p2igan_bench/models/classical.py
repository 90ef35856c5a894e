"""Classical, parameter-free baselines on the HIP path: ordinary kriging and all-gauge IDW of every frame's own gauges
(csrc/classical.hip).  The reference has no such method; they give the comparison table its non-learnt rows.

Both take the generators' (masked_frames, masks) pair, (B, T, 1, H, W) fp32 on the device, and return (B, T, 1, H, W).  The gauges
of frame (b, t) are its pixels with mask != 0 in raster order, their values masked_frames there, their coordinates pixel indices.
Neither has parameters (state_dict() is empty) and both are deterministic from run to run.

Uncertainty and validation (csrc/krig_uq.hip): KrigingGenerator.forward_uq adds the kriging variance map, and
cross_validate of either model predicts every gauge from the frame's other gauges (leave-one-out) and scores the residuals.

Conditional simulation (csrc/krig_cs.hip): KrigingGenerator.forward_ensemble adds ensemble members, fields that
carry the fitted variogram's texture and equal the gauge values at the gauge pixels; their mean and variance at a pixel are the
kriging mean and variance.

Space-time kriging (csrc/stkrig.hip): SpaceTimeKrigingGenerator kriges every pixel of every frame of a sample
from all gauges of all frames of that sample, one system per sample, with a metric space-time covariance.  Its truth-free score is
leave-one-site-out (csrc/stkrig_loso.hip): cross_validate_sites of all models predicts every point of a
site (a gauge pixel in all the sample's frames) with the whole site left out.

Space-time conditional simulation (csrc/stkrig_cs.hip): SpaceTimeKrigingGenerator.forward_simulation adds
ensemble members that are one Gaussian field over the whole sample: they equal the gauge values in every frame and their noise is
correlated from frame to frame as the space-time covariance says.

Lagrangian space-time kriging (csrc/lagkrig.hip for the velocity, csrc/stkrig.hip's kernels with it):
LagrangianKrigingGenerator measures the space-time distance in the frame that moves with the rain, with an advection velocity per
sample that it estimates from the gauges.

Moving-neighbourhood space-time kriging (csrc/lkrig.hip): LocalKrigingGenerator predicts every target from its
k nearest points in the space-time metric, from a small system of its own: no limit on the points of a sample, the kriging variance
and leave-one-site-out from the same kernel.  LocalLagrangianKrigingGenerator is the same in the Lagrangian
frame: the neighbours are the nearest in the frame that moves with the rain, where a site's copies in other frames are new support."""
from __future__ import annotations

import logging
import math
from typing import Any, Dict

import torch
import torch.nn as nn

from .. import ops

_FACTOR_BYTES = 1 << 30          # the factor workspace of one chunk of systems stays under this


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _frames(masked_frames, masks, who):
    if masked_frames.dim() != 5 or masked_frames.shape[2] != 1:
        raise RuntimeError(f"{who} takes (B, T, 1, H, W) frames")
    if masks.shape != masked_frames.shape:
        raise RuntimeError(f"{who}: masks shape {tuple(masks.shape)} differs from the frames' {tuple(masked_frames.shape)}")
    if not (masked_frames.is_cuda and masks.is_cuda):
        raise RuntimeError(f"{who} runs on the HIP path only (CUDA tensors)")
    b, t, _, h, w = masked_frames.shape
    return masked_frames.reshape(b, t, h, w).contiguous().float(), masks.reshape(b, t, h, w).contiguous().float()


class LOOResult:
    """Leave-one-out cross-validation of one call.  pix, z, pred, var: (B*T, cap) on the device, rows as ops.krig_compact packs them
    (pred is NaN where a frame has no model or fewer than 2 gauges, everything is 0 past the frame's count; var is None for IDW);
    counts (B*T,) int32; status: the kriging systems' factorisation flags (None for IDW).  site (cross_validate_sites only, else
    None): (B*T, cap) int32, the rank of the gauge's pixel among the sample's distinct gauge pixels in raster order, -1 past the count."""

    def __init__(self, pix, z, pred, var, counts, status, site=None):
        self.pix, self.z, self.pred, self.var, self.counts, self.status, self.site = pix, z, pred, var, counts, status, site

    def sums(self) -> torch.Tensor:
        """(5,) fp64 on the device: n, sum e, sum |e|, sum e^2, sum e^2 / var over the gauges with a prediction, e = z - pred."""
        return ops.loo_scores(self.z, self.pred, self.var, self.counts)

    def scores(self) -> Dict[str, float]:
        """n, ME, MAE, RMSE (and MSDR = mean(e^2 / var) where there is a variance) of those gauges."""
        return loo_summary(self.sums().cpu().tolist(), self.var is not None)


def loo_summary(sums, with_var: bool) -> Dict[str, float]:
    """The scores of ops.loo_scores' sums (n, sum e, sum |e|, sum e^2, sum e^2 / var); NaN when no gauge has a prediction."""
    n = int(sums[0])
    d = float(n) if n else math.nan
    out = {"n": n, "ME": sums[1] / d, "MAE": sums[2] / d, "RMSE": math.sqrt(sums[3] / d)}
    if with_var:
        out["MSDR"] = sums[4] / d
    return out


def _sites_of_frames(res: LOOResult, masks) -> LOOResult:
    """res with its site field filled for a model whose systems are per frame (leaving a site out is leaving a gauge out there): the
    rank of each gauge's pixel in the raster-order union of the sample's masks."""
    b, t, _, h, w = masks.shape
    union = (masks.reshape(b, t, h * w) != 0).any(dim=1)
    rank = (torch.cumsum(union, dim=1, dtype=torch.int32) - 1).to(torch.int32)
    pix = res.pix.view(b, t * res.pix.shape[1]).long()
    site = torch.gather(rank, 1, (pix >> 16) * w + (pix & 0xffff)).view_as(res.pix)
    past = torch.arange(res.pix.shape[1], device=site.device)[None, :] >= res.counts[:, None]
    res.site = site.masked_fill(past, -1).contiguous()
    return res


class _Systems:
    """The workspace of one call's nsys kriging systems of padded size np_, factored `per` at a time so that the factors (and, with
    inverse, their inverses: two workspaces per system) of one chunk stay under _FACTOR_BYTES; `limit` bounds the chunk further.
    work / winv: the chunk's factors / inverses; status (nsys,), alpha (rows, cap) and mean (rows,) span the whole call.
    pix, z, info, params, cand, model, r, t: the call's systems as ops.KrigSystems takes them (it checks them once, here)."""

    def __init__(self, pix, z, info, params, cand, model, r, t, np_, inverse=False, limit=None):
        rows, cap = pix.shape
        nsys, dev = rows // r, pix.device
        per = max(1, min(nsys, _FACTOR_BYTES // (np_ * np_ * 4 * (2 if inverse else 1))))
        if limit is not None:
            per = max(1, min(per, limit))
        self.nsys, self.per = nsys, per
        self.work = torch.empty(per * np_ * np_, device=dev, dtype=torch.float32)
        self.winv = torch.empty(per * np_ * np_, device=dev, dtype=torch.float32) if inverse else None
        self.status = torch.zeros(nsys, device=dev, dtype=torch.int32)
        self.alpha = torch.empty(rows, cap, device=dev, dtype=torch.float32)
        self.mean = torch.empty(rows, device=dev, dtype=torch.float32)
        self.sys = ops.KrigSystems(pix, z, info, params, cand, model, r, t, np_, self.status)

    def chunks(self):
        """The descriptor (ops.KrigChunk: s0, ns, status) of every chunk."""
        for s0 in range(0, self.nsys, self.per):
            yield self.sys.chunk(s0, min(self.per, self.nsys - s0))

    def finish(self, model, warning, each=1):
        """Leaves status in model.last_status and logs `warning` with the failed systems times `each` (a host read)."""
        model.last_status = self.status
        failed = int(self.status.sum()) * each
        if failed:
            logging.warning(warning, failed)


def _variogram_config(self, mc, space_time=False):
    """model.variogram on `self`: variogram_model, fit, n_lags and, with fit=false, fixed = (nugget, psill, range); the space-time
    models add n_tlags and, to fixed, time_scale."""
    vg = dict(mc.get("variogram") or {})
    name = str(vg.get("model", "exponential")).lower()
    if name not in ops.KRIG_MODELS:
        raise ValueError(f"model.variogram.model must be one of {sorted(ops.KRIG_MODELS)} (got '{name}')")
    self.variogram_model = ops.KRIG_MODELS[name]
    self.fit = bool(vg.get("fit", True))
    self.n_lags = int(vg.get("n_lags", 16))
    if space_time:
        self.n_tlags = int(vg.get("n_tlags", 3))
    if self.fit:
        if not 1 <= self.n_lags <= ops.KRIG_MAX_LAGS:
            raise ValueError(f"model.variogram.n_lags must be in [1, {ops.KRIG_MAX_LAGS}] (got {self.n_lags})")
        if space_time and not 0 <= self.n_tlags <= ops.STKRIG_MAX_TLAGS:
            raise ValueError(f"model.variogram.n_tlags must be in [0, {ops.STKRIG_MAX_TLAGS}] (got {self.n_tlags})")
        return
    keys = ("nugget", "psill", "range") + (("time_scale",) if space_time else ())
    bounds = ["nugget >= 0"] + [f"{k} > 0" for k in keys[1:]]
    try:
        self.fixed = tuple(float(vg[k]) for k in keys)
    except KeyError as e:
        raise ValueError(f"model.variogram with fit=false needs {', '.join(keys[:-1])} and {keys[-1]} (missing {e})") from None
    if not (self.fixed[0] >= 0 and all(v > 0 for v in self.fixed[1:])):
        raise ValueError(f"model.variogram: {', '.join(bounds[:-1])} and {bounds[-1]} are required")


class _ClassicalBase(nn.Module):
    DEFAULT_MAX_POINTS = 1024

    def __init__(self, config: Dict[str, Any]):
        super().__init__()
        self.config = config
        mc = config.get("model", {})
        self.max_points = int(mc.get("max_points", self.DEFAULT_MAX_POINTS))
        if not 1 <= self.max_points <= ops.KRIG_MAX_CAP:
            raise ValueError(f"model.max_points must be in [1, {ops.KRIG_MAX_CAP}] (got {self.max_points})")

    def _compact(self, masked_frames, masks):
        """(pix, z, info, counts on the host, 'every sample's frames share their mask') -- the call's one host read."""
        x, m = _frames(masked_frames, masks, type(self).__name__)
        f = x.shape[0] * x.shape[1]
        pix, z, info = ops.krig_compact(x, m, _round_up(self.max_points, ops.KRIG_TILE))
        host = info.cpu()
        counts, differs = host[:f], host[f:]
        if int(counts.max()) > self.max_points:
            raise ValueError(f"{type(self).__name__}: a frame has {int(counts.max())} gauges, more than model.max_points = {self.max_points}")
        return pix, z, info, counts, not bool(differs.any())


class KrigingGenerator(_ClassicalBase):
    """Ordinary kriging with a global neighbourhood in its dual form, one system per frame (or per sample when its frames share
    their mask).  model.variogram = {"model": "exponential" | "spherical", "fit": true, "n_lags": 16} fits (nugget, psill, range)
    per sample on the device; {"model", "fit": false, "nugget", "psill", "range"} takes them as given.  model.ensemble = {"embed": 2}
    (2 to 4) sets the side of forward_ensemble's embedding torus in frame sides."""

    def __init__(self, config: Dict[str, Any]):
        super().__init__(config)
        mc = config.get("model", {})
        _variogram_config(self, mc)
        self.share_sets = bool(mc.get("share_sets", True))   # false: one factorisation per frame even where a sample shares its mask
        ens = mc.get("ensemble")
        if ens is not None and not isinstance(ens, dict):
            raise ValueError(f"model.ensemble must be a mapping such as {{\"embed\": 2}} (got {ens!r})")
        self.embed = (ens or {}).get("embed", 2)             # forward_ensemble: the torus is embed times the frame on a side
        if isinstance(self.embed, bool) or not isinstance(self.embed, int) or self.embed not in ops.KRIG_CS_EMBEDS:
            raise ValueError(f"model.ensemble.embed must be an integer in {list(ops.KRIG_CS_EMBEDS)} (got {self.embed!r})")
        self.last_fit = None         # {"bins", "fit", "cand"} device tensors of the last call (fit=true)
        self.last_status = None      # per-system int32 of the last call: 1 where the factorisation met a non-positive pivot
        self.last_ensemble = None    # {"clip": (B,) fp64 clip share of each sample's spectrum, "embed"} of the last forward_ensemble

    @torch.no_grad()
    def forward(self, masked_frames, masks):
        return self._krige(masked_frames, masks)["pred"]

    @torch.no_grad()
    def forward_ensemble(self, masked_frames, masks, members, seed=0, streams=None):
        """(prediction (B, T, 1, H, W), ensemble (B, T, members, H, W)) by conditional simulation.  The prediction
        is forward()'s.  Every member carries the variogram's texture and equals the gauge values at the gauge pixels; the members'
        mean and variance at a pixel are the kriging mean and variance.  Member m of a frame is a function of (seed, the frame's
        stream id, m, the variogram, the gauges) only; streams (B, T) int64 defaults to b T + t.  Members are raw Gaussian (they can be
        negative) and NaN over a frame without a model, as the variance is.  1 <= members <= 64."""
        if isinstance(members, bool) or not isinstance(members, int) or not 1 <= members <= ops.KRIG_CS_MAX_MEMBERS:
            raise ValueError(f"forward_ensemble: members must be an integer in [1, {ops.KRIG_CS_MAX_MEMBERS}] (got {members!r})")
        if masked_frames.dim() != 5:
            raise RuntimeError(f"{type(self).__name__}.forward_ensemble takes (B, T, 1, H, W) frames")
        b, t, _, h, w = masked_frames.shape
        ops.krig_cs_torus(h, w, self.embed)                  # ValueError before any launch
        if not (masked_frames.is_cuda and masks.is_cuda):
            raise RuntimeError(f"{type(self).__name__}.forward_ensemble runs on the HIP path only (CUDA tensors)")
        if streams is None:
            streams = torch.arange(b * t, dtype=torch.int64)
        else:
            streams = torch.as_tensor(streams)
            if streams.dtype != torch.int64 or tuple(streams.shape) != (b, t):
                raise ValueError(f"forward_ensemble: streams must be an int64 ({b}, {t}) tensor")
        streams = streams.reshape(b * t).contiguous().to(masked_frames.device)
        out = self._krige(masked_frames, masks, ensemble=(members, int(seed), streams))
        return out["pred"], out["ens"]

    @torch.no_grad()
    def forward_uq(self, masked_frames, masks):
        """(prediction, kriging variance), both (B, T, 1, H, W).  The prediction is forward()'s; the variance is 0 on a gauge pixel and
        NaN over a frame without a model (no gauges, a degenerate fitted sample, a failed factorisation)."""
        out = self._krige(masked_frames, masks, variance=True)
        return out["pred"], out["var"]

    @torch.no_grad()
    def cross_validate(self, masked_frames, masks) -> LOOResult:
        """Leave-one-out at every gauge from the one factorisation per system (Dubrule 1983): no refits."""
        return self._krige(masked_frames, masks, predict=False, loo=True)["loo"]

    @torch.no_grad()
    def cross_validate_sites(self, masked_frames, masks) -> LOOResult:
        """cross_validate's result with its site field filled: the systems are per frame, so leaving a site out is leaving a gauge out."""
        return _sites_of_frames(self.cross_validate(masked_frames, masks), masks)

    def _krige(self, masked_frames, masks, predict=True, variance=False, loo=False, ensemble=None):
        b, t, _, h, w = masked_frames.shape
        pix, z, info, counts, shared = self._compact(masked_frames, masks)
        f, dev = b * t, masked_frames.device
        cand = None
        if self.fit:
            lag_width = (min(h, w) / 2.0) / self.n_lags
            bins, fit, cand, params = ops.krig_variogram(pix, z, info, b, t, self.n_lags, lag_width, self.variogram_model)
            self.last_fit = {"bins": bins, "fit": fit, "cand": cand}
        else:
            params = torch.tensor(self.fixed + (0.0,), dtype=torch.float32).repeat(b, 1).to(dev)
        r = t if (shared and self.share_sets) else 1
        nsys = f // r
        np_ = max(ops.KRIG_TILE, _round_up(int(counts.max()), ops.KRIG_TILE))
        inverse = variance or loo or ensemble is not None    # these also hold the factor's inverse
        limit = None
        if ensemble is not None:             # the members' dual coefficients of one chunk of systems stay under the same bound
            members, seed, streams = ensemble
            limit = _FACTOR_BYTES // (r * members * pix.shape[1] * 4)
            amp, clip = ops.krig_cs_spectrum(params, cand, self.variogram_model, h, w, self.embed)
            self.last_ensemble = {"clip": clip, "embed": self.embed}
            ens = torch.empty(f, members, h * w, device=dev, dtype=torch.float32)
            ops.krig_cs_fields(amp, streams, seed, t, members, h, w, self.embed, ens)
        sy = _Systems(pix, z, info, params, cand, self.variogram_model, r, t, np_, inverse, limit)
        work, winv, alpha, mean = sy.work, sy.winv, sy.alpha, sy.mean
        var = torch.empty(f, h * w, device=dev, dtype=torch.float32) if variance else None
        loo_pred, loo_var = (torch.empty_like(z), torch.empty_like(z)) if loo else (None, None)
        for ch in sy.chunks():
            ops.krig_factor(ch, work)
            sol = ops.krig_solve(ch, work, alpha, mean)
            if inverse:
                ops.krig_invert(work, ch.ns, np_, winv)
            if variance:
                ops.krig_variance(ch, winv, sol, h, w, var)
            if loo:
                ops.krig_loo(ch, winv, sol, alpha, loo_pred, loo_var)
            if ensemble is not None:
                ca, cm = ops.krig_cs_weights(ch, winv, sol, ens, members, h, w)
                ops.krig_cs_predict(ch, ca, cm, members, h, w, ens)
        out = {}
        if predict:
            out["pred"] = ops.krig_predict(sy.sys.chunk(0, nsys), alpha, mean, h, w).view(b, t, 1, h, w)
        sy.finish(self, "kriging: %d frame(s) met a non-positive pivot and predict their gauge mean", r)
        if variance:
            out["var"] = var.view(b, t, 1, h, w)
        if loo:
            out["loo"] = LOOResult(pix, z, loo_pred, loo_var, info[:f], sy.status)
        if ensemble is not None:
            out["ens"] = ens.view(b, t, members, h, w)
        return out


class IDWGenerator(_ClassicalBase):
    """Inverse-distance weighting over all gauges of the frame, weights h^-power (model.power, default 2)."""

    def __init__(self, config: Dict[str, Any]):
        super().__init__(config)
        self.power = float(config.get("model", {}).get("power", 2.0))
        if not self.power > 0:
            raise ValueError(f"model.power must be positive (got {self.power})")

    @torch.no_grad()
    def forward(self, masked_frames, masks):
        b, t, _, h, w = masked_frames.shape
        pix, z, info, _, _ = self._compact(masked_frames, masks)
        return ops.idw_all(pix, z, info, h, w, self.power).view(b, t, 1, h, w)

    @torch.no_grad()
    def cross_validate(self, masked_frames, masks) -> LOOResult:
        """Leave-one-out at every gauge: the same weights over the frame's other gauges."""
        pix, z, info, _, _ = self._compact(masked_frames, masks)
        return LOOResult(pix, z, ops.idw_loo(pix, z, info, self.power), None, info[:pix.shape[0]], None)

    @torch.no_grad()
    def cross_validate_sites(self, masked_frames, masks) -> LOOResult:
        """cross_validate's result with its site field filled: a frame's weights see that frame only."""
        return _sites_of_frames(self.cross_validate(masked_frames, masks), masks)


def _advection_config(self, mc):
    """model.advection of the Lagrangian models on `self` (after _variogram_config): fit_velocity and, fitted, vmax, vstep, nhalf,
    adv_tlags and bandwidth; with fit=false, fixed_v."""
    adv = dict(mc.get("advection") or {})
    self.fit_velocity = bool(adv.get("fit", True))
    if self.fit_velocity:
        self.vmax, self.vstep = float(adv.get("vmax", 4.0)), float(adv.get("vstep", 0.5))
        self.adv_tlags, self.bandwidth = int(adv.get("n_tlags", 3)), float(adv.get("bandwidth", 1.5))
        if not (self.vstep > 0 and self.vmax >= 0 and math.isfinite(self.vmax) and math.isfinite(self.vstep)):
            raise ValueError(f"model.advection: vstep > 0 and vmax >= 0 are required (got vmax {self.vmax}, vstep {self.vstep})")
        self.nhalf = int(math.floor(self.vmax / self.vstep + 0.5))
        if self.nhalf > ops.LAGKRIG_MAX_VHALF:
            raise ValueError(f"model.advection: round(vmax / vstep) = {self.nhalf} gives {(2 * self.nhalf + 1) ** 2} candidate velocities, "
                             f"more than the {ops.LAGKRIG_MAX_CANDIDATES} (|i|, |j| <= {ops.LAGKRIG_MAX_VHALF}) the kernel takes")
        if not 0 <= self.adv_tlags <= ops.STKRIG_MAX_TLAGS:
            raise ValueError(f"model.advection.n_tlags must be in [0, {ops.STKRIG_MAX_TLAGS}] (got {self.adv_tlags})")
        if not (self.bandwidth > 0 and math.isfinite(self.bandwidth)):
            raise ValueError(f"model.advection.bandwidth must be positive (got {self.bandwidth})")
        if not 1 <= self.n_lags <= ops.KRIG_MAX_LAGS:          # the bandwidth's unit
            raise ValueError(f"model.variogram.n_lags must be in [1, {ops.KRIG_MAX_LAGS}] (got {self.n_lags})")
    else:
        try:
            self.fixed_v = (float(adv["vy"]), float(adv["vx"]))
        except KeyError as e:
            raise ValueError(f"model.advection with fit=false needs vy and vx (missing {e})") from None
        if not all(math.isfinite(v) for v in self.fixed_v):
            raise ValueError(f"model.advection: vy and vx must be finite (got {self.fixed_v})")


def _simulation_config(mc):
    """(embed, embed_time) of model.ensemble for the space-time conditional simulation, each an integer in 2..4, default 2."""
    ens = mc.get("ensemble")
    if ens is not None and not isinstance(ens, dict):
        raise ValueError(f"model.ensemble must be a mapping such as {{\"embed\": 2, \"embed_time\": 2}} (got {ens!r})")
    out = []
    for key in ("embed", "embed_time"):
        v = (ens or {}).get(key, 2)
        if isinstance(v, bool) or not isinstance(v, int) or v not in ops.KRIG_CS_EMBEDS:
            raise ValueError(f"model.ensemble.{key} must be an integer in {list(ops.KRIG_CS_EMBEDS)} (got {v!r})")
        out.append(v)
    return tuple(out)


class SpaceTimeKrigingGenerator(_ClassicalBase):
    """Ordinary kriging of every pixel of every frame of a sample from ALL gauges of ALL frames of that sample: one system per sample,
    global in space and time, with the distance sqrt(dy^2 + dx^2 + kappa^2 dt^2) (kappa in pixels per frame) inside the covariance.
    model.variogram = {"model", "fit": true, "n_lags": 16, "n_tlags": 3} fits (nugget, psill, range, kappa) per sample on the device;
    {"model", "fit": false, "nugget", "psill", "range", "time_scale"} takes them as given (time_scale is kappa).  model.max_points
    (default 4096) bounds the points of one sample.  model.ensemble = {"embed": 2, "embed_time": 2} (each 2 to 4) sets the sides of
    forward_simulation's embedding torus in frame sides and in sample lengths.

    There is no forward_uq and no cross_validate: leaving out one (site, frame) observation while the same site's neighbouring
    frames stay in would flatter the method; the honest score is leave-one-site-out, cross_validate_sites."""

    DEFAULT_MAX_POINTS = 4096

    def __init__(self, config: Dict[str, Any]):
        super().__init__(config)
        _variogram_config(self, config.get("model", {}), space_time=True)
        self.last_fit = None         # {"bins", "fit", "cand", "q", "c"} device tensors of the last call (fit=true)
        self.last_status = None      # per-sample int32 of the last call: 1 where the factorisation met a non-positive pivot
        self._velf = None            # (B, 2) fp32 of the last call's velocities where _variogram fits them (LagrangianKrigingGenerator)
        self.embed, self.embed_time = _simulation_config(config.get("model", {}))     # forward_simulation's torus, in sample sides
        self.last_ensemble = None    # {"clip": (B,) fp64 clip share of each sample's spectrum, "embed", "embed_time"} of the last one

    def cross_validate(self, masked_frames, masks):
        raise RuntimeError(ST_NO_LOO)

    def _points(self, masked_frames, masks):
        """(pix, z, info of the frames, padded size of the samples' systems) after the host checks."""
        b, t = masked_frames.shape[:2]
        pix, z, info, counts, _ = self._compact(masked_frames, masks)
        per_sample = counts.view(b, t).sum(dim=1)
        if int(per_sample.max()) > self.max_points:
            raise ValueError(f"{type(self).__name__}: a sample has {int(per_sample.max())} space-time points ({t} frames), more than "
                             f"model.max_points = {self.max_points}: use shorter chunks (scripts/infer.py --stride)")
        return pix, z, info, max(ops.KRIG_TILE, _round_up(int(per_sample.max()), ops.KRIG_TILE))

    def _variogram(self, pix, z, info, b, t, h, w):
        """(cand or None, params (B, 4) fp32): the per-sample fit (kept in last_fit) or the fixed parameters."""
        if not self.fit:
            return None, torch.tensor(self.fixed, dtype=torch.float32).repeat(b, 1).to(pix.device)
        lag_width = (min(h, w) / 2.0) / self.n_lags
        bins, fit, cand, params = ops.stkrig_variogram(pix, z, info, b, t, self.n_lags, min(self.n_tlags, t - 1), lag_width,
                                                       self.variogram_model)
        q = torch.div(cand, ops.KRIG_CANDIDATES, rounding_mode="floor")
        self.last_fit = {"bins": bins, "fit": fit, "cand": cand, "q": q, "c": cand - q * ops.KRIG_CANDIDATES}
        return cand, params

    @torch.no_grad()
    def forward(self, masked_frames, masks):
        return self._krige(masked_frames, masks)["pred"]

    @torch.no_grad()
    def forward_simulation(self, masked_frames, masks, members, seed=0, streams=None):
        """(prediction (B, T, 1, H, W), ensemble (B, T, members, H, W)) by conditional simulation in space and time (DESIGN.md section
        26).  The prediction is forward()'s.  A member is one Gaussian field over the whole sample with the space-time covariance of the
        model, conditioned on all the sample's points: it equals the gauge values at the gauge pixels of every frame and its noise is
        correlated from frame to frame, so the spread of a member's accumulation over the sample is the model's.  Member m of a sample
        is a function of (seed, the sample's stream id, m, the variogram, the points) only; streams (B,) int64 defaults to b.  Members
        are raw Gaussian (they can be negative) and NaN over a sample without points, with a degenerate fit or with a failed
        factorisation; a frame without gauges inside a sample that has points is simulated like any other.  1 <= members <= 64."""
        if isinstance(members, bool) or not isinstance(members, int) or not 1 <= members <= ops.KRIG_CS_MAX_MEMBERS:
            raise ValueError(f"forward_simulation: members must be an integer in [1, {ops.KRIG_CS_MAX_MEMBERS}] (got {members!r})")
        if masked_frames.dim() != 5:
            raise RuntimeError(f"{type(self).__name__}.forward_simulation takes (B, T, 1, H, W) frames")
        b, t, _, h, w = masked_frames.shape
        ops.stcs_torus(t, h, w, self.embed, self.embed_time)     # ValueError before any launch
        if not (masked_frames.is_cuda and masks.is_cuda):
            raise RuntimeError(f"{type(self).__name__}.forward_simulation runs on the HIP path only (CUDA tensors)")
        if streams is None:
            streams = torch.arange(b, dtype=torch.int64)
        else:
            streams = torch.as_tensor(streams)
            if streams.dtype != torch.int64 or tuple(streams.shape) != (b,):
                raise ValueError(f"forward_simulation: streams must be an int64 ({b},) tensor")
        streams = streams.contiguous().to(masked_frames.device)
        out = self._krige(masked_frames, masks, simulation=(members, int(seed), streams))
        return out["pred"], out["ens"]

    def _krige(self, masked_frames, masks, simulation=None):
        b, t, _, h, w = masked_frames.shape
        pix, z, info, np_ = self._points(masked_frames, masks)
        stpix, stt, stz, stinfo = ops.stkrig_gather(pix, z, info, b, t, np_)
        cand, params = self._variogram(pix, z, info, b, t, h, w)
        limit = None
        if simulation is not None:           # the members' dual coefficients of one chunk of samples stay under the factors' bound
            members, seed, streams = simulation
            limit = _FACTOR_BYTES // (members * np_ * 4)
            amp, clip = ops.stcs_spectrum(params, cand, self.variogram_model, t, h, w, self.embed, self.embed_time)
            self.last_ensemble = {"clip": clip, "embed": self.embed, "embed_time": self.embed_time}
            ens = torch.empty(b, t, members, h * w, device=masked_frames.device, dtype=torch.float32)
            ops.stcs_fields(amp, streams, seed, members, t, h, w, self.embed, self.embed_time, ens)
            del amp
        # the samples stand in for frames
        sy = _Systems(stpix, stz, stinfo, params, cand, self.variogram_model, 1, 1, np_, simulation is not None, limit)
        for ch in sy.chunks():
            ops.stkrig_factor(ch, stt, sy.work, self._velf)
            sol = ops.krig_solve(ch, sy.work, sy.alpha, sy.mean)
            if simulation is not None:
                ops.krig_invert(sy.work, ch.ns, np_, sy.winv)
                ca, cm = ops.stcs_weights(ch, stt, sy.winv, sol, ens, members, t, h, w)
                ops.stcs_predict(ch, stt, ca, cm, members, t, h, w, ens)
        pred = ops.stkrig_predict(stpix, stt, sy.alpha, sy.mean, stinfo, params, self.variogram_model, t, h, w, self._velf)
        sy.finish(self, "space-time kriging: %d sample(s) met a non-positive pivot and predict their gauge mean")
        out = {"pred": pred.view(b, t, 1, h, w)}
        if simulation is not None:
            out["ens"] = ens.view(b, t, members, h, w)
        return out

    @torch.no_grad()
    def cross_validate_sites(self, masked_frames, masks) -> LOOResult:
        """Leave-one-site-out at every point: a site (a gauge pixel in all the sample's frames) is left out as a whole and its points
        are predicted from the other sites, by the block form of Dubrule's identity on one factorisation and one inverse per sample
        (DESIGN.md section 18).  pred and var are NaN for a sample with one site only, a degenerate fit or a failed factorisation."""
        b, t, _, h, w = masked_frames.shape
        pix, z, info, np_ = self._points(masked_frames, masks)
        if t > ops.KRIG_TILE:
            raise ValueError(f"{type(self).__name__}: leave-one-site-out takes at most {ops.KRIG_TILE} frames per sample (got {t}): use "
                             f"shorter chunks (scripts/crossvalidate.py --stride)")
        sites = ops.stkrig_gather_sites(pix, z, info, b, t, np_)
        cand, params = self._variogram(pix, z, info, b, t, h, w)
        sy = _Systems(sites["stpix"], sites["stz"], sites["stinfo"], params, cand, self.variogram_model, 1, 1, np_, inverse=True)
        pred, var = torch.zeros_like(z), torch.zeros_like(z)
        for ch in sy.chunks():
            ops.stkrig_factor(ch, sites["stt"], sy.work, self._velf)
            sol = ops.krig_solve(ch, sy.work, sy.alpha, sy.mean)
            ops.krig_invert(sy.work, ch.ns, np_, sy.winv)
            gram = ops.stkrig_site_gram(sy.winv, ch.ns, np_)
            ops.stkrig_loso(ch, gram, sol, sy.alpha, sites, t, pred, var)
        sy.finish(self, "space-time kriging: %d sample(s) met a non-positive pivot and have no leave-one-site-out scores")
        return LOOResult(pix, z, pred, var, info[:b * t], sy.status, sites["fsite"])


class LagrangianKrigingGenerator(SpaceTimeKrigingGenerator):
    """Space-time kriging in the frame that moves with the rain: SpaceTimeKrigingGenerator with the distance
    sqrt((dy - v_y dt)^2 + (dx - v_x dt)^2 + kappa^2 dt^2), one advection velocity v = (v_y, v_x) in pixels per frame per sample.
    model.variogram is SpaceTimeKrigingGenerator's.  model.advection = {"fit": true, "vmax": 4.0, "vstep": 0.5, "n_tlags": 3,
    "bandwidth": 1.5} estimates v per sample on the device from the gauges alone, over the candidates (i, j) vstep with |i|, |j| <=
    round(vmax / vstep) (ops.lagkrig_velocity; bandwidth in lag widths of the variogram binning); {"fit": false, "vy", "vx"} takes it
    as given.  last_fit holds "velocity" (B, 2) fp64 and, with a fitted velocity, the "score", "weight" and "support" tables (B, n, n) and "vcand";
    with a fitted variogram SpaceTimeKrigingGenerator's keys too.  As there, no forward_uq and no cross_validate; cross_validate_sites
    fits the velocity and the variogram once from all sites (no refits)."""

    def __init__(self, config: Dict[str, Any]):
        super().__init__(config)
        _advection_config(self, config.get("model", {}))

    def cross_validate(self, masked_frames, masks):
        raise RuntimeError(LAG_NO_LOO)

    def forward_simulation(self, masked_frames, masks, members, seed=0, streams=None):
        raise RuntimeError(LAG_NO_SIMULATION)

    def _variogram(self, pix, z, info, b, t, h, w):
        """(cand or None, params): the velocity first (kept in _velf for the factor and the predictor), then the variogram on the
        advected distance."""
        lag_width = (min(h, w) / 2.0) / self.n_lags
        if self.fit_velocity:
            score, weight, support, vel, velf, vcand = ops.lagkrig_velocity(pix, z, info, b, t, min(self.adv_tlags, t - 1), self.nhalf, self.vstep,
                                                                            self.bandwidth * lag_width)
            last = {"velocity": vel, "score": score, "weight": weight, "support": support, "vcand": vcand}
        else:
            vel = torch.tensor(self.fixed_v, dtype=torch.float64).repeat(b, 1).to(pix.device)
            velf = vel.float()
            last = {"velocity": vel}
        self._velf = velf
        cand = None
        if self.fit:
            bins, fit, cand, params = ops.lagkrig_variogram(pix, z, info, vel, b, t, self.n_lags, min(self.n_tlags, t - 1), lag_width,
                                                            self.variogram_model)
            q = torch.div(cand, ops.KRIG_CANDIDATES, rounding_mode="floor")
            last.update({"bins": bins, "fit": fit, "cand": cand, "q": q, "c": cand - q * ops.KRIG_CANDIDATES})
        else:
            params = torch.tensor(self.fixed, dtype=torch.float32).repeat(b, 1).to(pix.device)
        self.last_fit = last
        return cand, params


class LocalKrigingGenerator(_ClassicalBase):
    """Space-time ordinary kriging in a moving neighbourhood: every pixel of every frame from its k nearest
    points of the sample in the metric dy^2 + dx^2 + kappa^2 dt^2, among the frames within `frames` of its own, from a small system
    of its own (csrc/lkrig.hip).  model.variogram is SpaceTimeKrigingGenerator's; model.neighbourhood = {"k": 32, "frames": 2} with k in
    1 .. 64 and frames >= 0 (clipped to T - 1).  model.max_points bounds the gauges of one frame; the points of a sample are unbounded.

    forward_uq adds the kriging variance of the same systems, and cross_validate_sites is the same kernel with the gauges as targets
    and the target's own site out of the candidates: no inverse and no frame limit.  cross_validate is refused as for stkriging (with
    frames = 0 leave-one-site-out is leave-one-out).  last_status (B,) int32 counts the targets that met a non-positive pivot."""

    def __init__(self, config: Dict[str, Any]):
        super().__init__(config)
        mc = config.get("model", {})
        _variogram_config(self, mc, space_time=True)
        nb = dict(mc.get("neighbourhood") or {})
        k, frames = nb.get("k", 32), nb.get("frames", 2)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.LKRIG_MAX_K:
            raise ValueError(f"model.neighbourhood.k must be an integer in [1, {ops.LKRIG_MAX_K}] (got {k!r})")
        if isinstance(frames, bool) or not isinstance(frames, int) or frames < 0:
            raise ValueError(f"model.neighbourhood.frames must be an integer >= 0 (got {frames!r})")
        self.k, self.frames = k, frames
        self.last_fit = None         # SpaceTimeKrigingGenerator's keys (fit=true)
        self.last_status = None      # (B,) int32 of the last call: targets that met a non-positive pivot
        self.last_neighbours = None  # (B, T, H*W, k) int32 of the last forward(..., neighbours=True), else None
        self._velf = None            # (B, 2) fp32 of the last call's velocities where _variogram fits them (LocalLagrangianKrigingGenerator)

    _variogram = SpaceTimeKrigingGenerator._variogram

    def cross_validate(self, masked_frames, masks):
        raise RuntimeError(LOCAL_NO_LOO)

    def _warn(self, status, what):
        self.last_status = status
        failed = int(status.sum())
        if failed:
            logging.warning("local kriging: %d %s met a non-positive pivot and take the mean of their neighbours", failed, what)

    def _run(self, masked_frames, masks, variance, neighbours):
        b, t, _, h, w = masked_frames.shape
        pix, z, info, _, _ = self._compact(masked_frames, masks)
        cand, params = self._variogram(pix, z, info, b, t, h, w)
        out, var, status, nbr = ops.lkrig_predict(pix, z, info, params, cand, self.variogram_model, self.k, min(self.frames, t - 1), b, t,
                                                  h, w, variance, neighbours, self._velf)
        self.last_neighbours = nbr
        self._warn(status, "pixel(s)")
        return out.view(b, t, 1, h, w), (var.view(b, t, 1, h, w) if variance else None)

    @torch.no_grad()
    def forward(self, masked_frames, masks, neighbours=False):
        """The prediction (B, T, 1, H, W).  neighbours=True (a debug argument) keeps the kernel's selection in last_neighbours."""
        return self._run(masked_frames, masks, False, neighbours)[0]

    @torch.no_grad()
    def forward_uq(self, masked_frames, masks):
        """(prediction, kriging variance), both (B, T, 1, H, W).  The prediction is forward()'s; the variance is 0 on a gauge pixel in its
        own frame and NaN where a rule stood in for the system."""
        return self._run(masked_frames, masks, True, False)

    @torch.no_grad()
    def cross_validate_sites(self, masked_frames, masks) -> LOOResult:
        """Leave-one-site-out at every point: its k nearest points among the other sites, within `frames` frames.  pred and var are NaN
        where no candidate is left and over a degenerate fitted sample."""
        b, t, _, h, w = masked_frames.shape
        pix, z, info, _, _ = self._compact(masked_frames, masks)
        cand, params = self._variogram(pix, z, info, b, t, h, w)
        pred, var, status = ops.lkrig_loso(pix, z, info, params, cand, self.variogram_model, self.k, min(self.frames, t - 1), b, t,
                                           self._velf)
        self._warn(status, "point(s)")
        return _sites_of_frames(LOOResult(pix, z, pred, var, info[:b * t], status), masks)


class LocalLagrangianKrigingGenerator(LocalKrigingGenerator):
    """LocalKrigingGenerator in the frame that moves with the rain: the k nearest points in the metric
    (dy - v_y dt)^2 + (dx - v_x dt)^2 + kappa^2 dt^2, one advection velocity v = (v_y, v_x) in pixels per frame per sample, and
    LagrangianKrigingGenerator's distance inside the target's system.  In that frame a site's copies in the neighbouring frames sit at
    x - v dt, at different places: they are spatial support and no duplicates.  model.variogram and model.neighbourhood are
    LocalKrigingGenerator's, model.advection is LagrangianKrigingGenerator's, and so is the order of the fits: the velocity first, then
    the variogram on the advected distance, each once per sample from all sites (cross_validate_sites does not refit).  last_fit holds
    LagrangianKrigingGenerator's keys.  forward, forward_uq, forward(..., neighbours=True) and cross_validate_sites are the parent's;
    no point limit and no frame limit."""

    def __init__(self, config: Dict[str, Any]):
        super().__init__(config)
        _advection_config(self, config.get("model", {}))
        self._velf = None

    _variogram = LagrangianKrigingGenerator._variogram

    def cross_validate(self, masked_frames, masks):
        raise RuntimeError(LOCAL_LAG_NO_LOO)


ST_NO_LOO = ("space-time kriging ('stkriging') has no leave-one-out cross-validation: leaving out one (site, frame) observation while "
              "the same site's neighbouring frames stay in would flatter the method; the honest score is leave-one-site-out: "
              "cross_validate_sites, evaluation.run_loso, scripts/crossvalidate.py --by-site")

LAG_NO_LOO = ST_NO_LOO.replace("space-time kriging ('stkriging')", "Lagrangian space-time kriging ('lagkriging')")

LAG_NO_SIMULATION = ("Lagrangian space-time kriging ('lagkriging') has no conditional simulation: its covariance is stationary in the frame "
                     "that moves with the rain, which on the pixel grid is a sheared torus that the circulant embedding of 'stkriging' "
                     "(forward_simulation) does not draw")

LOCAL_NO_LOO = ST_NO_LOO.replace("space-time kriging ('stkriging')", "moving-neighbourhood space-time kriging ('localkriging')")

LOCAL_LAG_NO_LOO = ST_NO_LOO.replace("space-time kriging ('stkriging')",
                                     "moving-neighbourhood Lagrangian space-time kriging ('locallagkriging')")

LOCAL = ("localkriging", "locallagkriging")      # one system per target: no point-wise leave-one-out, LOSO of any length, a variance map

SPACE_TIME = ("stkriging", "lagkriging")          # one system per sample: no point-wise leave-one-out, LOSO chunks of at most 32 frames

CLASSICAL = {"kriging": KrigingGenerator, "idw": IDWGenerator, "stkriging": SpaceTimeKrigingGenerator,
             "lagkriging": LagrangianKrigingGenerator, "localkriging": LocalKrigingGenerator,
             "locallagkriging": LocalLagrangianKrigingGenerator}
