"""Model registry — the construction API of the reference (models/__init__.py:13-46).

The P2I-GAN family and the STDK (spatio-temporal DeepKriging) baseline are built on the HIP path, and so are two parameter-free
classical baselines the reference does not have: ordinary kriging and all-gauge IDW (models/classical.py),
space-time ordinary kriging over all frames of a sample (`stkriging`) and its Lagrangian form with a fitted
advection velocity (`lagkriging`), and space-time kriging in a moving neighbourhood (`localkriging`, section 20)
and its Lagrangian form (`locallagkriging`, section 21).
The purely spatial DK baseline and the `simple` fallback stub are out of this build's scope and raise a clear
error."""
from typing import Any, Dict

import torch.nn as nn

from .classical import (CLASSICAL, IDWGenerator, KrigingGenerator, LagrangianKrigingGenerator, LocalKrigingGenerator,
                        LocalLagrangianKrigingGenerator, SpaceTimeKrigingGenerator)
from .p2igan import P2IDiscriminator, P2IGenerator
from .stdk import STDKGenerator


def _model_name(cfg: Dict[str, Any]) -> str:
    return cfg.get("model", {}).get("name", "simple").lower()


def build_generator(cfg: Dict[str, Any]) -> nn.Module:
    name = _model_name(cfg)
    if name == "p2igan":
        return P2IGenerator(cfg)
    if name == "stdk":
        data_cfg = cfg.get("data_loader") or cfg.get("data", {}).get("train", {})
        return STDKGenerator(cfg, length=data_cfg.get("sample_length", 16))
    if name in CLASSICAL:
        return CLASSICAL[name](cfg)
    raise NotImplementedError(f"model '{name}': only 'p2igan', 'stdk', 'kriging', 'idw', 'stkriging', 'lagkriging', 'localkriging' and 'locallagkriging' are implemented on the MI355X path")


def build_discriminator(cfg: Dict[str, Any]) -> nn.Module:
    name = _model_name(cfg)
    if name == "p2igan":
        in_channels = cfg.get("model", {}).get("in_channels", 1)
        data_cfg = cfg.get("data_loader") or cfg.get("data", {}).get("train", {})
        sample_length = data_cfg.get("sample_length", 16)
        return P2IDiscriminator(in_channels=in_channels * sample_length)
    raise NotImplementedError(f"model '{name}': only 'p2igan' is implemented on the MI355X path")


__all__ = ["build_generator", "build_discriminator", "P2IGenerator", "P2IDiscriminator", "STDKGenerator",
           "KrigingGenerator", "IDWGenerator", "SpaceTimeKrigingGenerator", "LagrangianKrigingGenerator", "LocalKrigingGenerator",
           "LocalLagrangianKrigingGenerator"]
