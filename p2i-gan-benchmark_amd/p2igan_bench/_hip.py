"""ctypes binding of libp2i_hip.so (C ABI declared in include/p2i_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C p2i-gan-benchmark_amd/csrc``.
There is NO fallback: if the shared object is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libp2i_hip.so")
_lib = None

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH = 0, 1, 2, 3


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("B", "Cin", "Cout", "Ti", "Hi", "Wi", "To", "Ho", "Wo", "kt", "kh", "kw",
                 "st", "sh", "sw", "pt", "ph", "pw")]


class ConvSplit(C.Structure):
    """p2i_conv_split: what the bf16-split pipe of one forward / data-gradient call may use (pre-split weights, or a scratch to split
    them into; pre-split source planes)"""
    _fields_ = [("w_split", C.c_void_p), ("w_scratch", C.c_void_p), ("src_planes", C.c_void_p), ("w_split_taps", C.c_int)]


class EvalInput(C.Structure):
    """p2i_eval_input: one evaluation input [T][h][w] of dtype code ``dtype`` and the origin (top, left) of the crop read from it"""
    _fields_ = [("data", C.c_void_p)] + [(n, C.c_int) for n in ("dtype", "h", "w", "top", "left")]


class KrigSystems(C.Structure):
    """p2i_krig_systems: one chunk of nsys dense kriging systems, stated once for the nine stages that take it"""
    _fields_ = [(n, C.c_void_p) for n in "pix z counts params cand status".split()] + [(n, C.c_int) for n in "model f0 R T nsys np cap".split()]


_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_L = C.c_int64
_F64 = C.c_double
_D = C.POINTER(ConvDesc)
_S = C.POINTER(ConvSplit)
_E = C.POINTER(EvalInput)
_K = C.POINTER(KrigSystems)

# name -> argtypes (every entry point returns int); must list EVERY symbol of include/p2i_hip.h
SIGNATURES = {
    "p2i_conv_fwd": [_D, _P, _P, _S, _P, _P, _P, _I, _P],
    "p2i_conv_dgrad": [_D, _P, _P, _I, _P, _S, _P, _P, _I, _P, _P],
    "p2i_conv_wgrad": [_D, _P, _P, _P, _I, _P, _P, _P, _L, _P],
    "p2i_x6_split": [_P, _P, _I, _I, _I, _P],
    "p2i_x6_split_batched": [_P, _P, _P, _P, _P, _I, _P],
    "p2i_x6c_would_take": [_D, _I, _I],
    "p2i_conv_last_plan": [C.POINTER(C.c_int)],
    "p2i_wgrad_last_plan": [C.POINTER(C.c_int)],
    "p2i_fast_div_magic": [_I, C.POINTER(C.c_uint32)],
    "p2i_doconv_fold_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "p2i_doconv_fold_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "p2i_doconv_fold_fwd_batched": [_P, _P, _P, _I, _I, _I, _P, _P, _P],
    "p2i_doconv_fold_bwd_batched": [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
    "p2i_weight_pack": [_P, _I, _I, _I, _P, _P, _P, _P],
    "p2i_weight_pack_batched": [_P, _P, _P, _P, _P, _P, _P, _I, _P],
    "p2i_weight_unpack_grad_batched": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "p2i_weight_unpack_grad": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "p2i_spectral_norm": [_P, _I, _I, _P, _P, _I, _P, _P, _P],
    "p2i_spectral_norm_batched": [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P],
    "p2i_attn_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "p2i_attn_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "p2i_idw_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "p2i_idw_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "p2i_pooldup_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "p2i_pooldup_bwd": [_P, _P, _P, _I, _I, _I, _I, _P],
    "p2i_upmod_fwd": [_P, _P, _P, _I, _P, _I, _I, _I, _I, _P],
    "p2i_window_gather": [_P, _P, _P, _P, _I, _L, _I, _I, _I, _I, _P],
    "p2i_window_mean": [_P, _P, _I, _L, _I, _I, _I, _F, _P],
    "p2i_upmod_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "p2i_dtail_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "p2i_dtail_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "p2i_recloss": [_P, _P, _F, _P, _P, _P, _I, _I, _I, _P],
    "p2i_gan_loss": [_P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _P],
    "p2i_loss_transform_fwd": [_P, _P, _L, _P],
    "p2i_loss_transform_bwd": [_P, _P, _P, _L, _P],
    "p2i_fdiff_fwd": [_P, _P, _I, _I, _L, _P],
    "p2i_fdiff_bwd": [_P, _P, _I, _I, _L, _P],
    "p2i_wl1_fwd": [_P, _P, _P, _L, _P],
    "p2i_wl1_bwd": [_P, _P, _P, _P, _L, _P],
    "p2i_softmax_t_fwd": [_P, _P, _I, _I, _F, _P],
    "p2i_softmax_t_bwd": [_P, _P, _P, _I, _I, _F, _P],
    "p2i_kl_fwd": [_P, _P, _P, _L, _I, _P],
    "p2i_kl_bwd": [_P, _P, _P, _P, _L, _I, _P],
    "p2i_spool_fwd": [_P, _P, _P, _I, _I, _I, _P],
    "p2i_spool_bwd": [_P, _P, _P, _P, _I, _I, _I, _P],
    "p2i_tdm_fwd": [_P, _P, _P, _F, _F, _P, _P, _P, _I, _I, _I, _I, _P],
    "p2i_shock_map_fwd": [_P, _P, _I, _I, _I, _F, _F, _P],
    "p2i_shock_map_bwd": [_P, _P, _P, _P, _I, _I, _I, _F, _F, _P],
    "p2i_shock_loss_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _P],
    "p2i_shock_loss_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _P],
    "p2i_adam": [_P, _P, _P, _P, _L, _F, _F, _F, _F, _I, _P],
    "p2i_adam_dev": [_P, _P, _P, _P, _L, _F, _F, _F, _F, _P, _P, _P],
    "p2i_metrics_pointwise": [_P, _P, _L, C.POINTER(C.c_float), _I, _I, _P, _P, _P, _P],
    "p2i_metrics_fss": [_P, _I, _I, _I, _I, C.POINTER(C.c_int), _I, _P, _P, _P],
    "p2i_assemble_batch": [_P, _P, _L, _P, _P, _P, _I, _I, _I, _I, _P],
    "p2i_axpy": [_P, _P, _F, _L, _P],
    "p2i_add2": [_P, _P, _P, _L, _P],
    "p2i_zero": [_P, _L, _P],
    "p2i_act_bwd": [_P, _P, _I, _P, _L, _P],
    "p2i_bias_grad": [_P, _P, _I, _P, _I, _I, _L, _P],
    "p2i_act_bwd_bias": [_P, _P, _I, _P, _P, _I, _I, _L, _P],
    "p2i_det_workspace": [_P, _L, _P, _I],
    "p2i_x6_split_planes": [_P, _P, _I, _I, _L, _P],
    "p2i_event_record": [_I, _P],
    "p2i_event_wait": [_I, _P],
    "p2i_tape_begin": [_P],
    "p2i_tape_end": [C.POINTER(C.c_void_p)],
    "p2i_tape_info": [_P, C.POINTER(C.c_int)],
    "p2i_tape_replay": [_P, _P],
    "p2i_tape_free": [_P],
    "p2i_stdk_basis": [_P, _P, _I, _I, _I, _P, _P],
    "p2i_stdk_select": [_P, _P, _I, _I, _I, _P, _P, _P],
    "p2i_stdk_layer1_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "p2i_stdk_mlp_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P],
    "p2i_stdk_bwd_workspace": [_I, _I, C.POINTER(C.c_int64)],
    "p2i_stdk_mlp_bwd": [_P] * 8 + [_I, _I] + [_P] * 13,
    "p2i_stdk_layer1_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P],
    "p2i_exp1_transform": [_P, _I, _L, _I, _P, _P],
    "p2i_exp1_workspace": [_I, _I, _I, C.POINTER(C.c_int64)],
    "p2i_exp1_accumulate": [_E, _E, _I, _I, _I, _P, _I, _P, C.POINTER(C.c_double), _I, _I, _P, _P, _P, _P, _P, _P],
    "p2i_exp1_merge": [_P, _L, _P, _P],
    "p2i_exp1_hist": [_P, _P, _I, _I, _P, _P, _P, _P, _P],
    "p2i_exp1_ssim": [_P, _P, _I, _I, _P, _P, _P, _P],
    "p2i_exp1_finalize": [_P, C.POINTER(C.c_double), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "p2i_exp3_accumulate": [_E, _E, _I, _I, _P, _P, _I, _P, _P, _P, _P],
    "p2i_exp3_truth_hist": [_E, _I, _I, _P, _I, _P, _P],
    "p2i_exp3_scan": [_P, _L, _P, _P],
    "p2i_exp3_gather": [_E, _E, _I, _I, _P, _I, _P, _L, _P, _I, _P, _P, _P],
    "p2i_exp3_nse": [_P, _P, _I, _P, _I, _P, _P],
    "p2i_exp2_index": [_E, _I, _I, _I, _P, _P, _I, _P, _P],
    "p2i_exp2_compose": [_P, _I, _I, _I, _I, C.c_uint, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P],
    "p2i_krig_compact": [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "p2i_krig_bins": [_P, _P, _P, _I, _I, _I, _I, _F64, _P, _P],
    "p2i_krig_fit": [_P, _I, _I, _I, _F64, _I, _P, _P, _P, _P, _P],
    "p2i_krig_factor": [_K, _P, _P],
    "p2i_krig_solve": [_K, _P, _P, _P, _P, _P],
    "p2i_krig_predict": [_K, _P, _P, _I, _I, _P, _P],
    "p2i_idw_all": [_P, _P, _P, _I, _I, _I, _I, _F, _P, _P],
    "p2i_krig_invert": [_P, _I, _I, _P, _P],
    "p2i_krig_variance": [_K, _P, _P, _I, _I, _P, _P],
    "p2i_krig_loo": [_K, _P, _P, _P, _P, _P, _P, _P],
    "p2i_krig_cs_spectrum": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "p2i_krig_cs_noise": [C.c_uint64, _L, _I, _I, _I, _I, _P, _P],
    "p2i_krig_cs_fields": [_P, _P, _P, _P, C.c_uint64, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "p2i_krig_cs_weights": [_K, _P, _P, _P, _I, _I, _I, _P, _P, _P],
    "p2i_krig_cs_predict": [_K, _P, _P, _I, _I, _I, _P, _P],
    "p2i_stkrig_gather": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "p2i_stkrig_bins": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F64, _P, _P],
    "p2i_stkrig_fit": [_P, _I, _I, _I, _I, _F64, _I, _P, _P, _P, _P, _P],
    "p2i_stkrig_factor": [_K, _P, _P, _P, _P],
    "p2i_stkrig_predict": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P],
    "p2i_stkrig_gather_sites": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "p2i_stkrig_site_gram": [_P, _I, _I, _P, _P],
    "p2i_stkrig_loso": [_K, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P],
    "p2i_lagkrig_velocity": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F64, _F64, _P, _P],
    "p2i_lagkrig_pick": [_P, _I, _I, _I, _F64, _P, _P, _P, _P, _P, _P, _P],
    "p2i_lkrig_predict": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "p2i_lkrig_loso": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "p2i_idw_loo": [_P, _P, _P, _I, _I, _F, _P, _P],
    "p2i_loo_scores": [_P, _P, _P, _P, _I, _I, _P, _P, _P],
    "p2i_scale_fss": [_E, _E, _I, _I, _P, C.POINTER(C.c_double), _I, C.POINTER(C.c_int), _I, _I, _P, _P, _P],
    "p2i_scale_fss_merge": [_P, _L, _I, _P, _P],
    "p2i_scale_dft_rows": [_E, _I, _I, _I, _P, _I, _P, _P, _P, _P],
    "p2i_scale_dft_cols": [_P, _I, _I, _P, _P, _P],
    "p2i_scale_rings": [_P, _I, _I, _P, _P, _P, _P, _I, _P, _P],
    "p2i_scale_spectrum_merge": [_P, _P, _L, _I, _P, _P],
    "p2i_prob_record": [_I, _I, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "p2i_prob_accumulate": [_E, _E, _F64, _E, _L, _I, _I, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_double), _I,
                            C.POINTER(C.c_double), _I, C.POINTER(C.c_double), _I, _I, _I, _I, _I, _P, _L, _P],
    "p2i_prob_merge": [_P, _L, _I, _I, _P, _P],
    "p2i_objects_quantize": [_E, _I, _I, _I, _P, C.POINTER(C.c_double), _I, _F64, _F64, _I, _P, _P, _P, _P],
    "p2i_objects_label": [_P, _I, _I, _I, _I, _I, _P, _P],
    "p2i_objects_count": [_P, _I, _P, _I, _I, _I, _P, _P, _P],
    "p2i_objects_scan": [_P, _L, _P, _P],
    "p2i_objects_fill": [_P, _I, _P, _I, _I, _I, _P, _L, _P, _P],
}

# the ensemble-verification unit's entry points (include/p2i_ens.h, versioned by p2i_ens_abi_version): a table of their own, because
# the table above mirrors p2i_hip.h name for name; must list EVERY symbol of include/p2i_ens.h
ENS_SIGNATURES = {
    "p2i_ens_abi_version": [],
    "p2i_ens_record": [_I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "p2i_ens_points": [_E, _I, _L, _E, _L, _I, _I, _I, _P, C.POINTER(C.c_double), _I, C.POINTER(C.c_double), _I, _P, _L, _P],
    "p2i_ens_energy": [_E, _I, _L, _E, _L, _I, _I, _P, _P, _P],
    "p2i_ens_variogram": [_E, _I, _L, _E, _L, _I, _I, _P, C.POINTER(C.c_int), _I, _P, _P],
}

# the space-time conditional simulation's entry points (include/p2i_stcs.h, versioned by p2i_stcs_abi_version), a table of their own
# for the same reason; must list EVERY symbol of include/p2i_stcs.h
STCS_SIGNATURES = {
    "p2i_stcs_abi_version": [],
    "p2i_stcs_spectrum": [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "p2i_stcs_noise": [C.c_uint64, _L, _I, _I, _I, _I, _I, _P, _P],
    "p2i_stcs_fields": [_P, _P, _P, _P, _P, C.c_uint64, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "p2i_stcs_weights": [_K, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "p2i_stcs_predict": [_K, _P, _P, _P, _I, _I, _I, _I, _P, _P],
}


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load the HIP library (once).  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"libp2i_hip.so not found at {_LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C p2i-gan-benchmark_amd/csrc`.  There is no CPU fallback for the product path.")
    # P2I_HIP_LIB: another build of the SAME library (kernel A/B experiments, tools/); never a different backend
    lib = C.CDLL(os.environ.get("P2I_HIP_LIB") or _LIB_PATH)
    for table in (SIGNATURES, ENS_SIGNATURES, STCS_SIGNATURES):
        for name, args in table.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = C.c_int
    lib.p2i_abi_version.restype = C.c_int
    lib.p2i_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().p2i_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")
