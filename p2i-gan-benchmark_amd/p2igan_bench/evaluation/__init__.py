"""The benchmark's evaluation of inference outputs (reference experiments/exp1.py, exp2.py, exp3.py with experiments/io.py), with the
arithmetic on the device (csrc/eval_exp1.hip, eval_exp2.hip, eval_exp3.hip over eval_common.h).  There is no CPU path: without a GPU
every evaluator raises RuntimeError.  The package imports without a GPU, matplotlib or PIL.

exp1 (``exp1.py``): ``run_exp1`` takes the reference's arguments and returns its table: per method MAE, RMSE,
PSS, SSIM, DTSSIM_L1, DTSSIM_L2, NSE and ``CAT_<thr:g>`` = {POD, FAR, CSI, HSS}.  Inputs may be numpy arrays, torch tensors (CPU or
device) or dicts of per-event arrays (``[T, H, W]``, ``[T, 1, H, W]``, ``[T, H, W, 1]`` or ``[1, T, H, W]``, on the 0-255 scale).
``Exp1Evaluator`` is the streaming form it is built on: one ``update`` per aligned piece, one host sync in ``compute``.

exp2 (``exp2.py``, ``exp2_chrome.py``, section 12): ``run_exp2`` takes the reference's arguments and writes its
comparison GIFs and ``event_ranges.txt`` plus ``exp2_data.npz``; the frames are canvases of palette indices (``compute_exp2``,
``exp2_canvases``).  ``run_exp2_paper_zarr`` writes the paper's frame grid.

exp3 (``exp3.py``, section 11): ``run_exp3`` takes the reference's arguments, returns ``{"NSE_<name>": float}`` and writes the
reference's four figures plus ``exp3_data.npz`` (the numbers behind them).  ``Exp3Evaluator`` is its streaming form (one
``add_event`` per truth event, two host syncs in ``compute``).

scale (``scale.py``, section 15; no counterpart in the reference): ``run_scale`` returns per method the fractions skill score over
thresholds x neighbourhood sizes, the smallest useful scale, and the radially averaged power spectra with their log-spectral distance
and high-wavenumber ratio against the truth's.  ``ScaleEvaluator`` is its streaming form (one host sync in ``compute``).

loo (``loo.py``, section 16; no counterpart in the reference): ``run_loo`` cross-validates a classical baseline leave-one-out at the
gauges of every test event and writes ``loo.json``, ``loo.txt`` and ``loo_data.npz``; it needs no gridded truth.  ``run_loso`` (section 18) is the same with whole sites left out, the score of the
space-time baseline; it writes ``loso.json``, ``loso.txt`` and ``loso_data.npz``.

prob (``prob.py``, section 22; no counterpart in the reference): ``run_prob`` scores a prediction with its variance as a Gaussian,
left-censored at 0, against the truth: CRPS, PIT histogram, interval coverage and sharpness, standardised error, spread against skill
and Brier / reliability / ROC of the rain-rate exceedances, per method "dressed" (its own MSE as the variance) and with its variance
map.  ``run_prob_points`` does the same for cross-validation columns; ``ProbEvaluator`` is the streaming form.

objects (``objects.py``, section 23; no counterpart in the reference): ``run_objects`` labels the connected rain objects of every
frame at the absolute thresholds and at one relative level and returns per method and level SAL (structure, amplitude, location)
against the truth and the object population of both sides.  ``ObjectEvaluator`` is the streaming form (one host read per launch).

ensemble (``ensemble.py``, section 25; no counterpart in the reference): ``run_ensemble`` scores M-member ensembles (a deterministic
field is a one-member one) against the truth: CRPS and fair CRPS, rank histograms, spread against skill and exceedance reliability of
pixels and of box means, and per frame the energy score and the variogram score.  ``EnsembleEvaluator`` is the streaming form.

``_common.py`` holds what the units share: the input and event-dict rules and ``Streaming``, the base of the exp1, scale, prob and
objects evaluators (section 10a)."""
from ._common import crop_mask, crop_origin, ensure_thw_shape, selection, transform_mmhr, truth_lut  # noqa: F401
from .exp1 import DEFAULT_THRESHOLDS, PSS_BINS, PSS_MIN_VALUE, Exp1Evaluator, pss_bin, pss_edges, run_exp1  # noqa: F401
from .exp2 import (EXP2_MAX_EVENTS, EXP2_MAX_FRAMES, Exp2Event, Exp2Result, compute_exp2, default_zoom, exp2_canvases,  # noqa: F401
                   iter_exp2, paper_panels, run_exp2, run_exp2_paper_zarr)
from .exp2_chrome import (EXP2_GREYS, EXP2_IDX_BAD, EXP2_IDX_BG, EXP2_IDX_EDGE, EXP2_IDX_GREY, PAPER_BOUNDS, PAPER_COLORS,  # noqa: F401
                          PAPER_SUB, exp2_chrome, exp2_layout, exp2_palette, paper_cmap, write_exp2_gif)
from .exp3 import (EXP3_MAX_POINTS, EXP3_MIN_VALUE, EXP3_SEED, LOGFREQ_EDGES, SCATTER_COLORS, Exp3Evaluator, Exp3Result,  # noqa: F401
                   compute_exp3, linregress, run_exp3, write_exp3_figures)
from .loo import loo_lines, loso_lines, run_loo, run_loso  # noqa: F401
from .scale import (DEFAULT_SCALES, ScaleEvaluator, check_overflow, fss_value, ring_counts, ring_index, ring_list, run_scale,  # noqa: F401
                    scale_lines, spectrum_scores, twiddle, useful_scale, write_scale_figure, write_scale_outputs)
from .prob import (DEFAULT_LEVELS, DEFAULT_PIT_BINS, DEFAULT_REL_BINS, DEFAULT_SIGMA_EDGES, ProbEvaluator, half_width,  # noqa: F401
                   pixel_threshold, prob_arrays, prob_lines, prob_scores, roc_area, run_prob, run_prob_points, unpack_record,
                   write_prob_figure, write_prob_outputs)
from .ensemble import (DEFAULT_BOX_SIZES, DEFAULT_OFFSETS, EnsembleEvaluator, energy_scores, ens_arrays, ens_lines, ens_scores,  # noqa: F401
                       run_ensemble, variogram_scores, write_ens_figure, write_ens_outputs)
from .objects import (DEFAULT_SAL_FACTOR, DEFAULT_SAL_FLOOR, ObjectEvaluator, level_keys, objects_lines, run_objects, sal_frames,  # noqa: F401
                      sal_summary, write_objects_figure, write_objects_outputs)
