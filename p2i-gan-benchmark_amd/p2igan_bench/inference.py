"""Sliding-window inference of infer.py:188-262 on the device: window `stride` (16) every
`stride - overlap` (4) frames, the last windows padded by repeating the final frame, overlap-averaged,
scaled and clipped at 0.  All windows of an event go through the generator as ONE batch (the
reference runs them one by one at B=1) and the overlap-average is accumulated on the device."""
from __future__ import annotations

import torch


@torch.no_grad()
def infer_event(generator, masked: torch.Tensor, masks: torch.Tensor, stride: int = 16, overlap: int = 12,
                output_scale: float = 255.0, max_windows_per_batch: int = 32) -> torch.Tensor:
    """masked, masks: (1, L, 1, H, W) on the generator's device -> (L, 1, H, W) float32.
    HIP tensors (H*W a multiple of 4): windows are gathered and the overlap average / scale / clip is taken by two bandwidth kernels
    (p2i_window_gather, p2i_window_mean) -- no index tensors, no boolean-mask indexing (a device-to-host sync in ATen).  CPU tensors
    (drop-in users, tests): the same arithmetic in torch."""
    L = masked.shape[1]
    step = max(1, stride - overlap)
    nwin = len(range(0, L, step))
    hw = masked.shape[-2] * masked.shape[-1]
    if masked.is_cuda and hw % 4 == 0:
        from . import ops
        m0, k0 = masked[0].contiguous().float(), masks[0].contiguous().float()
        preds = torch.empty((nwin, stride) + tuple(masked.shape[2:]), device=masked.device, dtype=torch.float32)
        for s in range(0, nwin, max_windows_per_batch):
            nw = min(max_windows_per_batch, nwin - s)
            wm, wk = ops.window_gather(m0, k0, L, s, nw, stride, step)
            preds[s:s + nw] = generator(wm, wk)                  # (nw, stride, 1, H, W)
        return ops.window_mean(preds, L, stride, step, output_scale)
    starts = list(range(0, L, step))
    idx = torch.arange(stride, device=masked.device).unsqueeze(0) + torch.tensor(starts, device=masked.device).unsqueeze(1)
    valid = idx < L                                             # (nwin, stride)
    idx = idx.clamp(max=L - 1)                                  # repeat the last frame (infer.py:219-227)
    acc = torch.zeros(L, *masked.shape[2:], device=masked.device)
    cnt = torch.zeros(L, device=masked.device)
    for s in range(0, len(starts), max_windows_per_batch):
        ii = idx[s:s + max_windows_per_batch]
        out = generator(masked[0][ii].contiguous(), masks[0][ii].contiguous())      # (nw, stride, 1, H, W)
        vv = valid[s:s + max_windows_per_batch]
        acc.index_add_(0, ii[vv], out[vv])
        cnt.index_add_(0, ii[vv], torch.ones_like(ii[vv], dtype=torch.float32))
    comp = acc / cnt.clamp(min=1e-5).view(L, 1, 1, 1) * float(output_scale)
    return comp.clamp(min=0.0)


@torch.no_grad()
def infer_event_chunks(generator, masked: torch.Tensor, masks: torch.Tensor, stride: int = 16, output_scale: float = 255.0) -> torch.Tensor:
    """The parameter-free baselines' event pass: masked, masks (1, L, 1, H, W) -> (L, 1, H, W) float32.  The event runs in consecutive
    chunks of `stride` frames without overlap (the last one shorter); each chunk is one sample to the generator, so a fitted variogram
    pools the chunk's frames.  Scaled and clipped at 0 as infer_event does."""
    L = masked.shape[1]
    parts = [generator(masked[:, s:s + stride].contiguous(), masks[:, s:s + stride].contiguous())[0] for s in range(0, L, stride)]
    return (torch.cat(parts, dim=0) * float(output_scale)).clamp(min=0.0)


@torch.no_grad()
def infer_event_variance(generator, masked: torch.Tensor, masks: torch.Tensor, stride: int = 16, output_scale: float = 255.0) -> torch.Tensor:
    """The kriging variance of infer_event_chunks' predictions, chunk by chunk: (L, 1, H, W) float32 = sigma^2 x output_scale^2 (NaN
    over a frame without a model)."""
    L = masked.shape[1]
    parts = [generator.forward_uq(masked[:, s:s + stride].contiguous(), masks[:, s:s + stride].contiguous())[1][0] for s in range(0, L, stride)]
    return torch.cat(parts, dim=0) * float(output_scale) ** 2


@torch.no_grad()
def infer_event_ensemble(generator, masked: torch.Tensor, masks: torch.Tensor, members: int, seed: int = 0, event_index: int = 0,
                         stride: int = 16, output_scale: float = 255.0) -> torch.Tensor:
    """The conditional-simulation members of infer_event_chunks' predictions, chunk by chunk (the same chunks, so the same fits):
    (L, members, H, W) float32 = member x output_scale, unclipped (NaN where there is no model).  generator.last_ensemble["clip"] holds
    the clip shares of all the event's chunks afterwards.
    'kriging' (forward_ensemble): the noise is per frame; the stream id of frame l of the event is (event_index << 32) | l, so the chunk
    length changes the fit but not the noise.
    'stkriging' (forward_simulation): the noise is one space-time field per chunk; the stream id of a chunk is (event_index << 32) | its
    first frame.  Members are coherent within a chunk and independent across chunk borders."""
    L = masked.shape[1]
    per_frame = hasattr(generator, "forward_ensemble")
    if not per_frame and not hasattr(generator, "forward_simulation"):
        raise RuntimeError(f"{type(generator).__name__} has no conditional simulation: 'kriging' (forward_ensemble) and 'stkriging' "
                           f"(forward_simulation) have")
    parts, clips = [], []
    for s in range(0, L, stride):
        n = min(stride, L - s)
        x, m = masked[:, s:s + stride].contiguous(), masks[:, s:s + stride].contiguous()
        if per_frame:
            streams = (int(event_index) << 32) + torch.arange(s, s + n, dtype=torch.int64).view(1, n)
            parts.append(generator.forward_ensemble(x, m, members, seed=seed, streams=streams)[1][0])
        else:
            streams = torch.tensor([(int(event_index) << 32) + s], dtype=torch.int64)
            parts.append(generator.forward_simulation(x, m, members, seed=seed, streams=streams)[1][0])
        clips.append(generator.last_ensemble["clip"])
    generator.last_ensemble = dict(generator.last_ensemble, clip=torch.cat(clips))
    return torch.cat(parts, dim=0) * float(output_scale)
