"""Frames of heat-map videos on the device (concept_attention/video/video_utils.py): one coloured frame per timestep, with
the range taken over all frames, per concept (``make_individual_videos``) or over everything
(``make_concept_attention_video``).  The frames come out of ops.heatmap_render as bytes; writing a file is the caller's
business (examples/example_sweep_frames.py writes a GIF through PIL)."""
from __future__ import annotations

import torch

from . import ops


@torch.no_grad()
def concept_attention_frames(maps: torch.Tensor, cmap="inferno", per_concept: bool = True, size=None,
                             interpolation: str = "nearest") -> torch.Tensor:
    """``maps``: a device fp32 view (concepts, frames, h, w) whose planes are contiguous and, per concept, equally spaced --
    for a sweep table [levels, layers, C, side, side] that is ``table[:, layer].permute(1, 0, 2, 3)``, which is not
    copied.  Returns uint8 (concepts, frames, H, W, 3) on the device.
    ``per_concept=True``: every concept's frames share that concept's own min / max (make_individual_videos), one group
    per concept; ``per_concept=False``: one min / max over everything (make_concept_attention_video), found by one
    ``torch.aminmax`` on the device and handed to the kernel as its range, with no synchronisation.
    ``size``: None (h, w), an int or (H, W); ``interpolation``: "nearest" or "bilinear"."""
    if interpolation not in ("nearest", "bilinear"):
        raise ValueError(f"interpolation = {interpolation!r}: \"nearest\" or \"bilinear\"")
    if not isinstance(maps, torch.Tensor) or maps.dim() != 4 or maps.shape[0] < 1 or maps.shape[1] < 1:
        raise ValueError("concept_attention_frames: maps must be a tensor (concepts, frames, h, w)")
    C, T, h, w = (int(v) for v in maps.shape)
    H, W = (h, w) if size is None else ((int(size), int(size)) if isinstance(size, int) else (int(v) for v in size))
    ranges = None
    if not per_concept:
        lo, hi = torch.aminmax(maps)
        ranges = torch.stack([lo, hi]).to(torch.float32)
    out = torch.empty(C, T, H, W, 3, dtype=torch.uint8, device=maps.device)
    ops.heatmap_render([maps[c] for c in range(C)], ops.colormap_lut(cmap, maps.device), size=(H, W),
                       bilinear=interpolation == "bilinear", ranges=ranges, out=list(out))
    return out
