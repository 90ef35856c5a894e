"""The host side of exp2's pictures: the reference's colour table, the GIF's palette and index space, the canvas layout, the static
chrome (titles, colour bar; text rasterised with PIL, imported only when text is drawn) and the GIF writer."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .. import ops

PAPER_BOUNDS = (0, 0.5, 1, 2, 4, 8, 16, 200)
PAPER_COLORS = ("#000000", "#46327e", "#277f8e", "#4ac16d", "#a0da39", "#fde725", "#ffffff")
PAPER_SUB = 20
# the GIF's index space: 0 .. 140 the colour table, then "bad" (NaN: transparent in matplotlib, the white figure shows), the gauge
# panel's black background, the discs' edge colour #dddddd, and 16 greys from white to black for the host-drawn text
EXP2_IDX_BAD = ops.EXP2_BAD
EXP2_IDX_BG = 142
EXP2_IDX_EDGE = 143
EXP2_IDX_GREY = 144
EXP2_GREYS = 16
_EXP2_MARGIN, _EXP2_GAP, _EXP2_STRIP, _EXP2_LABEL = 8, 8, 22, 18
_EXP2_BAR_GAP, _EXP2_BAR_H, _EXP2_TICK_H, _EXP2_CBL_H, _EXP2_BOTTOM = 10, 12, 14, 16, 6


def paper_cmap() -> Tuple[np.ndarray, np.ndarray]:
    """(bounds [142] f64, colors [141, 4] f64 RGBA) of the reference's _build_paper_cmap, with its arithmetic: every segment of
    PAPER_BOUNDS is ``np.linspace(lo, hi, 21, endpoint=False)`` (so the coarse bounds 0.5 ... 16 are not among the fine ones), the
    first kept whole and the others without their first point, then 200; 6 x 20 colours interpolated between the hex colours
    with t = k / 19, the last hex colour, and white up to 141."""
    fine = []
    for i in range(len(PAPER_BOUNDS) - 1):
        seg = np.linspace(PAPER_BOUNDS[i], PAPER_BOUNDS[i + 1], PAPER_SUB + 1, endpoint=False)
        fine.extend(seg.tolist() if i == 0 else seg[1:].tolist())
    fine.append(PAPER_BOUNDS[-1])
    bounds = np.asarray(fine, float)
    base = [tuple(int(h[i:i + 2], 16) / 255.0 for i in (1, 3, 5)) for h in PAPER_COLORS]
    colors = []
    for c0, c1 in zip(base[:-1], base[1:]):
        for k in range(PAPER_SUB):
            t = k / float(PAPER_SUB - 1)
            colors.append(tuple((1 - t) * a + t * b for a, b in zip(c0, c1)))
    colors.append(base[-1])
    while len(colors) < len(bounds) - 1:
        colors.append(base[-1])
    rgba = np.ones((len(colors), 4), dtype=np.float64)
    rgba[:, :3] = np.asarray(colors, dtype=np.float64)
    return bounds, rgba


def exp2_palette() -> np.ndarray:
    """The GIF palette [256, 3] uint8: the colour table as matplotlib turns it into bytes (``(rgba * 255).astype(uint8)``), then the
    entries listed at EXP2_IDX_*; the rest is black and unused."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[:EXP2_IDX_BAD] = (paper_cmap()[1][:, :3] * 255).astype(np.uint8)
    pal[EXP2_IDX_BAD] = 255
    pal[EXP2_IDX_BG] = 0
    pal[EXP2_IDX_EDGE] = 0xdd
    for i in range(EXP2_GREYS):
        pal[EXP2_IDX_GREY + i] = 255 - 17 * i
    return pal


def exp2_layout(npanels: int, size: int, zoom: int) -> Dict[str, int]:
    """Where things lie on the canvas: the title strip, the panel labels, the panel row (panel p at column ox + p * step), the
    colour bar.  pitch is the row pitch of the device canvas (the width rounded up to 16)."""
    side = size * zoom
    width = 2 * _EXP2_MARGIN + npanels * side + (npanels - 1) * _EXP2_GAP
    oy = _EXP2_STRIP + _EXP2_LABEL
    bar_y = oy + side + _EXP2_BAR_GAP
    height = bar_y + _EXP2_BAR_H + _EXP2_TICK_H + _EXP2_CBL_H + _EXP2_BOTTOM
    return {"width": width, "height": height, "pitch": ops.exp2_pitch(width), "oy": oy, "ox": _EXP2_MARGIN, "step": side + _EXP2_GAP,
            "side": side, "bar_y": bar_y}


def _exp2_text(text: str, size: int) -> np.ndarray:
    """A line of text as grey indices [h, w] (black on white, nearest of the 16 greys)."""
    from PIL import Image, ImageDraw, ImageFont
    try:
        font = ImageFont.load_default(size)
    except (TypeError, OSError):
        font = ImageFont.load_default()
    l, t, r, b = font.getbbox(text or " ")
    img = Image.new("L", (max(r, 1) + 2, max(b, 1) + 2), 255)
    ImageDraw.Draw(img).text((1, 1), text, fill=0, font=font)
    g = np.asarray(img, dtype=np.int32)
    return (EXP2_IDX_GREY + (255 - g + 8) // 17).astype(np.uint8)


def _exp2_paste(dst: np.ndarray, src: np.ndarray, y: int, cx: int, width: int):
    """src centred on column cx with its top at row y, clipped to dst[:, :width]."""
    x = cx - src.shape[1] // 2
    y0, x0 = max(y, 0), max(x, 0)
    y1, x1 = min(y + src.shape[0], dst.shape[0]), min(x + src.shape[1], width)
    if y1 > y0 and x1 > x0:
        dst[y0:y1, x0:x1] = src[y0 - y:y1 - y, x0 - x:x1 - x]


def exp2_chrome(labels: Sequence[str], size: int, zoom: int) -> np.ndarray:
    """The static part of an event's frames as palette indices [height, pitch]: white, the panel titles, and the colour bar (141
    colours of equal width, as matplotlib spaces a BoundaryNorm bar; ticks at PAPER_BOUNDS; "Rainfall (mm/h)")."""
    lay = exp2_layout(len(labels), size, zoom)
    W = lay["width"]
    img = np.full((lay["height"], lay["pitch"]), EXP2_IDX_GREY, dtype=np.uint8)
    for p, label in enumerate(labels):
        _exp2_paste(img, _exp2_text(label, 11), _EXP2_STRIP + 1, lay["ox"] + p * lay["step"] + lay["side"] // 2, W)
    x0, bw = _EXP2_MARGIN, W - 2 * _EXP2_MARGIN
    ncol = EXP2_IDX_BAD
    img[lay["bar_y"]:lay["bar_y"] + _EXP2_BAR_H, x0:x0 + bw] = (np.arange(bw) * ncol // bw).astype(np.uint8)[None, :]
    bounds = paper_cmap()[0]
    pos = np.interp(np.asarray(PAPER_BOUNDS, float), bounds, np.arange(len(bounds))) / ncol
    for b, f in zip(PAPER_BOUNDS[:-1], pos[:-1]):
        _exp2_paste(img, _exp2_text(f"{b:g}", 8), lay["bar_y"] + _EXP2_BAR_H + 1, x0 + int(f * bw), W)
    _exp2_paste(img, _exp2_text("Rainfall (mm/h)", 10), lay["bar_y"] + _EXP2_BAR_H + _EXP2_TICK_H, W // 2, W)
    return img


def write_exp2_gif(canvases: np.ndarray, palette: np.ndarray, path: str, fps: int) -> None:
    """The frames as one GIF of the given palette (no quantisation: the file's colours are the palette's), frame duration
    int(1000 / max(fps, 1)) ms, looping forever, as the reference saves it."""
    from PIL import Image
    imgs = []
    for c in canvases:
        im = Image.fromarray(np.ascontiguousarray(c, dtype=np.uint8))
        im.putpalette(np.asarray(palette, np.uint8).reshape(-1).tobytes())
        imgs.append(im)
    if not imgs:
        return
    duration = int(1000 / max(fps, 1))
    imgs[0].save(path, format="GIF", save_all=True, append_images=imgs[1:], duration=duration, loop=0, optimize=False)
