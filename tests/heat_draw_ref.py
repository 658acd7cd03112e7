"""The heat-map draw rule of DESIGN section 21 in numpy integers, restated from the rule: a map [Gh, Gw], its peak and
a style -> the bytes of a BGR picture or an NV12 surface.  Only bytes with a positive alpha on the map are written."""
import numpy as np

from tests.render_ref import bgr_to_yuv


def yuv_table(palette, matrix, full_range):
    """256 BGR rows -> their (Y, U, V) as a [256, 3] uint8 array, one colour at a time through the render oracle."""
    return np.asarray([bgr_to_yuv(c, matrix, full_range) for c in palette], np.uint8)


def levels(cells, scale):
    """L(c) = min(255, 255 max(v, 0) / scale) in int64."""
    v = np.maximum(np.asarray(cells, np.int64), 0)
    return np.minimum(255, 255 * v // int(scale))


def axis_weights(u, cell, G):
    """One axis of the smooth rule at half-pixel coordinates u -> (i0 clamped, i1 clamped, w0, w1)."""
    u = np.asarray(u, np.int64)
    t = u - cell
    i0 = t // (2 * cell)                     # floor
    f = t - 2 * cell * i0
    return np.clip(i0, 0, G - 1), np.clip(i0 + 1, 0, G - 1), 2 * cell - f, f


def sample(L, ux, uy, cell, smooth):
    """The level at every (uy, ux) of half-pixel coordinates: a [len(uy), len(ux)] int64 array."""
    Gh, Gw = L.shape
    if not smooth:                           # the cell of pixel (u - 1) / 2 (a chroma sample: of its block's first pixel)
        gx, gy = ((np.asarray(ux) - 1) // 2) // cell, ((np.asarray(uy) - 1) // 2) // cell
        return L[np.clip(gy, 0, Gh - 1)[:, None], np.clip(gx, 0, Gw - 1)[None, :]]
    xa, xb, wx0, wx1 = axis_weights(ux, cell, Gw)
    ya, yb, wy0, wy1 = axis_weights(uy, cell, Gh)
    total = (wy0[:, None] * (wx0[None, :] * L[ya[:, None], xa[None, :]] + wx1[None, :] * L[ya[:, None], xb[None, :]])
             + wy1[:, None] * (wx0[None, :] * L[yb[:, None], xa[None, :]] + wx1[None, :] * L[yb[:, None], xb[None, :]]))
    shift = 2 + 2 * (int(cell).bit_length() - 1)
    return (total + 2 * cell * cell) >> shift


def alpha_of(level, style):
    return np.where(level < style.floor, 0, (style.alpha_max * level + 128) >> 8)


def blend(src, col, a):
    return ((src.astype(np.int64) * (256 - a) + col.astype(np.int64) * a + 128) >> 8).astype(np.uint8)


def _scale(peak, style):
    m = ('dwell', 'visits').index(style.source)
    return style.full_scale if style.full_scale is not None else max(int(peak[m]), 1)


def draw_bgr(image, maps, size, cell, style):
    """image [H, W, 3] uint8; maps dict(dwell, visits, peak) of one camera; size the map's (width, height)."""
    out = np.array(image, dtype=np.uint8)
    H, W = min(out.shape[0], size[1]), min(out.shape[1], size[0])
    L = levels(maps[style.source], _scale(maps['peak'], style))
    lv = sample(L, 2 * np.arange(W) + 1, 2 * np.arange(H) + 1, cell, style.smooth)
    a = alpha_of(lv, style)
    col = np.asarray(style.palette, np.uint8)[lv]                     # [H, W, 3]
    mixed = blend(out[:H, :W], col, a[..., None])
    out[:H, :W] = np.where((a > 0)[..., None], mixed, out[:H, :W])
    return out


def draw_nv12(surface, width, maps, size, cell, style, matrix='bt601', full_range=False):
    """surface [H * 3 // 2, pitch] uint8."""
    out = np.array(surface, dtype=np.uint8)
    Hs = out.shape[0] * 2 // 3
    H, W = min(Hs, size[1]), min(width, size[0])
    yuv = yuv_table(style.palette, matrix, full_range)
    L = levels(maps[style.source], _scale(maps['peak'], style))
    lv = sample(L, 2 * np.arange(W) + 1, 2 * np.arange(H) + 1, cell, style.smooth)
    a = alpha_of(lv, style)
    out[:H, :W] = np.where(a > 0, blend(out[:H, :W], yuv[lv, 0], a), out[:H, :W])
    # the chroma samples of the blocks whose first pixel is on the map, from the level at the block's centre
    bx, by = np.arange(0, W, 2), np.arange(0, H, 2)
    lc = sample(L, 2 * bx + 2, 2 * by + 2, cell, style.smooth)
    ac = alpha_of(lc, style)
    rows = Hs + by // 2
    for ch in (1, 2):
        old = out[rows[:, None], (bx + ch - 1)[None, :]]
        out[rows[:, None], (bx + ch - 1)[None, :]] = np.where(ac > 0, blend(old, yuv[lc, ch], ac), old)
    return out
