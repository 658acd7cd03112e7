"""Track ids in the picture ("Track ids in the picture") in numpy, written from the rule and not
from the kernel: the oracle of tests/test_render_ids_cpu.py and tests/test_render_ids_gpu.py.  Validity,
quantisation, capsule coverage, the largest-id rule and the NV12 chroma rule are tests/render_ref.py's, by import;
this file adds the colour by id, the 'skip' mode and the label (plate and ink), pixel by pixel in Python integers.

A `style` is anything with the fields of pavenet_amd.render.TrackStyle (PoseStyle's, and label_color, label_scale,
untracked); `palette` (32 BGR triples) and `font` (10 digits x 7 rows of 5 bits) are plain data, passed in.
"""
import numpy as np

from tests import render_ref as RR


def drawn_poses(kpts, bboxes, keep, ids, style):
    """The poses that are drawn: section 13's validity, and under 'skip' an id >= 1 where the surface has ids."""
    kpts, bboxes = np.asarray(kpts, np.float32), np.asarray(bboxes, np.float32)
    out = []
    for p in range(kpts.shape[0]):
        if keep is not None and int(keep[p]) == 0:
            continue
        if not bboxes[p, 4] > np.float32(style.score_thr):
            continue
        if not (np.isfinite(kpts[p, :, :2]).all() and np.isfinite(bboxes[p, :4]).all()):
            continue
        if ids is not None and style.untracked == 'skip' and int(ids[p]) <= 0:
            continue
        out.append(p)
    return out


def label_geometry(box, scale, v, g):
    """(ax, ay, Wp, Hp, digits) of the label of id v >= 1 at scale g >= 1 over the fp32 box (x1, y1, x2, y2)."""
    x1, x2 = (int(q) for q in RR.quantise(np.asarray(box, np.float32)[[0, 2]], scale[0]))
    y1, y2 = (int(q) for q in RR.quantise(np.asarray(box, np.float32)[[1, 3]], scale[1]))
    digits = [int(c) for c in str(int(v))]
    n = len(digits)
    Wp, Hp = g * (6 * n + 1), 9 * g
    return min(x1, x2) >> 2, max((min(y1, y2) >> 2) - Hp, 0), Wp, Hp, digits


def ink_pixels(digits, g, font):
    """[(u, w)] of the ink, relative to (ax + g, ay + g)."""
    out = []
    for u in range(6 * g * len(digits)):
        if u % (6 * g) >= 5 * g:
            continue
        for w in range(7 * g):
            if (font[digits[u // (6 * g)]][w // g] >> (4 - (u % (6 * g)) // g)) & 1:
                out.append((u, w))
    return out


def id_map_and_colours(W, H, kpts, bboxes, keep, ids, scale, style, palette, font):
    """-> ([H, W] int64 map of the largest covering primitive id, -1 where none; {id: BGR})."""
    N = np.asarray(kpts).shape[0]
    per_pose = 4 + len(style.edges) + style.K
    drawn = drawn_poses(kpts, bboxes, keep, ids, style)
    mask = np.zeros(N, np.int32)
    mask[drawn] = 1
    prims = RR.primitives(kpts, bboxes, mask, scale, style)
    assert {pid // per_pose for pid, *_ in prims} <= set(drawn)
    id_of = RR.id_map(W, H, prims)
    colours = {}
    for pid, _, _, _, (kind, i) in prims:
        v = 0 if ids is None else int(ids[pid // per_pose])
        if kind == 'kpt':
            colours[pid] = style.kpt_colors[i]
        elif v >= 1:
            colours[pid] = tuple(palette[(v - 1) % 32])
        else:
            colours[pid] = style.bbox_color if kind == 'box' else style.edge_colors[i]
    g = style.label_scale
    if ids is not None and g >= 1:
        for p in drawn:                      # ascending: a later label has the larger ids anyway
            v = int(ids[p])
            if v < 1:
                continue
            ax, ay, Wp, Hp, digits = label_geometry(np.asarray(bboxes, np.float32)[p, :4], scale, v, g)
            plate = N * per_pose + 2 * p
            colours[plate], colours[plate + 1] = tuple(palette[(v - 1) % 32]), tuple(style.label_color)
            part = id_of[ay:min(ay + Hp, H), ax:min(ax + Wp, W)]      # (clipped: pixels outside are not written)
            part[part < plate] = plate
            for u, w in ink_pixels(digits, g, font):
                px, py = ax + g + u, ay + g + w
                if px < W and py < H and id_of[py, px] < plate + 1:
                    id_of[py, px] = plate + 1
    return id_of, colours


def draw_bgr(image, kpts, bboxes, keep, ids, scale, style, palette, font):
    """image [H, W, 3] uint8 -> the drawn copy."""
    out = np.array(image, copy=True)
    H, W = out.shape[:2]
    id_of, colours = id_map_and_colours(W, H, kpts, bboxes, keep, ids, scale, style, palette, font)
    for c in range(3):
        out[..., c] = np.where(id_of >= 0, RR._paint(id_of, colours, c), out[..., c])
    return out


def draw_nv12(surface, width, kpts, bboxes, keep, ids, scale, style, palette, font, matrix='bt601', full_range=False):
    """surface [H * 3 // 2, pitch] uint8 -> the drawn copy; a chroma sample takes the largest id over its 2 x 2 luma
    pixels (so a sample under ink takes the ink's U, V for its whole block)."""
    out = np.array(surface, copy=True)
    H, W = out.shape[0] * 2 // 3, int(width)
    id_of, colours = id_map_and_colours(W, H, kpts, bboxes, keep, ids, scale, style, palette, font)
    yuv = {pid: RR.bgr_to_yuv(c, matrix, full_range) for pid, c in colours.items()}
    out[:H, :W] = np.where(id_of >= 0, RR._paint(id_of, yuv, 0), out[:H, :W])
    cids = id_of.reshape(H // 2, 2, W // 2, 2).max(axis=(1, 3))
    chroma = out[H:, :W].reshape(H // 2, W // 2, 2)
    chroma[..., 0] = np.where(cids >= 0, RR._paint(cids, yuv, 1), chroma[..., 0])
    chroma[..., 1] = np.where(cids >= 0, RR._paint(cids, yuv, 2), chroma[..., 1])
    out[H:, :W] = chroma.reshape(H // 2, W)
    return out
