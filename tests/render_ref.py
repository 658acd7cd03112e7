"""The drawing rule of DESIGN section 13 in numpy, written from the rule and not from the kernel: the oracle of
tests/test_render_cpu.py and tests/test_render_gpu.py.  Everything is int64 after the quantisation; a surface is
drawn by painting the id map (largest covering primitive id per pixel) and then storing colours where it is >= 0.

A `style` is anything with the fields of pavenet_amd.render.PoseStyle (K, edges, edge_colors, kpt_colors, bbox_color,
thickness, radius, score_thr, kpt_thr, draw_boxes): plain data here.
"""
import numpy as np

QMAX = 32767
MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}


def quantise(x, s):
    """Quarter pixels: clamp((int)rintf((x / s) * 4.f), 0, 32767), every step in fp32."""
    with np.errstate(all='ignore'):
        q = np.asarray(x, np.float32) / np.float32(s)
        v = np.rint(q * np.float32(4.0))
        return np.clip(np.nan_to_num(v, nan=0.0, posinf=QMAX, neginf=0.0), 0, QMAX).astype(np.int64)


def primitives(kpts, bboxes, keep, scale, style):
    """-> [(id, (ax, ay), (bx, by), r, ('box', 0) | ('limb', e) | ('kpt', k))] of the drawn poses, ascending id."""
    kpts, bboxes = np.asarray(kpts, np.float32), np.asarray(bboxes, np.float32)
    K, E = style.K, len(style.edges)
    per_pose, out = 4 + E + K, []
    sx, sy = scale
    for p in range(kpts.shape[0]):
        if keep is not None and int(keep[p]) == 0:
            continue
        if not bboxes[p, 4] > np.float32(style.score_thr):
            continue
        if not (np.isfinite(kpts[p, :, :2]).all() and np.isfinite(bboxes[p, :4]).all()):
            continue
        X, Y = quantise(kpts[p, :, 0], sx), quantise(kpts[p, :, 1], sy)
        vis = kpts[p, :, 2] > np.float32(style.kpt_thr)
        base = p * per_pose
        if style.draw_boxes:
            x1, x2 = (int(v) for v in quantise(bboxes[p, [0, 2]], sx))
            y1, y2 = (int(v) for v in quantise(bboxes[p, [1, 3]], sy))
            corners = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
            for i in range(4):
                out.append((base + i, corners[i], corners[(i + 1) % 4], 2 * style.thickness, ('box', 0)))
        for e, (a, b) in enumerate(style.edges):
            if vis[a] and vis[b]:
                out.append((base + 4 + e, (int(X[a]), int(Y[a])), (int(X[b]), int(Y[b])), 2 * style.thickness,
                            ('limb', e)))
        for k in range(K):
            if vis[k] and style.radius > 0:
                out.append((base + 4 + E + k, (int(X[k]), int(Y[k])), (int(X[k]), int(Y[k])), 4 * style.radius,
                            ('kpt', k)))
    return out


def covered(A, B, r, PX, PY):
    """The coverage rule for the points (PX, PY) (int64 arrays, quarter pixels) -> bool array."""
    ax, ay, bx, by, r = (np.int64(v) for v in (A[0], A[1], B[0], B[1], r))
    dx, dy = bx - ax, by - ay
    wx, wy = PX - ax, PY - ay
    L2 = dx * dx + dy * dy
    t = wx * dx + wy * dy
    near_a = wx * wx + wy * wy <= r * r
    near_b = (PX - bx) ** 2 + (PY - by) ** 2 <= r * r
    cross = wx * dy - wy * dx
    inside = cross * cross <= r * r * L2
    return np.where(t <= 0, near_a, np.where(t >= L2, near_b, inside))


def window(A, B, r, W, H, margin=0):
    """Pixel rows / columns that can be covered: the rest is farther than r from the segment's bounding box."""
    lo_x = max((min(A[0], B[0]) - r) // 4 - margin, 0)
    hi_x = min(-(-(max(A[0], B[0]) + r) // 4) + margin, W - 1)
    lo_y = max((min(A[1], B[1]) - r) // 4 - margin, 0)
    hi_y = min(-(-(max(A[1], B[1]) + r) // 4) + margin, H - 1)
    return lo_x, hi_x, lo_y, hi_y


def id_map(W, H, prims):
    """[H, W] int64: the largest id among the primitives covering each pixel, -1 where there is none."""
    ids = np.full((H, W), -1, np.int64)
    for pid, A, B, r, _ in prims:
        lo_x, hi_x, lo_y, hi_y = window(A, B, r, W, H)
        if lo_x > hi_x or lo_y > hi_y:
            continue
        PX, PY = np.meshgrid(4 * np.arange(lo_x, hi_x + 1, dtype=np.int64), 4 * np.arange(lo_y, hi_y + 1, dtype=np.int64))
        cov = covered(A, B, r, PX, PY)
        part = ids[lo_y:hi_y + 1, lo_x:hi_x + 1]
        part[cov & (part < pid)] = pid
    return ids


def bgr_to_yuv(bgr, matrix, full_range):
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yoff, cy, q = (0.0, 1.0, 1.0) if full_range else (16.0, 255.0 / 219.0, 255.0 / 224.0)
    b, g, r = (float(v) for v in bgr)
    yp = kr * r + kg * g + kb * b
    vals = (yoff + yp / cy, 128.0 + (b - yp) / (2.0 * (1.0 - kb)) / q, 128.0 + (r - yp) / (2.0 * (1.0 - kr)) / q)
    return tuple(int(min(max(np.rint(v), 0), 255)) for v in vals)


def _colour_of(style, prims):
    table = {}
    for pid, _, _, _, (kind, i) in prims:
        table[pid] = {'box': lambda i: style.bbox_color, 'limb': lambda i: style.edge_colors[i],
                      'kpt': lambda i: style.kpt_colors[i]}[kind](i)
    return table


def _paint(ids, colour_of, channel):
    """[H, W] of one stored byte per pixel (0 where ids < 0)."""
    lut = np.zeros(max(int(ids.max()), 0) + 1, np.uint8)
    for pid, colour in colour_of.items():
        if pid < lut.shape[0]:
            lut[pid] = colour[channel]
    return lut[np.maximum(ids, 0)]


def draw_bgr(image, kpts, bboxes, keep, scale, style):
    """image [H, W, 3] uint8 -> the drawn copy."""
    out = np.array(image, copy=True)
    H, W = out.shape[:2]
    prims = primitives(kpts, bboxes, keep, scale, style)
    ids = id_map(W, H, prims)
    colour_of = _colour_of(style, prims)
    for c in range(3):
        out[..., c] = np.where(ids >= 0, _paint(ids, colour_of, c), out[..., c])
    return out


def draw_nv12(surface, width, kpts, bboxes, keep, scale, style, matrix='bt601', full_range=False):
    """surface [H * 3 // 2, pitch] uint8 -> the drawn copy: Y where a luma pixel is covered; U, V of a chroma sample
    from the largest id over its 2 x 2 luma pixels."""
    out = np.array(surface, copy=True)
    H, W = out.shape[0] * 2 // 3, int(width)
    prims = primitives(kpts, bboxes, keep, scale, style)
    ids = id_map(W, H, prims)
    bgr = _colour_of(style, prims)
    yuv = {pid: bgr_to_yuv(c, matrix, full_range) for pid, c in bgr.items()}
    out[:H, :W] = np.where(ids >= 0, _paint(ids, yuv, 0), out[:H, :W])
    cids = ids.reshape(H // 2, 2, W // 2, 2).max(axis=(1, 3))
    chroma = out[H:, :W].reshape(H // 2, W // 2, 2)
    chroma[..., 0] = np.where(cids >= 0, _paint(cids, yuv, 1), chroma[..., 0])
    chroma[..., 1] = np.where(cids >= 0, _paint(cids, yuv, 2), chroma[..., 1])
    out[H:, :W] = chroma.reshape(H // 2, W)
    return out
