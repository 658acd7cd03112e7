"""The zone drawing rule of DESIGN section 19 in numpy and Python integers, written from the rule and not from the
kernel: the oracle of tests/test_zone_draw_cpu.py and tests/test_zone_draw_gpu.py.  The capsule coverage test and the
colour conversion are tests/render_ref.py's, by import; the fill restates section 17's inside test on whole pixel
grids (tests/test_zone_draw_cpu.py ties it to tests/zones_ref.py's own, pixel by pixel).

A draw takes plain data: `geometry`, `counts` and `state` are what ZoneRef.geometry(c), .counts(c) and .state(c) (or
the monitor's views, as numpy) hold for one camera; `style` is anything with the fields of pavenet_amd.overlay.ZoneStyle;
`font` is 11 faces (the digits, then the minus) of 7 rows of 5 bits.
"""
import math

import numpy as np

from tests import render_ref as RR
from tests.smooth_ref import wrap32

QMAX = 32767
ALERT, INK = 16, 17                         # rows of the colour table after the 8 zones and the 8 lines


def blend(src, col, a):
    """out = (src (256 - a) + col a + 128) >> 8, on ints or int64 arrays."""
    return (src * (256 - a) + col * a + 128) >> 8


def fill_mask(W, H, polygon):
    """[H, W] bool: pixel (px, py) is the point (8 px, 8 py); inside by section 17's test, polygon in 1/8 pixel."""
    X, Y = np.meshgrid(8 * np.arange(W, dtype=np.int64), 8 * np.arange(H, dtype=np.int64))
    hit = np.zeros((H, W), bool)
    for i in range(len(polygon)):
        (ax, ay), (bx, by) = polygon[i], polygon[(i + 1) % len(polygon)]
        dy = by - ay
        t = (X - ax) * dy - (Y - ay) * (bx - ax)
        hit ^= ((ay > Y) != (by > Y)) & ((t < 0) if dy > 0 else (t > 0))
    return hit


def read_geometry(geometry):
    """-> (polygons, lines) in 1/8 pixel, counts clamped to 8 and 16 and vertex words to 0 .. 65535 as the kernel
    reads them; a zone without vertices stays in the list (its index counts) as an empty polygon."""
    nz, nl = min(max(int(geometry['n_zones']), 0), 8), min(max(int(geometry['n_lines']), 0), 8)
    clamp = lambda p: tuple(min(max(int(v), 0), 65535) for v in p)
    polygons = [[clamp(p) for p in np.asarray(geometry['zones'])[z, :min(max(int(geometry['n_vertices'][z]), 0), 16)]]
                for z in range(nz)]
    lines = [tuple(clamp(p) for p in np.asarray(geometry['lines'])[l]) for l in range(nl)]
    return polygons, lines


def zone_states(nz, counts, state, style):
    """-> [(colour row, alpha)] per zone: alerted iff a slot with id != 0 has the bit in inside and alerted."""
    bits = 0
    for ident, inside, alerted in zip(np.asarray(state['id']).tolist(), np.asarray(state['inside']).tolist(),
                                      np.asarray(state['alerted']).tolist()):
        if ident != 0:
            bits |= inside & alerted
    out = []
    for z in range(nz):
        if (bits >> z) & 1:
            out.append((ALERT, style.alpha_alert))
        elif int(counts['occupancy'][z]) > 0:
            out.append((z, style.alpha_occupied))
        else:
            out.append((z, style.alpha))
    return out


def glyphs(v):
    """The faces of the int32 v: an optional minus (face 10) and the decimal digits of |v|."""
    return ([10] if v < 0 else []) + [int(c) for c in str(abs(int(v)))]


def stem_of(line, arrow):
    """(M, T, drawn) of a line ((Ax, Ay), (Bx, By)) in 1/8 pixel, in quarter pixels."""
    (ax, ay), (bx, by) = ((p[0] >> 1, p[1] >> 1) for p in line)
    M = ((ax + bx) >> 1, (ay + by) >> 1)
    dx, dy = bx - ax, by - ay
    if arrow <= 0 or (dx == 0 and dy == 0):
        return M, M, False
    L = math.isqrt(dx * dx + dy * dy)
    trunc = lambda n: abs(n) // L * (1 if n >= 0 else -1)
    T = tuple(min(max(m + trunc(n * 4 * arrow), 0), QMAX) for m, n in zip(M, (-dy, dx)))
    return M, T, True


def plate_of(centre, n, g):
    """(ax, ay, Wp, Hp) of a plate of n glyphs at scale g about the pixel `centre`."""
    Wp, Hp = g * (6 * n + 1), 9 * g
    return max(centre[0] - Wp // 2, 0), max(centre[1] - Hp // 2, 0), Wp, Hp


def primitives(geometry, counts, state, style):
    """-> (capsules [(id, A, B, r, row)] in quarter pixels, labels [(plate id, (ax, ay, Wp, Hp), faces, row)])."""
    polygons, lines = read_geometry(geometry)
    states = zone_states(len(polygons), counts, state, style)
    g = style.label_scale
    capsules, labels = [], []
    for z, polygon in enumerate(polygons):
        if not polygon:
            continue
        Q = [(x >> 1, y >> 1) for x, y in polygon]
        if style.outline > 0:
            for e in range(len(Q)):
                capsules.append((16 * z + e, Q[e], Q[(e + 1) % len(Q)], 2 * style.outline, states[z][0]))
        if g >= 1 and style.zone_label != 'none':
            v = int(counts['occupancy'][z]) if style.zone_label == 'occupancy' else \
                wrap32(int(counts['entered'][z]) + int(counts['appeared'][z]))
            centre = ((sum(q[0] for q in Q) // len(Q)) >> 2, (sum(q[1] for q in Q) // len(Q)) >> 2)
            labels.append((144 + 2 * z, plate_of(centre, len(glyphs(v)), g), glyphs(v), states[z][0]))
    for l, line in enumerate(lines):
        (ax, ay), (bx, by) = ((p[0] >> 1, p[1] >> 1) for p in line)
        capsules.append((128 + l, (ax, ay), (bx, by), 2 * style.thickness, 8 + l))
        M, T, drawn = stem_of(line, style.arrow)
        if drawn:
            capsules.append((136 + l, M, T, 2 * style.thickness, 8 + l))
        if g >= 1 and style.line_label != 'none':
            fwd, back = int(counts['crossed'][l][0]), int(counts['crossed'][l][1])
            v = {'net': wrap32(fwd - back), 'forward': fwd, 'backward': back}[style.line_label]
            labels.append((160 + 2 * l, plate_of((T[0] >> 2, T[1] >> 2), len(glyphs(v)), g), glyphs(v), 8 + l))
    return capsules, labels


def id_map(W, H, geometry, counts, state, style, font):
    """-> ([H, W] int64 of the largest covering primitive id, -1 where none; {id: row of the colour table})."""
    capsules, labels = primitives(geometry, counts, state, style)
    ids = RR.id_map(W, H, [(pid, A, B, r, None) for pid, A, B, r, _ in capsules])
    rows = {pid: row for pid, _, _, _, row in capsules}
    g = style.label_scale
    for plate, (ax, ay, Wp, Hp), faces, row in labels:
        rows[plate], rows[plate + 1] = row, INK
        part = ids[ay:min(ay + Hp, H), ax:min(ax + Wp, W)]          # (clipped at the borders, never moved)
        part[part < plate] = plate
        for cell, face in enumerate(faces):
            for w in range(7 * g):
                for u in range(5 * g):
                    px, py = ax + g + 6 * g * cell + u, ay + g + w
                    if (font[face][w // g] >> (4 - u // g)) & 1 and px < W and py < H and ids[py, px] < plate + 1:
                        ids[py, px] = plate + 1
    return ids, rows


def fills(W, H, geometry, counts, state, style):
    """-> [(mask [H, W], row, alpha)] in ascending zone index, zones with alpha 0 or no vertices left out."""
    polygons, _ = read_geometry(geometry)
    states = zone_states(len(polygons), counts, state, style)
    return [(fill_mask(W, H, polygon), row, a) for polygon, (row, a) in zip(polygons, states) if polygon and a > 0]


def _table(style, convert=None):
    table = [tuple(c) for c in style.zone_colors] + [tuple(c) for c in style.line_colors] + \
            [tuple(style.alert_color), tuple(style.label_color)]
    return [tuple(int(v) for v in (c if convert is None else convert(c))) for c in table]


def draw_bgr(image, geometry, counts, state, style, font):
    """image [H, W, 3] uint8 -> the drawn copy."""
    out = np.array(image, copy=True)
    H, W = out.shape[:2]
    table = _table(style)
    acc = out.astype(np.int64)
    for mask, row, a in fills(W, H, geometry, counts, state, style):
        for c in range(3):
            acc[..., c] = np.where(mask, blend(acc[..., c], table[row][c], a), acc[..., c])
    ids, rows = id_map(W, H, geometry, counts, state, style, font)
    for pid in np.unique(ids[ids >= 0]):
        acc[ids == pid] = table[rows[int(pid)]]
    return acc.astype(np.uint8)


def draw_nv12(surface, width, geometry, counts, state, style, font, matrix='bt601', full_range=False):
    """surface [H * 3 // 2, pitch] uint8 -> the drawn copy.  Luma per pixel; a chroma sample once per zone with
    a_c = (a n + 2) >> 2 for its n luma pixels inside, and under a primitive the colour of the largest id over its
    2 x 2 luma pixels."""
    out = np.array(surface, copy=True)
    H, W = out.shape[0] * 2 // 3, int(width)
    table = _table(style, lambda c: RR.bgr_to_yuv(c, matrix, full_range))
    luma = out[:H, :W].astype(np.int64)
    chroma = out[H:, :W].reshape(H // 2, W // 2, 2).astype(np.int64)
    for mask, row, a in fills(W, H, geometry, counts, state, style):
        luma = np.where(mask, blend(luma, table[row][0], a), luma)
        ac = (a * mask.reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3)) + 2) >> 2
        for c in (0, 1):
            chroma[..., c] = np.where(ac > 0, blend(chroma[..., c], table[row][1 + c], ac), chroma[..., c])
    ids, rows = id_map(W, H, geometry, counts, state, style, font)
    cids = ids.reshape(H // 2, 2, W // 2, 2).max(axis=(1, 3))
    for pid in np.unique(ids[ids >= 0]):
        yuv = table[rows[int(pid)]]
        luma[ids == pid] = yuv[0]
        chroma[cids == pid] = yuv[1:]
    out[:H, :W] = luma.astype(np.uint8)
    out[H:, :W] = chroma.astype(np.uint8).reshape(H // 2, W)
    return out
