"""The trail draw rule of DESIGN section 22 in numpy integers, restated from the rule: one camera's trail state (the
arrays of `TrackTrails.state()` and `points()`) and a style -> the bytes of a BGR picture or an NV12 surface.  The
coverage rule is section 13's, taken from its statement (tests/render_ref.py).  Only covered bytes are written."""
import numpy as np

from tests.render_ref import QMAX, bgr_to_yuv, covered, window
from tests.trail_ref import committed

NONE = -2 ** 62


def quarter(p):
    return min(max(int(p) >> 1, 0), QMAX)


def radii(n, thickness, thickness_tail):
    """The radius of capsule j = 0 .. n - 1 in quarter pixels."""
    return [2 * thickness_tail + 2 * (thickness - thickness_tail) * (j + 1) // n for j in range(n)]


def primitives(st, style):
    """[(key, A, B, r, palette row)] of every primitive of the camera, key = id * 128 + j."""
    out = []
    frame = int(st['frame'])
    for t in range(st['id'].shape[0]):
        ident = int(st['id'][t])
        if ident == 0 or (style.linger is not None and frame - int(st['last'][t]) > style.linger):
            continue
        pts = committed(st['pts'][t], st['when'][t], st['head'][t], st['count'][t])
        n = len(pts)
        pos = (quarter(st['pos'][t, 0]), quarter(st['pos'][t, 1]))
        ends = [(quarter(x), quarter(y)) for x, y, _ in pts] + [pos]
        row = ((ident - 1) & 0xffffffff) % 32
        for j, r in enumerate(radii(n, style.thickness, style.thickness_tail)):
            if style.tail_frames is None or frame - pts[j][2] <= style.tail_frames:
                out.append((ident * 128 + j, ends[j], ends[j + 1], r, row))
        if style.head_radius > 0:
            out.append((ident * 128 + n, pos, pos, 4 * style.head_radius, row))
    return out


def key_map(W, H, prims):
    """[H, W] int64: the largest key among the primitives covering each pixel, and its palette row; NONE where there
    is none."""
    keys, rows = np.full((H, W), NONE, np.int64), np.zeros((H, W), np.int64)
    for key, A, B, r, row in prims:
        lo_x, hi_x, lo_y, hi_y = window(A, B, r, W, H)
        if lo_x > hi_x or lo_y > hi_y:
            continue
        PX, PY = np.meshgrid(4 * np.arange(lo_x, hi_x + 1, dtype=np.int64), 4 * np.arange(lo_y, hi_y + 1, dtype=np.int64))
        top = covered(A, B, r, PX, PY) & (keys[lo_y:hi_y + 1, lo_x:hi_x + 1] < key)
        keys[lo_y:hi_y + 1, lo_x:hi_x + 1][top] = key
        rows[lo_y:hi_y + 1, lo_x:hi_x + 1][top] = row
    return keys, rows


def draw_bgr(image, st, style):
    """image [H, W, 3] uint8 -> the drawn copy."""
    out = np.array(image, dtype=np.uint8)
    H, W = out.shape[:2]
    keys, rows = key_map(W, H, primitives(st, style))
    colour = np.asarray(style.palette, np.uint8)[rows]
    return np.where((keys != NONE)[..., None], colour, out)


def draw_nv12(surface, width, st, style, matrix='bt601', full_range=False):
    """surface [H * 3 // 2, pitch] uint8 -> the drawn copy: Y where a luma pixel is covered; U, V of a chroma sample from
    the largest key over its 2 x 2 luma pixels."""
    out = np.array(surface, dtype=np.uint8)
    H, W = out.shape[0] * 2 // 3, int(width)
    keys, rows = key_map(W, H, primitives(st, style))
    yuv = np.asarray([bgr_to_yuv(c, matrix, full_range) for c in style.palette], np.uint8)
    out[:H, :W] = np.where(keys != NONE, yuv[rows, 0], out[:H, :W])
    k4 = keys.reshape(H // 2, 2, W // 2, 2).transpose(0, 2, 1, 3).reshape(H // 2, W // 2, 4)
    r4 = rows.reshape(H // 2, 2, W // 2, 2).transpose(0, 2, 1, 3).reshape(H // 2, W // 2, 4)
    top = k4.argmax(-1)
    ck, cr = np.take_along_axis(k4, top[..., None], -1)[..., 0], np.take_along_axis(r4, top[..., None], -1)[..., 0]
    chroma = out[H:, :W].reshape(H // 2, W // 2, 2)
    chroma[..., 0] = np.where(ck != NONE, yuv[cr, 1], chroma[..., 0])
    chroma[..., 1] = np.where(ck != NONE, yuv[cr, 2], chroma[..., 1])
    out[H:, :W] = chroma.reshape(H // 2, W)
    return out


def state_from(tracks, S, L, frame):
    """One camera's trail state as numpy, written directly.  tracks: dicts with slot, id, points (the committed points,
    oldest first, in pixels) and optionally pos (pixels; default the newest point), when (default: consecutive frames
    ending at `frame`), last (default `frame`) and head (the ring index of the newest point; default len(points) - 1,
    any other value wraps the ring)."""
    z = lambda *shape: np.zeros(shape, np.int32)
    st = dict(id=z(S), last=z(S), pos=z(S, 2), head=z(S), count=z(S), box=z(S, 4), pts=z(S, L, 2), when=z(S, L),
              frame=np.asarray(frame, np.int32), dropped=np.asarray(0, np.int32))
    for tr in tracks:
        t, n = tr['slot'], len(tr['points'])
        p8 = [(int(round(8 * x)), int(round(8 * y))) for x, y in tr['points']]
        pos = p8[-1] if tr.get('pos') is None else (int(round(8 * tr['pos'][0])), int(round(8 * tr['pos'][1])))
        head = tr.get('head', n - 1) % L
        when = tr.get('when') or list(range(frame - n + 1, frame + 1))
        for j in range(n):
            i = (head - n + 1 + j) % L
            st['pts'][t, i], st['when'][t, i] = p8[j], when[j]
        st['id'][t], st['last'][t], st['pos'][t], st['head'][t], st['count'][t] = tr['id'], tr.get('last', frame), pos, head, n
        xs, ys = [p[0] for p in p8 + [pos]], [p[1] for p in p8 + [pos]]
        st['box'][t] = min(xs), min(ys), max(xs), max(ys)
    return st
