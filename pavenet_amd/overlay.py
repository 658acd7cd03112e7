"""What the ``ZoneMonitor`` knows, drawn into frames on the device (``csrc/pave_overlay.hip``):
zones tinted by their state (empty, occupied, somebody stayed too long), counting lines with a stem that points the
way a forward crossing goes, and the running counts as digits on small plates.  ``draw_zones_nv12`` composites into
the NV12 surfaces a hardware decoder handed out, ``draw_zones_bgr`` into [H, W, 3] BGR pictures, in place, one launch
per 32 surfaces on the caller's stream.  The monitor's geometry, counters and alert bits are read where they live, on
the device: no value is read on the host and the monitor's tensors are only read.

In the loop the call sits between hiding and drawing people, so skeletons lie over zones:

    anonymize_nv12(...); draw_zones_nv12(surface, width, monitor); draw_poses_nv12(...)

Geometry is in original-image pixels and so is the surface: there is no scale factor.  Hard-edged integer coverage as
in ``render.py``; the fills are blended with an integer alpha of 0 .. 256.

Not built: anti-aliasing, text other than digits and a minus, per-person dwell badges, flashing on events,
ground-plane zones.
"""
import numpy as np
import torch

from . import ops
from .render import DIGIT_FONT, MINUS_FACE, _bgr_triple, _per_surface, bgr_to_yuv
from .zones import MAX_LINES, MAX_ZONES, ZoneMonitor

ZONE_FONT = DIGIT_FONT + (MINUS_FACE,)      # the 11 faces of the plan: the digits, then the minus
# BGR, one per zone and per line: cool hues for places, warm ones for lines, all darker than white ink
ZONE_COLORS = ((200, 120, 40), (160, 160, 30), (190, 90, 110), (120, 150, 60), (210, 150, 90), (150, 100, 30),
               (170, 130, 130), (110, 170, 100))
LINE_COLORS = ((40, 170, 240), (60, 110, 230), (30, 200, 200), (90, 140, 250), (20, 140, 200), (80, 190, 230),
               (50, 90, 190), (100, 170, 210))


class ZoneStyle:
    """How zones and lines are drawn.  `zone_colors`, `line_colors`: 8 BGR triples each, by index; `alert_color`: a
    zone in which a track has stayed past its dwell time; `label_color`: the ink of the digits.  A zone's fill takes
    `alpha` of 256 parts of its colour, `alpha_occupied` while somebody is inside and `alpha_alert` while alerted
    (0 .. 256 each; 0: no fill).  `outline` 0 .. 32 px: the zone's edges (0: none); `thickness` 1 .. 32 px: a line;
    `arrow` 0 .. 255 px: the stem from the line's middle towards the side a forward crossing ends on (0: none).
    `label_scale` g in 0 .. 8: a font pixel is g x g picture pixels (0: no labels).  `zone_label`: 'occupancy' (the
    tracks inside now) | 'entered' (entered + appeared) | 'none'; `line_label`: 'net' (forward - backward) | 'forward'
    | 'backward' | 'none'."""

    def __init__(self, zone_colors=ZONE_COLORS, line_colors=LINE_COLORS, alert_color=(36, 36, 242),
                 label_color=(255, 255, 255), alpha=48, alpha_occupied=96, alpha_alert=128, outline=2, thickness=3,
                 arrow=24, label_scale=2, zone_label='occupancy', line_label='net'):
        who = 'ZoneStyle'
        for name, colors, n in (('zone_colors', zone_colors, MAX_ZONES), ('line_colors', line_colors, MAX_LINES)):
            try:
                colors = list(colors)
            except TypeError:
                colors = []
            if len(colors) != n:
                raise ValueError(f'{who}: {name} is {n} BGR triples, got {len(colors)}')
            setattr(self, name, [_bgr_triple(c, f'{who}: a colour of {name}') for c in colors])
        self.alert_color = _bgr_triple(alert_color, f'{who}: alert_color')
        self.label_color = _bgr_triple(label_color, f'{who}: label_color')
        for name, v, lo, hi in (('alpha', alpha, 0, 256), ('alpha_occupied', alpha_occupied, 0, 256),
                                ('alpha_alert', alpha_alert, 0, 256), ('outline', outline, 0, 32),
                                ('thickness', thickness, 1, 32), ('arrow', arrow, 0, 255),
                                ('label_scale', label_scale, 0, 8)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
            setattr(self, name, int(v))
        if zone_label not in ops.ZONE_LABELS:
            raise ValueError(f"{who}: zone_label is 'occupancy', 'entered' or 'none', got {zone_label!r}")
        if line_label not in ops.LINE_LABELS:
            raise ValueError(f"{who}: line_label is 'net', 'forward', 'backward' or 'none', got {line_label!r}")
        self.zone_label, self.line_label = zone_label, line_label

    def color_table(self):
        """The [18, 3] BGR table of the plan: rows 0 .. 7 zones, 8 .. 15 lines, 16 the alert colour, 17 the ink."""
        return np.asarray(self.zone_colors + self.line_colors + [self.alert_color, self.label_color], dtype=np.uint8)

    def table_bytes(self, matrix=None, full_range=False):
        """color_table as the 54 bytes of the plan: BGR (matrix None) or the (Y, U, V) of a matrix and range; kept per
        colour set, so a style drawn every frame converts its colours once."""
        table = self.color_table()
        key = (matrix, bool(full_range), table.tobytes())
        cache = self.__dict__.setdefault('_tables', {})
        if key not in cache:
            cache[key] = (table if matrix is None else bgr_to_yuv(table, matrix, full_range)).tobytes()
        return cache[key]


def _gather(surfaces, monitor, camera, style, who):
    """-> (surfaces, cameras, style): lists of one entry per surface.  Every refusal a host can see."""
    surf = [surfaces] if isinstance(surfaces, torch.Tensor) else (
        list(surfaces) if isinstance(surfaces, (list, tuple)) else None)
    if not surf or any(not (isinstance(s, torch.Tensor) and s.dtype == torch.uint8) for s in surf):
        raise ValueError(f'{who}: one uint8 tensor or a non-empty list of them')
    if not isinstance(monitor, ZoneMonitor):
        raise ValueError(f'{who}: monitor is a ZoneMonitor, got {type(monitor).__name__}')
    if style is None:
        style = ZoneStyle()
    if not isinstance(style, ZoneStyle):
        raise ValueError(f'{who}: style is a ZoneStyle')
    cams = [monitor._camera(c, who) for c in _per_surface(camera, len(surf), 'camera', (int, np.integer), who)]
    state = monitor.device_tensors()
    return surf, cams, style, state


def _where(surf, state, who):
    """After the shapes: the surfaces live on a HIP device, the monitor's when it has a state."""
    for i, s in enumerate(surf):
        if not s.is_cuda:
            raise ValueError(f'{who}: surface {i} must be a HIP device tensor (pavenet_amd has no CPU path)')
        if state is not None and s.device != state['id'].device:
            raise ValueError(f"{who}: surface {i} is on {s.device}, the monitor's state on {state['id'].device}")


def _draw(kind, items, state, tables, style):
    ops.draw_zones(kind, items, state, tables, ZONE_FONT, alpha=style.alpha, alpha_occupied=style.alpha_occupied,
                   alpha_alert=style.alpha_alert, outline=style.outline, thickness=style.thickness, arrow=style.arrow,
                   label_scale=style.label_scale, zone_label=style.zone_label, line_label=style.line_label)


def _nv12_size(s, w, i, who):
    """The checks of one NV12 surface that need no monitor: made even where nothing will be drawn."""
    if isinstance(w, bool) or not isinstance(w, (int, np.integer)):
        raise ValueError(f'{who}: the width of surface {i} must be an integer, got {w!r}')
    if s.dim() != 2:
        raise ValueError(f'{who}: surface {i} must be [H * 3 // 2, pitch], got {tuple(s.shape)}')
    rows, pitch = s.shape
    if rows % 3 != 0 or (rows * 2 // 3) % 2 != 0 or rows <= 0:
        raise ValueError(f'{who}: surface {i}: {rows} rows are not the 3/2 of an even height')
    if w <= 0 or w % 2 != 0:
        raise ValueError(f'{who}: surface {i}: width {w} must be even and positive')
    if w > pitch:
        raise ValueError(f'{who}: surface {i}: width {w} exceeds the pitch {pitch}')


def draw_zones_nv12(surfaces, width, monitor, camera=0, style=None, matrix='bt601', full_range=False):
    """Draws the zones, lines and counts of `monitor`, a ``ZoneMonitor``, into NV12 `surfaces` in place and returns
    `surfaces`.  surfaces, width, matrix and full_range: what ``draw_poses_nv12`` takes (one tensor or a list of any
    sizes; one value or one per surface); camera: whose geometry a surface shows, one index or one per surface;
    style: a ``ZoneStyle``.  More than 32 surfaces go in several launches.  A monitor that has no state yet draws
    nothing, and a camera without geometry leaves its surface untouched."""
    who = 'draw_zones_nv12'
    surf, cams, style, state = _gather(surfaces, monitor, camera, style, who)
    n = len(surf)
    widths = _per_surface(width, n, 'width', (int, np.integer), who)
    modes = list(zip(_per_surface(matrix, n, 'matrix', str, who),
                     (bool(f) for f in _per_surface(full_range, n, 'full_range', (bool, int), who))))
    combos = sorted(set(modes))
    tables = [style.table_bytes(m, f) for m, f in combos]
    for i, (s, w) in enumerate(zip(surf, widths)):
        _nv12_size(s, w, i, who)
    _where(surf, state, who)
    if state is not None:
        _draw('nv12', [(s, int(w), c, combos.index(md)) for s, w, c, md in zip(surf, widths, cams, modes)], state,
              tables, style)
    return surfaces


def draw_zones_bgr(images, monitor, camera=0, style=None):
    """Draws the zones, lines and counts of `monitor` into [H, W, 3] uint8 BGR device `images` (one tensor or a list,
    any sizes) in place and returns `images`; monitor, camera and style as in ``draw_zones_nv12``."""
    who = 'draw_zones_bgr'
    surf, cams, style, state = _gather(images, monitor, camera, style, who)
    for i, s in enumerate(surf):
        if s.dim() != 3 or s.shape[2] != 3 or s.shape[0] < 1 or s.shape[1] < 1:
            raise ValueError(f'{who}: surface {i} must be [H, W, 3], got {tuple(s.shape)}')
    _where(surf, state, who)
    if state is not None:
        _draw('bgr', [(s, None, c, 0) for s, c in zip(surf, cams)], state, [style.table_bytes()], style)
    return images
