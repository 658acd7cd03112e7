"""ctypes binding of libpave_hip.so (C ABI declared in include/pave_hip.h).

The library is built in-tree by ``pavenet_amd.build_native`` (hipcc,
--offload-arch=gfx950).  There is NO fallback: if the shared object is missing
or a symbol is absent, importing the product ops raises.
"""
import contextlib
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libpave_hip.so')
DIAG_LIB_PATH = os.path.join(_HERE, 'lib', 'libpave_hip_diag.so')   # -DPAVE_DIAG build (tests/, tools/)

HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'pave_hip.h')   # the only description of the ABI

_c_int = ctypes.c_int
_vp = ctypes.c_void_p


class NativeLibraryError(RuntimeError):
    pass


_SCALARS = {'int': _c_int, 'long long': ctypes.c_longlong, 'float': ctypes.c_float, 'double': ctypes.c_double}
_RESTYPES = {'int': _c_int, 'long long': ctypes.c_longlong, 'const char*': ctypes.c_char_p}


def parse_header(text):
    """(functions, defines) of a C header in the style of include/pave_hip.h: functions[name] = (restype, argtypes)
    for every `ret pave_name(args);`, defines[name] = int for every integer `#define PAVE_*`.  A parameter is a
    pointer (c_void_p) or an int / long long / float / double by value.  Nothing is guessed: ctypes calls a function
    it has no argtypes for with C ints and truncates pointers without a word, so a `pave_name(` that is not part of
    a declaration typed here, or a parameter of any other type, raises NativeLibraryError."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    defines = {m.group(1): int(m.group(2)) for m in
               re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(PAVE_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    functions = {}
    for m in re.finditer(r'([\w\s*]+?)\b(pave_\w+)\s*\(([^()]*)\)\s*;', text):
        ret, name, params = re.sub(r'\s*\*\s*', '*', ' '.join(m.group(1).split())), m.group(2), m.group(3).strip()
        if ret not in _RESTYPES:
            raise NativeLibraryError(f'{name}: return type {ret!r} is not one of {sorted(_RESTYPES)}')
        argtypes = []
        for p in ([] if params == 'void' else params.split(',')):
            if '*' in p:
                argtypes.append(_vp)
                continue
            kind = ' '.join(w for w in p.split()[:-1] if w != 'const')     # (the last word is the parameter's name)
            if kind not in _SCALARS or '[' in p:
                raise NativeLibraryError(f'{name}: parameter {" ".join(p.split())!r} is neither a pointer nor one of '
                                         f'{sorted(_SCALARS)}')
            argtypes.append(_SCALARS[kind])
        functions[name] = (_RESTYPES[ret], argtypes)
    untyped = sorted(set(re.findall(r'\b(pave_\w+)\s*\(', text)) - set(functions))
    if untyped:
        raise NativeLibraryError(f'{", ".join(untyped)}: not a declaration of the form `ret pave_name(args);`')
    return functions, defines


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise NativeLibraryError(f'{HEADER_PATH} not readable ({e}): pavenet_amd types its entry points from the '
                                 f'header, there is no second table') from None


FUNCTIONS, DEFINES = _read_header()
EXPORTED = tuple(FUNCTIONS)        # every symbol include/pave_hip.h declares
# name -> argtypes of the entry points that return a status (0 = PAVE_OK): int, with arguments
SIGNATURES = {name: argtypes for name, (restype, argtypes) in FUNCTIONS.items() if restype is _c_int and argtypes}
ABI_VERSION = DEFINES['PAVE_ABI_VERSION']


class GnLevel(ctypes.Structure):
    """`pave_gn_level` of include/pave_hip.h (one map of pave_groupnorm_levels_nhwc_f32)."""
    _fields_ = [('x', ctypes.c_void_p), ('gamma', ctypes.c_void_p), ('beta', ctypes.c_void_p), ('y', ctypes.c_void_p),
                ('y_batch_stride', ctypes.c_longlong), ('HW', ctypes.c_int), ('nchunks', ctypes.c_int),
                ('eps', ctypes.c_float)]


AUG_MAX_AUGS, AUG_MAX_SLOTS, AUG_MAX_K = (DEFINES['PAVE_AUG_MAX_' + n] for n in ('AUGS', 'SLOTS', 'K'))


class AugPlan(ctypes.Structure):
    """`pave_aug_plan` of include/pave_hip.h (the by-value argument of pave_aug_merge_nms_f32)."""
    _fields_ = [('bboxes', ctypes.c_void_p * AUG_MAX_AUGS), ('kpts', ctypes.c_void_p * AUG_MAX_AUGS),
                ('keep', ctypes.c_void_p * AUG_MAX_AUGS), ('flip', ctypes.c_int32 * AUG_MAX_AUGS),
                ('img_w', ctypes.c_float * AUG_MAX_SLOTS), ('scale_factor', (ctypes.c_float * 4) * AUG_MAX_SLOTS),
                ('flip_perm', ctypes.c_int32 * AUG_MAX_K), ('n_aug', ctypes.c_int32), ('B', ctypes.c_int32),
                ('N', ctypes.c_int32), ('K', ctypes.c_int32)]


INGEST_MAX_SURFACES = DEFINES['PAVE_INGEST_MAX_SURFACES']
SCATTER_MAX_ROWS, SCATTER_MAX_TENSORS = DEFINES['PAVE_SCATTER_MAX_ROWS'], DEFINES['PAVE_SCATTER_MAX_TENSORS']


class IngestPlan(ctypes.Structure):
    """`pave_ingest_plan` of include/pave_hip.h (the by-value argument of pave_preprocess_surfaces_nv12)."""
    _fields_ = [('src', ctypes.c_void_p * INGEST_MAX_SURFACES), ('pitch', ctypes.c_int * INGEST_MAX_SURFACES),
                ('csc', (ctypes.c_float * 6) * INGEST_MAX_SURFACES), ('n', ctypes.c_int)]


class ScatterPlan(ctypes.Structure):
    """`pave_scatter_plan` of include/pave_hip.h (the by-value argument of pave_scatter_rows_f32)."""
    _fields_ = [('src', ctypes.c_void_p * SCATTER_MAX_TENSORS), ('dst', ctypes.c_void_p * SCATTER_MAX_TENSORS),
                ('row', ctypes.c_int * SCATTER_MAX_ROWS), ('n', ctypes.c_int), ('k', ctypes.c_int),
                ('dst_rows', ctypes.c_int), ('row_elems', ctypes.c_longlong)]


DRAW_MAX_SURFACES, DRAW_MAX_K, DRAW_MAX_E, DRAW_MAX_TABLES, DRAW_COLORS, DRAW_MAX_POSES, DRAW_MAX_SIZE = (
    DEFINES['PAVE_DRAW_' + n] for n in ('MAX_SURFACES', 'MAX_K', 'MAX_E', 'MAX_TABLES', 'COLORS', 'MAX_POSES',
                                        'MAX_SIZE'))


class DrawPlan(ctypes.Structure):
    """`pave_draw_plan` of include/pave_hip.h (the by-value argument of pave_draw_poses_nv12 / _bgr)."""
    _fields_ = [('dst', ctypes.c_void_p * DRAW_MAX_SURFACES), ('kpts', ctypes.c_void_p * DRAW_MAX_SURFACES),
                ('bboxes', ctypes.c_void_p * DRAW_MAX_SURFACES), ('keep', ctypes.c_void_p * DRAW_MAX_SURFACES),
                ('pitch', ctypes.c_int * DRAW_MAX_SURFACES), ('width', ctypes.c_int * DRAW_MAX_SURFACES),
                ('height', ctypes.c_int * DRAW_MAX_SURFACES), ('n_poses', ctypes.c_int * DRAW_MAX_SURFACES),
                ('scale', (ctypes.c_float * 2) * DRAW_MAX_SURFACES), ('table', ctypes.c_uint8 * DRAW_MAX_SURFACES),
                ('color', ((ctypes.c_uint8 * 3) * DRAW_COLORS) * DRAW_MAX_TABLES),
                ('edge', (ctypes.c_uint8 * 2) * DRAW_MAX_E), ('n', ctypes.c_int), ('K', ctypes.c_int),
                ('E', ctypes.c_int), ('thickness', ctypes.c_int), ('radius', ctypes.c_int),
                ('draw_boxes', ctypes.c_int), ('score_thr', ctypes.c_float), ('kpt_thr', ctypes.c_float)]


DRAW_PALETTE = DEFINES['PAVE_DRAW_PALETTE']


class DrawIdsPlan(ctypes.Structure):
    """`pave_draw_ids_plan` of include/pave_hip.h (the by-value argument of pave_draw_tracks_nv12 / _bgr)."""
    _fields_ = [('base', DrawPlan), ('ids', ctypes.c_void_p * DRAW_MAX_SURFACES),
                ('palette', ((ctypes.c_uint8 * 3) * (DRAW_PALETTE + 1)) * DRAW_MAX_TABLES),
                ('font', (ctypes.c_uint8 * 7) * 10), ('label_scale', ctypes.c_int), ('untracked_skip', ctypes.c_int)]


ANON_MAX_HEAD, ANON_MAX_CELL, ANON_MAX_MARGIN, ANON_MAX_SIXTEENTHS = (
    DEFINES['PAVE_ANON_MAX_' + n] for n in ('HEAD', 'CELL', 'MARGIN', 'SIXTEENTHS'))


class AnonPlan(ctypes.Structure):
    """`pave_anon_plan` of include/pave_hip.h (the by-value argument of pave_anonymize_nv12 / _bgr)."""
    _fields_ = [('dst', ctypes.c_void_p * DRAW_MAX_SURFACES), ('kpts', ctypes.c_void_p * DRAW_MAX_SURFACES),
                ('bboxes', ctypes.c_void_p * DRAW_MAX_SURFACES), ('keep', ctypes.c_void_p * DRAW_MAX_SURFACES),
                ('pitch', ctypes.c_int * DRAW_MAX_SURFACES), ('width', ctypes.c_int * DRAW_MAX_SURFACES),
                ('height', ctypes.c_int * DRAW_MAX_SURFACES), ('n_poses', ctypes.c_int * DRAW_MAX_SURFACES),
                ('scale', (ctypes.c_float * 2) * DRAW_MAX_SURFACES), ('table', ctypes.c_uint8 * DRAW_MAX_SURFACES),
                ('fill', (ctypes.c_uint8 * 3) * DRAW_MAX_TABLES), ('head', ctypes.c_uint8 * ANON_MAX_HEAD),
                ('n', ctypes.c_int), ('K', ctypes.c_int), ('n_head', ctypes.c_int), ('region', ctypes.c_int),
                ('mode', ctypes.c_int), ('fallback_skip', ctypes.c_int), ('cell', ctypes.c_int),
                ('margin', ctypes.c_int), ('grow', ctypes.c_int), ('head_scale', ctypes.c_int),
                ('head_min', ctypes.c_int), ('score_thr', ctypes.c_float), ('kpt_thr', ctypes.c_float)]


TRACK_MAX_FRAMES, TRACK_MAX_POSES,TRACK_MAX_TRACKS, TRACK_MAX_K, TRACK_MAX_CAMERAS = (
    DEFINES['PAVE_TRACK_MAX_' + n] for n in ('FRAMES', 'POSES', 'TRACKS', 'K', 'CAMERAS'))


class TrackPlan(ctypes.Structure):
    """`pave_track_plan` of include/pave_hip.h (the by-value argument of pave_track_poses)."""
    _fields_ = [('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('n', ctypes.c_int * TRACK_MAX_FRAMES), ('camera', ctypes.c_int * TRACK_MAX_FRAMES),
                ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES), ('track_id', ctypes.c_void_p),
                ('track_last', ctypes.c_void_p), ('track_kpts', ctypes.c_void_p), ('track_vis', ctypes.c_void_p),
                ('track_area', ctypes.c_void_p), ('frame', ctypes.c_void_p), ('next_id', ctypes.c_void_p),
                ('dropped', ctypes.c_void_p), ('scratch', ctypes.c_void_p), ('C', ctypes.c_int * TRACK_MAX_K),
                ('entries', ctypes.c_int), ('cameras', ctypes.c_int), ('M', ctypes.c_int), ('K', ctypes.c_int),
                ('min_kpts', ctypes.c_int), ('max_age', ctypes.c_int), ('score_thr', ctypes.c_float),
                ('kpt_thr', ctypes.c_float)]


class TrackMotionPlan(ctypes.Structure):
    """`pave_track_motion_plan` of include/pave_hip.h (the by-value argument of pave_track_poses_motion)."""
    _fields_ = [('base', TrackPlan), ('track_vel', ctypes.c_void_p), ('track_hits', ctypes.c_void_p),
                ('gain', ctypes.c_int), ('max_predict', ctypes.c_int), ('new_gate', ctypes.c_int)]


class SmoothPlan(ctypes.Structure):
    """`pave_smooth_plan` of include/pave_hip.h (the by-value argument of pave_smooth_poses)."""
    _fields_ = [('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('n', ctypes.c_int * TRACK_MAX_FRAMES), ('camera', ctypes.c_int * TRACK_MAX_FRAMES),
                ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES), ('slot_id', ctypes.c_void_p),
                ('slot_last', ctypes.c_void_p), ('slot_pos', ctypes.c_void_p), ('slot_vel', ctypes.c_void_p),
                ('frame', ctypes.c_void_p), ('dropped', ctypes.c_void_p), ('entries', ctypes.c_int),
                ('cameras', ctypes.c_int), ('S', ctypes.c_int), ('K', ctypes.c_int), ('alpha_min', ctypes.c_int),
                ('beta', ctypes.c_int), ('velocity_gain', ctypes.c_int), ('max_age', ctypes.c_int),
                ('score_thr', ctypes.c_float), ('kpt_thr', ctypes.c_float)]


ZONE_MAX_ZONES, ZONE_MAX_LINES, ZONE_MAX_VERTICES, ZONE_MAX_ANCHOR_KPTS, ZONE_MAX_EVENTS = (
    DEFINES['PAVE_ZONE_MAX_' + n] for n in ('ZONES', 'LINES', 'VERTICES', 'ANCHOR_KPTS', 'EVENTS'))
ZONE_EVENT_WORDS, ZONE_COUNTER_WORDS, ZONE_GEOM_WORDS = (
    DEFINES['PAVE_ZONE_' + n] for n in ('EVENT_WORDS', 'COUNTER_WORDS', 'GEOM_WORDS'))


class ZonePlan(ctypes.Structure):
    """`pave_zone_plan` of include/pave_hip.h (the by-value argument of pave_zone_events)."""
    _fields_ = [('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_zones', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_dwell', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_events', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_n_events', ctypes.c_void_p * TRACK_MAX_FRAMES), ('n', ctypes.c_int * TRACK_MAX_FRAMES),
                ('camera', ctypes.c_int * TRACK_MAX_FRAMES), ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES),
                ('slot_id', ctypes.c_void_p), ('slot_last', ctypes.c_void_p), ('slot_pos', ctypes.c_void_p),
                ('slot_inside', ctypes.c_void_p), ('slot_alerted', ctypes.c_void_p), ('slot_streak', ctypes.c_void_p),
                ('slot_since', ctypes.c_void_p), ('frame', ctypes.c_void_p), ('dropped', ctypes.c_void_p),
                ('counters', ctypes.c_void_p), ('geometry', ctypes.c_void_p),
                ('anchor_kpt', ctypes.c_int * ZONE_MAX_ANCHOR_KPTS), ('entries', ctypes.c_int),
                ('cameras', ctypes.c_int), ('S', ctypes.c_int), ('K', ctypes.c_int), ('anchor', ctypes.c_int),
                ('n_anchor', ctypes.c_int), ('min_frames', ctypes.c_int), ('max_events', ctypes.c_int),
                ('max_age', ctypes.c_int), ('score_thr', ctypes.c_float), ('kpt_thr', ctypes.c_float)]


ZONE_DRAW_COLORS, ZONE_DRAW_ALERT, ZONE_DRAW_INK, ZONE_DRAW_FACES = (
    DEFINES['PAVE_ZONE_DRAW_' + n] for n in ('COLORS', 'ALERT', 'INK', 'FACES'))


class ZoneDrawPlan(ctypes.Structure):
    """`pave_zone_draw_plan` of include/pave_hip.h (the by-value argument of pave_draw_zones_nv12 / _bgr)."""
    _fields_ = [('dst', ctypes.c_void_p * DRAW_MAX_SURFACES), ('pitch', ctypes.c_int * DRAW_MAX_SURFACES),
                ('width', ctypes.c_int * DRAW_MAX_SURFACES), ('height', ctypes.c_int * DRAW_MAX_SURFACES),
                ('camera', ctypes.c_int * DRAW_MAX_SURFACES), ('table', ctypes.c_uint8 * DRAW_MAX_SURFACES),
                ('geometry', ctypes.c_void_p), ('counters', ctypes.c_void_p), ('slot_id', ctypes.c_void_p),
                ('slot_alerted', ctypes.c_void_p), ('slot_inside', ctypes.c_void_p),
                ('color', ((ctypes.c_uint8 * 3) * ZONE_DRAW_COLORS) * DRAW_MAX_TABLES),
                ('font', (ctypes.c_uint8 * 7) * ZONE_DRAW_FACES), ('n', ctypes.c_int), ('cameras', ctypes.c_int),
                ('S', ctypes.c_int), ('alpha', ctypes.c_int), ('alpha_occupied', ctypes.c_int),
                ('alpha_alert', ctypes.c_int), ('outline', ctypes.c_int), ('thickness', ctypes.c_int),
                ('arrow', ctypes.c_int), ('label_scale', ctypes.c_int), ('zone_label', ctypes.c_int),
                ('line_label', ctypes.c_int)]


REID_BINS, REID_CAP, REID_MIN_SAMPLES, REID_MAX_PART, REID_MAX_HITS, REID_NEVER = (
    DEFINES['PAVE_REID_' + n] for n in ('BINS', 'CAP', 'MIN_SAMPLES', 'MAX_PART', 'MAX_HITS', 'NEVER'))


class ReidDescribePlan(ctypes.Structure):
    """`pave_reid_describe_plan` of include/pave_hip.h (the by-value argument of pave_reid_describe_nv12 / _bgr)."""
    _fields_ = [('src', ctypes.c_void_p * TRACK_MAX_FRAMES), ('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES), ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('hist', ctypes.c_void_p * TRACK_MAX_FRAMES), ('count', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('pitch', ctypes.c_int * TRACK_MAX_FRAMES), ('width', ctypes.c_int * TRACK_MAX_FRAMES),
                ('height', ctypes.c_int * TRACK_MAX_FRAMES), ('n', ctypes.c_int * TRACK_MAX_FRAMES),
                ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES),
                ('part', ((ctypes.c_int * REID_MAX_PART) * 2) * 2), ('n_part', (ctypes.c_int * 2) * 2),
                ('entries', ctypes.c_int), ('K', ctypes.c_int), ('score_thr', ctypes.c_float),
                ('kpt_thr', ctypes.c_float)]


class ReidPlan(ctypes.Structure):
    """`pave_reid_plan` of include/pave_hip.h (the by-value argument of pave_reid_update_nv12 / _bgr)."""
    _fields_ = [('d', ReidDescribePlan), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_ids', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_sim', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('camera', ctypes.c_int * TRACK_MAX_FRAMES), ('person', ctypes.c_void_p), ('track', ctypes.c_void_p),
                ('last', ctypes.c_void_p), ('hits', ctypes.c_void_p), ('hist', ctypes.c_void_p),
                ('frame', ctypes.c_void_p), ('next', ctypes.c_void_p), ('dropped', ctypes.c_void_p),
                ('pairs', ctypes.c_void_p), ('cameras', ctypes.c_int), ('S', ctypes.c_int), ('max_lost', ctypes.c_int),
                ('match_thr', ctypes.c_int), ('min_hits', ctypes.c_int), ('gain', ctypes.c_int)]


POSTURE_CLASSES, POSTURE_PARTS, POSTURE_MAX_PART, POSTURE_MAX_EVENTS, POSTURE_EVENT_WORDS, POSTURE_COUNTER_WORDS = (
    DEFINES['PAVE_POSTURE_' + n] for n in ('CLASSES', 'PARTS', 'MAX_PART', 'MAX_EVENTS', 'EVENT_WORDS', 'COUNTER_WORDS'))
POSTURE_MAX_SLOPE, POSTURE_MAX_WAIT, POSTURE_HANDS_OFF = (
    DEFINES['PAVE_POSTURE_' + n] for n in ('MAX_SLOPE', 'MAX_WAIT', 'HANDS_OFF'))


class PosturePlan(ctypes.Structure):
    """`pave_posture_plan` of include/pave_hip.h (the by-value argument of pave_posture_events)."""
    _fields_ = [('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_posture', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_raw', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_hands', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_since', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_events', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_n_events', ctypes.c_void_p * TRACK_MAX_FRAMES), ('n', ctypes.c_int * TRACK_MAX_FRAMES),
                ('camera', ctypes.c_int * TRACK_MAX_FRAMES), ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES),
                ('slot_id', ctypes.c_void_p), ('slot_last', ctypes.c_void_p), ('slot_posture', ctypes.c_void_p),
                ('slot_since', ctypes.c_void_p), ('slot_upright', ctypes.c_void_p), ('slot_streak', ctypes.c_void_p),
                ('slot_alerted', ctypes.c_void_p), ('slot_hands', ctypes.c_void_p),
                ('slot_hand_streak', ctypes.c_void_p), ('frame', ctypes.c_void_p), ('dropped', ctypes.c_void_p),
                ('counters', ctypes.c_void_p), ('part', (ctypes.c_int * POSTURE_MAX_PART) * POSTURE_PARTS),
                ('n_part', ctypes.c_int * POSTURE_PARTS), ('entries', ctypes.c_int), ('cameras', ctypes.c_int),
                ('S', ctypes.c_int), ('K', ctypes.c_int), ('min_frames', ctypes.c_int), ('lean', ctypes.c_int),
                ('flat', ctypes.c_int), ('squat', ctypes.c_int), ('hand_up', ctypes.c_int),
                ('fall_window', ctypes.c_int), ('down_frames', ctypes.c_int), ('max_events', ctypes.c_int),
                ('max_age', ctypes.c_int), ('score_thr', ctypes.c_float), ('kpt_thr', ctypes.c_float)]


HEAT_MAX_GRID, HEAT_MAX_RADIUS, HEAT_MAX_HALF_LIFE, HEAT_MAX_TABLES = (
    DEFINES['PAVE_HEAT_MAX_' + n] for n in ('GRID', 'RADIUS', 'HALF_LIFE', 'TABLES'))


class HeatPlan(ctypes.Structure):
    """`pave_heat_plan` of include/pave_hip.h (the by-value argument of pave_heat_update)."""
    _fields_ = [('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_cell', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_dwell', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_visits', ctypes.c_void_p * TRACK_MAX_FRAMES), ('n', ctypes.c_int * TRACK_MAX_FRAMES),
                ('camera', ctypes.c_int * TRACK_MAX_FRAMES), ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES),
                ('slot_id', ctypes.c_void_p), ('slot_last', ctypes.c_void_p), ('slot_cell', ctypes.c_void_p),
                ('frame', ctypes.c_void_p), ('dropped', ctypes.c_void_p), ('peak', ctypes.c_void_p),
                ('dwell', ctypes.c_void_p), ('visits', ctypes.c_void_p),
                ('anchor_kpt', ctypes.c_int * ZONE_MAX_ANCHOR_KPTS), ('entries', ctypes.c_int),
                ('cameras', ctypes.c_int), ('S', ctypes.c_int), ('K', ctypes.c_int), ('anchor', ctypes.c_int),
                ('n_anchor', ctypes.c_int), ('width', ctypes.c_int), ('height', ctypes.c_int), ('cell', ctypes.c_int),
                ('radius', ctypes.c_int), ('half_life', ctypes.c_int), ('max_age', ctypes.c_int),
                ('score_thr', ctypes.c_float), ('kpt_thr', ctypes.c_float)]


class HeatDrawPlan(ctypes.Structure):
    """`pave_heat_draw_plan` of include/pave_hip.h (the by-value argument of pave_draw_heat_nv12 / _bgr)."""
    _fields_ = [('dst', ctypes.c_void_p * DRAW_MAX_SURFACES), ('pitch', ctypes.c_int * DRAW_MAX_SURFACES),
                ('width', ctypes.c_int * DRAW_MAX_SURFACES), ('height', ctypes.c_int * DRAW_MAX_SURFACES),
                ('camera', ctypes.c_int * DRAW_MAX_SURFACES), ('table', ctypes.c_uint8 * DRAW_MAX_SURFACES),
                ('map', ctypes.c_void_p), ('peak', ctypes.c_void_p), ('palette', ctypes.c_void_p),
                ('n', ctypes.c_int), ('cameras', ctypes.c_int), ('tables', ctypes.c_int), ('map_width', ctypes.c_int),
                ('map_height', ctypes.c_int), ('cell', ctypes.c_int), ('source', ctypes.c_int),
                ('full_scale', ctypes.c_int), ('alpha_max', ctypes.c_int), ('floor', ctypes.c_int),
                ('smooth', ctypes.c_int)]


TRAIL_MAX_POINTS, TRAIL_MAX_STRIDE, TRAIL_MAX_STEP, TRAIL_MAX_THICKNESS, TRAIL_MAX_RADIUS, TRAIL_MAX_FRAMES = (
    DEFINES['PAVE_TRAIL_MAX_' + n] for n in ('POINTS', 'STRIDE', 'STEP', 'THICKNESS', 'RADIUS', 'FRAMES'))


class TrailPlan(ctypes.Structure):
    """`pave_trail_plan` of include/pave_hip.h (the by-value argument of pave_trail_update)."""
    _fields_ = [('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_count', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_span', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_dist', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_path', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('n', ctypes.c_int * TRACK_MAX_FRAMES), ('camera', ctypes.c_int * TRACK_MAX_FRAMES),
                ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES), ('slot_id', ctypes.c_void_p),
                ('slot_last', ctypes.c_void_p), ('slot_pos', ctypes.c_void_p), ('slot_head', ctypes.c_void_p),
                ('slot_count', ctypes.c_void_p), ('slot_box', ctypes.c_void_p), ('pts', ctypes.c_void_p),
                ('when', ctypes.c_void_p), ('frame', ctypes.c_void_p), ('dropped', ctypes.c_void_p),
                ('anchor_kpt', ctypes.c_int * ZONE_MAX_ANCHOR_KPTS), ('entries', ctypes.c_int),
                ('cameras', ctypes.c_int), ('S', ctypes.c_int), ('K', ctypes.c_int), ('L', ctypes.c_int),
                ('anchor', ctypes.c_int), ('n_anchor', ctypes.c_int), ('stride', ctypes.c_int),
                ('min_step', ctypes.c_int), ('max_age', ctypes.c_int), ('score_thr', ctypes.c_float),
                ('kpt_thr', ctypes.c_float)]


class TrailDrawPlan(ctypes.Structure):
    """`pave_trail_draw_plan` of include/pave_hip.h (the by-value argument of pave_draw_trails_nv12 / _bgr)."""
    _fields_ = [('dst', ctypes.c_void_p * DRAW_MAX_SURFACES), ('pitch', ctypes.c_int * DRAW_MAX_SURFACES),
                ('width', ctypes.c_int * DRAW_MAX_SURFACES), ('height', ctypes.c_int * DRAW_MAX_SURFACES),
                ('camera', ctypes.c_int * DRAW_MAX_SURFACES), ('table', ctypes.c_uint8 * DRAW_MAX_SURFACES),
                ('slot_id', ctypes.c_void_p), ('slot_last', ctypes.c_void_p), ('slot_pos', ctypes.c_void_p),
                ('slot_head', ctypes.c_void_p), ('slot_count', ctypes.c_void_p), ('slot_box', ctypes.c_void_p),
                ('pts', ctypes.c_void_p), ('when', ctypes.c_void_p), ('frame', ctypes.c_void_p),
                ('palette', ((ctypes.c_uint8 * 3) * DRAW_PALETTE) * DRAW_MAX_TABLES), ('n', ctypes.c_int),
                ('cameras', ctypes.c_int), ('S', ctypes.c_int), ('L', ctypes.c_int), ('thickness', ctypes.c_int),
                ('thickness_tail', ctypes.c_int), ('head_radius', ctypes.c_int), ('tail_frames', ctypes.c_int),
                ('linger', ctypes.c_int)]

FLOOR_CALIB_WORDS, FLOOR_CALIB_BOUNDS, FLOOR_CALIB_VALID, FLOOR_OUT_WORDS = (
    DEFINES['PAVE_FLOOR_' + n] for n in ('CALIB_WORDS', 'CALIB_BOUNDS', 'CALIB_VALID', 'OUT_WORDS'))
FLOOR_MAX_MM, FLOOR_MAX_NEAR, FLOOR_MAX_UNIT, FLOOR_MAX_GAIN, FLOOR_MAX_HITS = (
    DEFINES['PAVE_FLOOR_MAX_' + n] for n in ('MM', 'NEAR', 'UNIT', 'GAIN', 'HITS'))


class FloorPlan(ctypes.Structure):
    """`pave_floor_plan` of include/pave_hip.h (the by-value argument of pave_floor_update)."""
    _fields_ = [('kpts', ctypes.c_void_p * TRACK_MAX_FRAMES), ('bboxes', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('keep', ctypes.c_void_p * TRACK_MAX_FRAMES), ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out_floor', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('n', ctypes.c_int * TRACK_MAX_FRAMES), ('camera', ctypes.c_int * TRACK_MAX_FRAMES),
                ('scale', (ctypes.c_float * 2) * TRACK_MAX_FRAMES), ('slot_id', ctypes.c_void_p),
                ('slot_last', ctypes.c_void_p), ('slot_hits', ctypes.c_void_p), ('slot_pos', ctypes.c_void_p),
                ('slot_vel', ctypes.c_void_p), ('slot_travel', ctypes.c_void_p), ('frame', ctypes.c_void_p),
                ('dropped', ctypes.c_void_p), ('calib', ctypes.c_void_p),
                ('anchor_kpt', ctypes.c_int * ZONE_MAX_ANCHOR_KPTS), ('entries', ctypes.c_int),
                ('cameras', ctypes.c_int), ('S', ctypes.c_int), ('K', ctypes.c_int), ('anchor', ctypes.c_int),
                ('n_anchor', ctypes.c_int), ('velocity_gain', ctypes.c_int), ('near', ctypes.c_int),
                ('unit', ctypes.c_int), ('origin_x', ctypes.c_int), ('origin_y', ctypes.c_int),
                ('max_age', ctypes.c_int), ('score_thr', ctypes.c_float), ('kpt_thr', ctypes.c_float)]


CONTACT_OUT_WORDS, CONTACT_EVENT_WORDS, CONTACT_COUNTER_WORDS = (
    DEFINES['PAVE_CONTACT_' + n] for n in ('OUT_WORDS', 'EVENT_WORDS', 'COUNTER_WORDS'))
CONTACT_MAX_RADIUS, CONTACT_MAX_RELEASE, CONTACT_MAX_LONG, CONTACT_MAX_EVENTS = (
    DEFINES['PAVE_CONTACT_MAX_' + n] for n in ('RADIUS', 'RELEASE', 'LONG', 'EVENTS'))


class ContactPlan(ctypes.Structure):
    """`pave_contact_plan` of include/pave_hip.h (the by-value argument of pave_contact_update)."""
    _fields_ = [('on', ctypes.c_void_p * TRACK_MAX_FRAMES), ('xy', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('ids', ctypes.c_void_p * TRACK_MAX_FRAMES), ('out', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_events', ctypes.c_void_p * TRACK_MAX_FRAMES),
                ('out_n_events', ctypes.c_void_p * TRACK_MAX_FRAMES), ('n', ctypes.c_int * TRACK_MAX_FRAMES),
                ('camera', ctypes.c_int * TRACK_MAX_FRAMES), ('slot_id', ctypes.c_void_p),
                ('slot_last', ctypes.c_void_p), ('slot_pos', ctypes.c_void_p), ('link', ctypes.c_void_p),
                ('since', ctypes.c_void_p), ('frame', ctypes.c_void_p), ('dropped', ctypes.c_void_p),
                ('counters', ctypes.c_void_p), ('entries', ctypes.c_int), ('cameras', ctypes.c_int),
                ('S', ctypes.c_int), ('radius', ctypes.c_int), ('release', ctypes.c_int),
                ('min_frames', ctypes.c_int), ('long_frames', ctypes.c_int), ('max_events', ctypes.c_int),
                ('max_age', ctypes.c_int)]


_lib = None


def _open(path):
    if not os.path.exists(path):
        raise NativeLibraryError(
            f'{path} not found: run `python -c "import __graft_entry__ as g; '
            f'g.build()"` (hipcc --offload-arch=gfx950). pavenet_amd has no '
            f'CPU or eager fallback for its HIP kernels.')
    lib = ctypes.CDLL(path)
    # entry points added without a signature change keep the ABI version: a library built before them lacks them
    missing = [n for n in EXPORTED if not hasattr(lib, n)]
    if missing:
        raise NativeLibraryError(
            f'{path} lacks {", ".join(missing)} (built from older sources): rebuild it '
            f'(`python -m pavenet_amd.build_native`)')
    for name, (restype, argtypes) in FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    have = lib.pave_abi_version()
    if have != ABI_VERSION:   # a stale .so against a newer header: the wrong argument list corrupts memory
        raise NativeLibraryError(
            f'{path} has ABI version {have}, this package expects {ABI_VERSION}: rebuild it '
            f'(`python -m pavenet_amd.build_native`)')
    return lib


def load():
    """Load libpave_hip.so (once) and type its entry points."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


_diag_lib = None


@contextlib.contextmanager
def diag_build(variant=0):
    """tests/ and tools/ only: inside the block every op of this package runs on the -DPAVE_DIAG
    build of the same sources with kernel-form override `variant` (enum PaveDiag in
    csrc/pave_internal.h lists the values); yields that library (it also has pave_diag_enc_tile_ablate).  The shipped library
    has no such switch, and is back in place when the block ends."""
    global _lib, _diag_lib
    if _diag_lib is None:
        _diag_lib = _open(DIAG_LIB_PATH)
        _diag_lib.pave_diag_gemm_variant.argtypes = [_c_int]
        _diag_lib.pave_diag_gemm_variant.restype = None
    product = load()
    _diag_lib.pave_diag_gemm_variant(int(variant))
    _lib = _diag_lib
    try:
        yield _diag_lib
    finally:
        _diag_lib.pave_diag_gemm_variant(0)
        _lib = product


def use_diag_build(variant=0):
    """tools/ only: run the rest of this process on the -DPAVE_DIAG build with override `variant`."""
    global _lib
    with diag_build(variant) as lib:
        pass
    lib.pave_diag_gemm_variant(int(variant))
    _lib = lib
    return lib


_SYNC_DEBUG = os.environ.get('PAVE_SYNC_DEBUG', '0') == '1'


def check(status, what):
    if status != 0:
        msg = load().pave_last_error().decode()
        raise RuntimeError(f'{what} failed with status {status}: {msg}')
    if _SYNC_DEBUG:   # fault localisation: every native launch is drained and reported
        import sys

        import torch
        torch.cuda.synchronize()
        print(f'[pave] {what} ok', file=sys.stderr, flush=True)
