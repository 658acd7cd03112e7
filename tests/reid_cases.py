"""Painted people for the re-identification tests: figures of the 15-point skeleton with a shirt and trousers of a
colour each on NV12 surfaces, shared by tests/test_reid_cpu.py (the measurement behind the default match_thr) and
tests/test_reid_gpu.py."""
import numpy as np

SENTINEL = 0xA5
# (x, y) of the 15 PoseTrack key points in units of the figure's height; the box is 0.4 x 1
FIGURE15 = np.asarray([(.20, .08), (.20, .14), (.20, .00), (.05, .20), (.35, .20), (.00, .36), (.40, .36), (.02, .50),
                       (.38, .50), (.10, .52), (.30, .52), (.09, .76), (.31, .76), (.08, 1.0), (.32, 1.0)], np.float64)
SHIRT = (.03, .17, .37, .53)       # x0, y0, x1, y1 of the painted shirt, in units of the height
TROUSERS = (.07, .53, .33, 1.0)
BACKGROUND = (118, 120, 134)       # (Y, U, V)
MARGIN = 32                        # two people differ by at least this much in U or in V, shirt and trousers alike
NOISE = (10.0, 5.0)                # sigma of the luma and of the chroma noise
SHIFT, TINT = 12, 3                # the brightness shift and the tint between two sightings, at the most


def colours(n, seed):
    """n shirt and n trouser colours (Y, U, V), n <= 24: any two shirts, and any two trousers, are at least MARGIN
    apart in U or in V, and each is that far from the background.  The chroma values are the points of a grid of
    pitch MARGIN with a seeded offset, so they fall anywhere between the centres of the bins."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        du, dv = (int(v) for v in rng.integers(0, 16, 2))
        grid = [(40 + du + MARGIN * i, 40 + dv + MARGIN * j) for i in range(6) for j in range(6)]
        grid = [g for g in grid if max(abs(g[0] - BACKGROUND[1]), abs(g[1] - BACKGROUND[2])) >= MARGIN]
        pick = rng.permutation(len(grid))[:n]
        out.append([(int(rng.integers(50, 201)), grid[i][0], grid[i][1]) for i in pick])
    return out[0], out[1]


def poses15(rng, pos, height, scale=(1.0, 1.0), jitter=0.01):
    """People with their top-left corners at pos [P, 2] (picture pixels) -> kpts [P, 15, 3], bboxes [P, 5] float32 in
    the coordinates of the picture scaled by `scale`."""
    pos = np.asarray(pos, np.float64).reshape(-1, 2)
    P = len(pos)
    xy = FIGURE15[None] * height + pos[:, None, :] + rng.uniform(-jitter, jitter, (P, 15, 2)) * height
    kpts = np.empty((P, 15, 3), np.float32)
    kpts[..., :2] = xy * np.asarray(scale)
    kpts[..., 2] = 0.9
    bboxes = np.empty((P, 5), np.float32)
    bboxes[:, :2] = pos * np.asarray(scale)
    bboxes[:, 2:4] = (pos + (0.4 * height, height)) * np.asarray(scale)
    bboxes[:, 4] = 0.8
    return kpts, bboxes


def paint_nv12(rng, W, H, pitch, people, shift=0, tint=(0, 0), noise=NOISE):
    """A [H * 3 // 2, pitch] uint8 NV12 surface: the background, then every (x, y, height, shirt, trousers) of
    `people` in order, every colour moved by `shift` in Y and `tint` in (U, V), Gaussian noise on every sample, and
    SENTINEL in the pitch padding."""
    Y = np.full((H, W), float(BACKGROUND[0]))
    U, V = np.full((H // 2, W // 2), float(BACKGROUND[1])), np.full((H // 2, W // 2), float(BACKGROUND[2]))
    for x, y, h, shirt, trousers in people:
        for (x0, y0, x1, y1), c in ((SHIRT, shirt), (TROUSERS, trousers)):
            a, b = int(round(x + x0 * h)), int(round(x + x1 * h))
            t, u = int(round(y + y0 * h)), int(round(y + y1 * h))
            a, b, t, u = max(a, 0), min(b, W), max(t, 0), min(u, H)
            if a >= b or t >= u:
                continue
            Y[t:u, a:b] = c[0]
            U[t // 2:(u + 1) // 2, a // 2:(b + 1) // 2] = c[1]
            V[t // 2:(u + 1) // 2, a // 2:(b + 1) // 2] = c[2]
    Y = Y + shift + rng.normal(0, noise[0], Y.shape)
    U = U + tint[0] + rng.normal(0, noise[1], U.shape)
    V = V + tint[1] + rng.normal(0, noise[1], V.shape)
    s = np.full((H * 3 // 2, pitch), SENTINEL, np.uint8)
    s[:H, :W] = np.clip(np.rint(Y), 0, 255)
    s[H:, 0:W:2] = np.clip(np.rint(U), 0, 255)
    s[H:, 1:W:2] = np.clip(np.rint(V), 0, 255)
    return s


def noise_nv12(H, W, pitch, seed=0):
    """[H * 3 // 2, pitch] uint8: noise in the picture's columns, SENTINEL in the pitch padding."""
    s = np.full((H * 3 // 2, pitch), SENTINEL, np.uint8)
    s[:, :W] = np.random.default_rng(seed).integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
    return s
