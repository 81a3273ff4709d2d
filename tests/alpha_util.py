"""Numpy model of DCTE_LQR_ALPHA (include/dctenergy.h): test infrastructure.

The one rule taken from liblqr without a liblqr to check it against [liblqr,
unverified] is alpha_plane(): LQR_ER_LUMA's reading of an RGBA pixel is the RGB
brightness times alpha / 255, in double.  Everything after it is DCTE_LQR's
own: the window, dctNxN and the last-maximum scan, through the oracle's
luma-plane entry (pinned bit for bit to the reference's transforms, oracle/_ref).
"""
import json
import os

import numpy as np

import oracle_py as O
from golden_util import GOLDEN
from seam_util import carve

NS = (2, 4, 8, 16)
WEIGHTS = ((0.15, 0.85), (0.5, 0.5))
SHAPES = [(1, 1), (1, 300), (300, 1), (2, 3), (5, 7), (8, 8), (17, 255), (33, 256),
          (9, 257), (130, 129), (260, 700)]


def alpha_plane(px):
    """H x W x 4 uint8 -> the luma plane of the rule, float64."""
    px = np.asarray(px, dtype=np.uint8)
    assert px.ndim == 3 and px.shape[2] == 4, px.shape
    return O.luma_plane(px[..., :3]) * (px[..., 3].astype(np.float64) / 255)


def alpha_map(px, n, e, t, nthreads=1):
    return O.energy_map_luma(alpha_plane(px), n, e, t, nthreads=nthreads)


def cpu_carve_loop(px, seams, n, e, t):
    """lqr_carver_resize's loop on the model: -> (carved frame, step columns)."""
    cols = []
    for _ in range(seams):
        s = O.seam_find(alpha_map(px, n, e, t))
        cols.append(s)
        px = carve(px, s)
    return px, np.array(cols, np.int32).reshape(seams, px.shape[0])


def random_rgba(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (4,), dtype=np.uint8)


def masked_frame(h=64, w=96, seed=11):
    """Random colours under a 0 / 255 alpha mask (blocks and a diagonal band)."""
    px = random_rgba((h, w), seed)
    yy, xx = np.mgrid[0:h, 0:w]
    px[..., 3] = np.where(((yy // 9 + xx // 13) & 1).astype(bool) | ((xx + yy) % 29 < 3), 255, 0)
    return px


def tie_frames_rgba(S, seed):
    """Line art, strokes and dots (exact edge/texture ties in real arithmetic)
    under a 0 / 255 alpha mask whose edges cut across the lines."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    line = np.where((yy % 23 == 0) | (xx % 31 == 0) | ((xx + 2 * yy) % 97 == 0), 0, 255).astype(np.uint8)
    ink = np.array([[20, 40, 200], [200, 30, 30], [0, 0, 0]], np.uint8)
    strokes = np.full((S, S, 3), 255, np.uint8)
    for k in range(3):
        strokes[((xx + (k + 1) * yy) % (41 + 6 * k)) == 0] = ink[k]
    dots = np.repeat(np.where(rng.random((S, S)) < 1 / 64, 255, 16).astype(np.uint8)[..., None], 3, -1)
    mask = np.where(((yy // 37 + xx // 53) & 1).astype(bool) | ((xx - yy) % 61 < 8), 255, 0).astype(np.uint8)
    out = {}
    for name, rgb in (("lineart", np.repeat(line[..., None], 3, -1)), ("strokes", strokes), ("dots", dots)):
        out[name] = np.ascontiguousarray(np.concatenate([rgb, mask[..., None]], -1))
    return out


def manifest_alpha():
    with open(os.path.join(GOLDEN, "manifest_alpha.json")) as f:
        return json.load(f)
