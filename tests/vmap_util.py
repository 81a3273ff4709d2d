"""Numpy model of the seam visibility map (include/dctenergy.h, "seam
visibility map"): test infrastructure, no device.

The two conventions taken from liblqr without a liblqr to check them against
[liblqr, unverified] are one function each -- level() and inserted() -- as in
csrc/dcte_vmap.hip (vmap_level, vmap_inserted).
"""
import numpy as np


def level(k):
    """The number step k (0-based) leaves at the pixel it removes [liblqr, unverified]."""
    return k + 1


def inserted(left, here):
    """The pixel inserted left of `here` when enlarging: the per-channel integer
    mean with its left neighbour, truncated [liblqr, unverified]."""
    return ((left.astype(np.uint16) + here.astype(np.uint16)) // 2).astype(np.uint8)


def green(vis, depth):
    """255 * vis / depth in double, truncated (src/render.c:228-230)."""
    return (255.0 * np.asarray(vis, np.float64) / np.float64(depth)).astype(np.int64).astype(np.uint8)


def vmap_model(cols, w):
    """cols: depth x H step columns (each in its step's frame, clamped to it)
    -> H x w int32 visibility map."""
    cols = np.asarray(cols)
    depth, h = cols.shape
    out = np.zeros((h, w), np.int32)
    for y in range(h):
        alive = list(range(w))
        for k in range(depth):
            c = min(max(int(cols[k, y]), 0), len(alive) - 1)
            out[y, alive.pop(c)] = level(k)
    return out


def inserted_mask(vmap, delta):
    """H x (w + delta) bool, delta > 0: which output pixels render() inserts."""
    h, w = vmap.shape
    ins = (vmap > 0) & (vmap <= delta)
    mask = np.zeros((h, w + delta), bool)
    for y in range(h):
        pos = np.arange(w) + np.cumsum(ins[y])      # where pixel x itself lands
        mask[y, pos[ins[y]] - 1] = True
    return mask


def render_model(img, vmap, delta):
    """img H x w [x C] -> H x (w + delta) [x C]."""
    h, w = vmap.shape
    out = np.empty((h, w + delta) + img.shape[2:], np.uint8)
    for y in range(h):
        v = vmap[y]
        if delta <= 0:
            out[y] = img[y][(v == 0) | (v > -delta)]
        else:
            ins = (v > 0) & (v <= delta)
            pos = np.arange(w) + np.cumsum(ins)
            out[y, pos] = img[y]
            left = img[y][np.maximum(np.arange(w) - 1, 0)]
            out[y, pos[ins] - 1] = inserted(left, img[y])[ins]
    return out


def seams_model(img, vmap, depth):
    """The "Seams" layer in the caller's orientation: removed pixels painted
    (0, G, 0) (grey: G), alpha kept, last row and last column never painted."""
    out = img.copy()
    h, w = vmap.shape
    paint = vmap != 0
    paint[h - 1, :] = False
    paint[:, w - 1] = False
    g = green(vmap[paint], depth) if depth > 0 else np.zeros(0, np.uint8)
    if img.ndim == 2:
        out[paint] = g
    else:
        px = out[paint]
        px[:, 0] = 0
        px[:, 1] = g
        px[:, 2] = 0
        out[paint] = px
    return out
