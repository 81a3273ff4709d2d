"""Seam visibility map without a device: the numpy model (tests/vmap_util.py)
is consistent with itself and with seam_util.carve, and the new entry points
refuse NULL handles."""
import ctypes

import numpy as np
import pytest

import dctenergy
import vmap_util as V
from golden_util import load_input
from seam_util import carve


def _cols(h, w, depth, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, w - k, h) for k in range(depth)]).astype(np.int32) \
        if depth else np.empty((0, h), np.int32)


@pytest.mark.parametrize("h,w,depth", [(5, 70, 69), (3, 64, 10), (4, 1, 0), (2, 200, 37)])
def test_model_rows_hold_each_level_once(h, w, depth):
    vm = V.vmap_model(_cols(h, w, depth, 1), w)
    assert vm.shape == (h, w)
    for row in vm:
        assert sorted(row[row > 0]) == [V.level(k) for k in range(depth)]
        assert (row == 0).sum() == w - depth


def test_model_clamps_like_the_carve():
    cols = np.array([[-1, 99, 3], [7, -5, 3]], np.int32)       # 2 steps, 3 rows, w = 6
    vm = V.vmap_model(cols, 6)
    assert vm.tolist() == [[1, 0, 0, 0, 0, 2], [2, 0, 0, 0, 0, 1], [0, 0, 0, 1, 2, 0]]


def test_model_shrink_equals_repeated_carve():
    img = load_input("natural_rgb_97x41.npy")
    h, w = img.shape[:2]
    cols = _cols(h, w, 12, 2)
    vm = V.vmap_model(cols, w)
    host = img
    for j in range(13):
        assert np.array_equal(V.render_model(img, vm, -j), host), j
        if j < 12:
            host = carve(host, cols[j])


@pytest.mark.parametrize("name", ["natural_rgb_97x41.npy", "rgba_45x38.npy",
                                  "natural_grey_200x120.npy"])
def test_model_enlarge_minus_inserted_is_the_frame(name):
    img = load_input(name)
    h, w = img.shape[:2]
    cols = _cols(h, w, 12, 3)
    cols[0, 0] = 0                       # an insert at x = 0: its left neighbour is itself
    vm = V.vmap_model(cols, w)
    for j in (1, 5, 12):
        big = V.render_model(img, vm, j)
        mask = V.inserted_mask(vm, j)
        assert big.shape[:2] == (h, w + j) and (mask.sum(1) == j).all()
        assert np.array_equal(big[~mask].reshape(img.shape), img)
    x0 = int(np.flatnonzero(vm[0] == 1)[0])
    assert x0 == 0 and np.array_equal(V.render_model(img, vm, 1)[0, 0], img[0, 0])


def test_model_seams_image():
    img = load_input("natural_rgb_97x41.npy")
    h, w = img.shape[:2]
    vm = V.vmap_model(_cols(h, w, 3, 4), w)
    out = V.seams_model(img, vm, 3)
    assert np.array_equal(out[-1], img[-1]) and np.array_equal(out[:, -1], img[:, -1])
    inner = vm[:-1, :-1]
    assert (out[:-1, :-1][inner == 3] == (0, 255, 0)).all()
    assert (out[:-1, :-1][inner == 1] == (0, 85, 0)).all()
    assert np.array_equal(out[:-1, :-1][inner == 0], img[:-1, :-1][inner == 0])


def test_null_handles_are_invalid_arguments():
    L = dctenergy.lib()
    E = dctenergy.DCTE_EINVAL
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert L.dcte_vmap_device(None, 0, p, 1, 4, 4, p, 4, None) == E
    assert L.dcte_vmap_render_device(None, 0, p, 4, 4, 4, 1, p, 4, 1, 0, p, 4, None) == E
    assert L.dcte_vmap_seams_u8_device(None, 0, p, 4, 4, 4, 1, p, 4, 1, p, 4, None) == E
    r = ctypes.c_void_p()
    assert L.dcte_resizer_create(None, p, 4, 4, 1, 4, 8, 0.5, 0.5, 0, 1, 0, None,
                                 ctypes.byref(r)) == E
    assert not r.value
    assert L.dcte_resizer_render(None, 0, p) == E
    assert L.dcte_resizer_vmap(None, p) == E
    assert L.dcte_resizer_seams_u8(None, p) == E
    assert L.dcte_resizer_depth(None) == 0
    L.dcte_resizer_destroy(None)  # no-op


def test_new_names_are_exported():
    for name in ("dcte_vmap_device", "dcte_vmap_render_device", "dcte_vmap_seams_u8_device",
                 "dcte_resizer_create", "dcte_resizer_render", "dcte_resizer_vmap",
                 "dcte_resizer_seams_u8", "dcte_resizer_depth", "dcte_resizer_destroy"):
        assert name in dctenergy.EXPORTS
    assert dctenergy.lib().dcte_abi_version() == 2
