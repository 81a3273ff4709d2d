"""DCTE_LQR_ALPHA without a device: the model, its goldens, the glue's refusal.

The model (tests/alpha_util.py) is one numpy line over the oracle's luma-plane
entry.  Alpha-weighted planes are not of the integer-luma form the oracle was
pinned on, so it is pinned again here against the reference's own transforms
(oracle/_ref, where built) and against the committed goldens made from them.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import dctenergy
import oracle_py as O
from alpha_util import (NS, WEIGHTS, alpha_map, alpha_plane, manifest_alpha, masked_frame,
                        random_rgba)
from golden_util import load_input, load_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _planes():
    yield "rgba_45x38", load_input("rgba_45x38.npy")
    for shape in [(1, 1), (2, 3), (5, 7), (17, 255), (33, 256), (9, 257), (130, 129)]:
        yield f"random{shape}", random_rgba(shape, 100 + shape[0])
    yield "mask_64x96", masked_frame()


@pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("n", NS)
def test_oracle_equals_reference_transforms_on_alpha_planes(n):
    for name, img in _planes():
        plane = alpha_plane(img)
        got = O.energy_map_luma(plane, n, 0.15, 0.85)
        assert np.array_equal(_bits(got), _bits(O.ref_energy_map_luma(plane, n, 0.15, 0.85))), name


def test_model_equals_committed_goldens():
    entries = manifest_alpha()["maps"]
    assert sorted((m["N"], m["edges"], m["textures"]) for m in entries) == \
        sorted((n, e, t) for n in NS for e, t in WEIGHTS)
    for m in entries:
        img = load_input(m["input"])
        assert list(img.shape) == m["shape"] and img.shape[2] == 4
        got = alpha_map(img, m["N"], m["edges"], m["textures"])
        assert np.array_equal(_bits(got), _bits(load_map(m["output"]))), m["output"]


@pytest.mark.parametrize("n", NS)
def test_opaque_alpha_is_the_rgb_map(n):
    """alpha = 255 everywhere: A / 255 is exactly 1, the plane is the RGB luma."""
    img = random_rgba((37, 53), 5)
    img[..., 3] = 255
    for e, t in WEIGHTS:
        assert np.array_equal(_bits(alpha_map(img, n, e, t)),
                              _bits(O.energy_map(np.ascontiguousarray(img[..., :3]), n, e, t)))


@pytest.mark.parametrize("n", NS)
def test_transparent_alpha_is_all_zero(n):
    img = random_rgba((37, 53), 6)
    img[..., 3] = 0
    for e, t in WEIGHTS:
        assert not _bits(alpha_map(img, n, e, t)).any()          # +0.0, not -0.0


def test_first_seam_depends_on_alpha():
    """A kernel that ignored alpha would cut other seams: on the golden RGBA
    frame the first seam of the alpha map differs from the RGB map's in every row."""
    img = load_input("rgba_45x38.npy")
    for n in NS:
        a = O.seam_find(alpha_map(img, n, 0.3, 0.7))
        b = O.seam_find(O.energy_map(np.ascontiguousarray(img[..., :3]), n, 0.3, 0.7))
        assert (a != b).all(), n


def test_constant_is_exported_and_matches_the_header():
    with open(os.path.join(ROOT, "include", "dctenergy.h")) as f:
        text = f.read()
    assert int(re.search(r"^#define DCTE_LQR_ALPHA (\d+)$", text, re.M).group(1)) == 2
    assert dctenergy.DCTE_LQR_ALPHA == 2 and "DCTE_LQR_ALPHA" in dctenergy.__all__
    assert int(re.search(r"^#define DCTE_ABI_VERSION (\d+)$", text, re.M).group(1)) == 2
    with open(os.path.join(ROOT, "dct-carver_amd", "plugin", "dcte_plugin.h")) as f:
        assert re.search(r"^#define DCTE_PLUGIN_ALPHA 4u$", f.read(), re.M)


def glue():
    """The plug-in glue as tests/fake_lqr links it (test_plugin_shim.fake)."""
    from test_plugin_shim import fake
    L = fake()
    L.dcte_plugin_build_ex.restype = ctypes.c_int
    L.dcte_plugin_build_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_int, ctypes.c_uint]
    L.dcte_plugin_lookup.restype = ctypes.c_int
    L.dcte_plugin_lookup.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.dcte_plugin_release.restype = None
    L.dcte_plugin_release.argtypes = [ctypes.c_void_p]
    return L


PLUGIN_ALPHA = 4
CACHE_BYTES = 4096            # a zeroed buffer larger than dcte_map_cache (no layout mirrored)


def test_glue_without_a_device_reports_enodev():
    if dctenergy.device_count() != 0:
        pytest.skip("a device is present: tests/test_alpha.py drives the glue on it")
    L = glue()
    img = load_input("rgba_45x38.npy")
    h, w = img.shape[:2]
    cache = ctypes.create_string_buffer(CACHE_BYTES)
    for flags in (PLUGIN_ALPHA, 0):
        st = L.dcte_plugin_build_ex(cache, img.ctypes.data, w, h, 4, w * 4, 8, 0.3, 0.7, 0, flags)
        assert st == dctenergy.DCTE_ENODEV, (flags, st)
        v = ctypes.c_float(-1.0)
        assert L.dcte_plugin_lookup(cache, 3, 4, w, h, 0, ctypes.byref(v)) == 0
        L.dcte_plugin_release(cache)
