"""DCTE_LQR_ALPHA on the device: liblqr energies and carving for RGBA layers.

Every energy of this semantics is computed in the reference's fp64 operation
order, so every comparison here is bit for bit (np.array_equal / torch.equal)
against the model of tests/alpha_util.py -- the alpha rule [liblqr,
unverified] over the oracle's luma-plane entry, itself pinned to the
reference's transforms (tests/test_alpha_cpu.py).
"""
import ctypes
import os

import numpy as np
import pytest

import dctenergy
import oracle_py as O
import vmap_util as V
from alpha_util import (NS, SHAPES, WEIGHTS, alpha_map, cpu_carve_loop, manifest_alpha,
                        random_rgba, tie_frames_rgba)
from golden_util import load_input, load_map
from seam_util import carve, random_seams
from stream_util import Case, Delay, run_alone, run_ordered, same

pytestmark = pytest.mark.gpu

ALPHA = dctenergy.DCTE_LQR_ALPHA
NTHREADS = max(1, min(16, len(os.sched_getaffinity(0))))
E, T = 0.3, 0.7


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def actx():
    """A default context: fp32 maps with tie refinement for the other semantics."""
    with dctenergy.Context(ngpus=1) as c:
        yield c


@pytest.fixture(scope="module")
def ex():
    with dctenergy.Context(ngpus=1, exact=True) as c:
        yield c


@pytest.fixture(scope="module")
def tau0():
    with dctenergy.Context(ngpus=1, tie_tau=0.0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, ref):
    return got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


# ---- 1. argument checks ------------------------------------------------------
def _einval(fn):
    with pytest.raises(dctenergy.DcteError) as ei:
        fn()
    assert ei.value.code == dctenergy.DCTE_EINVAL


def test_semantics_and_bpp_pairs(actx):
    rng = np.random.default_rng(0)
    xy = np.array([[1, 2], [3, 4]], np.int32)
    for bpp in (1, 2, 3):
        img = rng.integers(0, 256, (20, 24) + ((bpp,) if bpp > 1 else ()), dtype=np.uint8)
        _einval(lambda: actx.energy_map(img, 8, E, T, semantics=ALPHA))
        _einval(lambda: actx.energy_map2(img, 8, E, T, semantics=ALPHA))
        _einval(lambda: actx.energy_points(img, xy, 8, E, T, semantics=ALPHA))
        _einval(lambda: actx.carve(img, 2, 8, E, T, semantics=ALPHA))
        _einval(lambda: actx.resizer(img, 2, 8, E, T, semantics=ALPHA))
        _einval(lambda: actx.energy_image_u8(img, 8, E, T, semantics=ALPHA))
    rgba = random_rgba((20, 24), 1)
    # DCTE_LQR itself keeps refusing RGBA
    _einval(lambda: actx.energy_map(rgba, 8, E, T))
    _einval(lambda: actx.energy_points(rgba, xy, 8, E, T))
    _einval(lambda: actx.carve(rgba, 2, 8, E, T))
    _einval(lambda: actx.resizer(rgba, 2, 8, E, T))
    _einval(lambda: actx.energy_map(rgba, 3, E, T, semantics=ALPHA))       # N as ever
    assert _same_bits(actx.energy_map(rgba, 8, E, T, semantics=ALPHA), alpha_map(rgba, 8, E, T))


# ---- 2. golden maps ----------------------------------------------------------
def test_golden_maps(actx):
    for m in manifest_alpha()["maps"]:
        img = load_input(m["input"])
        got = actx.energy_map(img, m["N"], m["edges"], m["textures"], semantics=ALPHA)
        assert _same_bits(got, load_map(m["output"])), m["output"]
        assert actx.last_refined == 0


# ---- 3. shapes and borders; the arithmetic options are inert -----------------
@pytest.mark.parametrize("n", NS)
def test_shapes_and_borders_in_every_mode(actx, ex, tau0, n):
    for shape in SHAPES:
        img = random_rgba(shape, hash((n,) + shape) & 0xFFFF)
        for e, t in WEIGHTS:
            ref = alpha_map(img, n, e, t, nthreads=NTHREADS)
            for name, c in (("default", actx), ("exact", ex), ("tie_tau=0", tau0)):
                got = c.energy_map(img, n, e, t, semantics=ALPHA)
                assert _same_bits(got, ref), (shape, e, t, name)
                assert c.last_refined == 0, (shape, name)


# ---- 4. metamorphic ----------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_opaque_and_transparent_frames(actx, ex, n):
    img = random_rgba((97, 300), 40 + n)
    img[..., 3] = 255
    rgb = np.ascontiguousarray(img[..., :3])
    for e, t in WEIGHTS:
        assert _same_bits(actx.energy_map(img, n, e, t, semantics=ALPHA), ex.energy_map(rgb, n, e, t))
    img[..., 3] = 0
    for e, t in WEIGHTS:
        assert not _bits(actx.energy_map(img, n, e, t, semantics=ALPHA)).any()


@pytest.mark.parametrize("n", NS)
def test_ties_at_alpha_edges(actx, n):
    """Line art under a 0 / 255 mask: exact edge/texture ties, decided only by
    the reference's rounding, also where the mask cuts the lines."""
    for name, img in tie_frames_rgba(300, 60 + n).items():
        got = actx.energy_map(img, n, E, T, semantics=ALPHA)
        ref = alpha_map(img, n, E, T, nthreads=NTHREADS)
        bad = int((_bits(got) != _bits(ref)).sum())
        assert bad == 0, f"{name} N={n}: {bad} pixels differ"


# ---- 5. addressing -----------------------------------------------------------
AH, AW = 37, 261          # a second, 5-column tile at N = 8; 5 strips at N = 16


@pytest.fixture(scope="module")
def addr_frame():
    img = random_rgba((AH, AW), 77)
    img[:, 100:180, 3] //= 5
    return img, {n: alpha_map(img, n, E, T) for n in NS}


def _map_at(torch, c, img, n, off, stride):
    """The frame laid into a flat byte buffer at byte offset `off` with byte
    row stride `stride`, its last byte the buffer's last byte."""
    h, w = img.shape[:2]
    nbytes = off + (h - 1) * stride + 4 * w
    buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (h, 4 * w), (stride, 1), off)
    view.copy_(torch.from_numpy(img.reshape(h, 4 * w)).cuda())
    out = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
    c.energy_map_device(buf.data_ptr() + off, stride, w, h, 4, 0, h, 0, h, n, E, T,
                        out.data_ptr(), out.stride(0),
                        torch.cuda.current_stream().cuda_stream, semantics=ALPHA)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", NS)
def test_unaligned_bases_and_odd_row_strides(torch, actx, addr_frame, n):
    img, ref = addr_frame
    for off in (0, 1, 2, 3):
        for pad in (0, 1, 2, 3):
            got = _map_at(torch, actx, img, n, off, 4 * AW + pad)
            assert _same_bits(got, ref[n]), (off, pad)


def test_tile_heights_on_an_unaligned_frame(torch, addr_frame):
    img, ref = addr_frame
    with dctenergy.Context(ngpus=1) as c:
        for k, th in enumerate((1, 7, 8, 9, 33)):
            c.set_option(dctenergy.DCTE_OPT_TILE_H, th)
            for n in NS:
                got = _map_at(torch, c, img, n, 1 + k % 3, 4 * AW + 1 + (k + n) % 3)
                assert _same_bits(got, ref[n]), (th, n)


# ---- 6. bands, two ranges, orientations, several devices ---------------------
BH, BW = 140, 261


@pytest.fixture(scope="module")
def band_frame():
    img = random_rgba((BH, BW), 91)
    img[40:90, :, 3] //= 3
    return img, {n: alpha_map(img, n, E, T, nthreads=NTHREADS) for n in NS}


def test_bands_and_two_range_launch(torch, actx, band_frame):
    img, ref = band_frame
    frame = torch.from_numpy(img).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for n in NS:
        full = torch.empty((BH, BW), dtype=torch.float32, device="cuda")
        actx.energy_map_tensor(frame, full, n, E, T, semantics=ALPHA)
        torch.cuda.synchronize()
        assert _same_bits(full.cpu().numpy(), ref[n]), n
        parts = torch.full((BH, BW), -1.0, dtype=torch.float32, device="cuda")
        r = n // 2
        cuts = [0, 1, 2, 65, 66, 139, 140]
        for a, b in zip(cuts[:-1], cuts[1:]):
            lo, hi = max(0, a - (r - 1)), min(BH - 1, b - 1 + r)
            band = frame[lo:hi + 1].clone()
            actx.energy_map_tensor(band, parts[a:b], n, E, T, h=BH, in_row0=lo, y0=a, y1=b,
                                   semantics=ALPHA)
        torch.cuda.synchronize()
        assert torch.equal(full, parts), n
        for a0, a1, b0, b1 in [(0, 3, 136, 140), (10, 14, 60, 63), (5, 70, 80, 130), (5, 9, 9, 9)]:
            got = torch.full((BH, BW), -1.0, dtype=torch.float32, device="cuda")
            actx.energy_map_device2(frame.data_ptr(), frame.stride(0), BW, BH, 4, 0, BH, a0, a1, b0, b1,
                                    n, E, T, got[a0:].data_ptr(), got.stride(0), st, semantics=ALPHA)
            torch.cuda.synchronize()
            want = torch.full((BH, BW), -1.0, dtype=torch.float32, device="cuda")
            want[a0:a1] = full[a0:a1]
            want[b0:b1] = full[b0:b1]
            assert torch.equal(got, want), (n, (a0, a1, b0, b1))


def test_transposed_map2_and_same_device_split(actx, band_frame):
    img, ref = band_frame
    tr = np.ascontiguousarray(np.swapaxes(img, 0, 1))
    with dctenergy.Context(ngpus=3, same_device=True) as many:
        assert many.ndevices == 3
        for n in NS:
            ref_t = alpha_map(tr, n, E, T, nthreads=NTHREADS)
            one = actx.energy_map(img, n, E, T, semantics=ALPHA)
            one_t = actx.energy_map(img, n, E, T, semantics=ALPHA, transposed=True)
            assert _same_bits(one, ref[n]) and _same_bits(one_t, ref_t), n
            both = actx.energy_map2(img, n, E, T, semantics=ALPHA)
            assert _same_bits(both[0], one) and _same_bits(both[1], one_t), n
            assert actx.last_refined == 0
            assert _same_bits(many.energy_map(img, n, E, T, semantics=ALPHA), one), n
            assert _same_bits(many.energy_map(img, n, E, T, semantics=ALPHA, transposed=True), one_t), n
            both = many.energy_map2(img, n, E, T, semantics=ALPHA)
            assert _same_bits(both[0], one) and _same_bits(both[1], one_t), n


# ---- 7. points and the seam-band update --------------------------------------
@pytest.mark.parametrize("n", NS)
def test_points_host_and_device(torch, actx, tau0, band_frame, n):
    img, ref = band_frame
    rng = np.random.default_rng(n)
    xy = np.stack([rng.integers(0, BW, 500), rng.integers(0, BH, 500)], 1).astype(np.int32)
    xy[:4] = [[0, 0], [BW - 1, 0], [0, BH - 1], [BW - 1, BH - 1]]
    want = ref[n][xy[:, 1], xy[:, 0]]
    for c in (actx, tau0):
        assert _same_bits(c.energy_points(img, xy, n, E, T, semantics=ALPHA), want)
    assert actx.energy_points(img, xy[:0], n, E, T, semantics=ALPHA).shape == (0,)
    # the host entry refuses coordinates outside the frame, the device entry clamps them
    for bad in ([BW, 0], [0, BH], [-1, 3]):
        _einval(lambda: actx.energy_points(img, np.array([bad], np.int32), n, E, T, semantics=ALPHA))
    wild = xy.copy()
    wild[::3, 0] += BW
    wild[1::3, 1] -= BH
    frame, pts = torch.from_numpy(img).cuda(), torch.from_numpy(wild).cuda()
    out = torch.full((len(wild),), -1.0, dtype=torch.float32, device="cuda")
    actx.energy_points_tensor(frame, pts, out, n, E, T, semantics=ALPHA)
    torch.cuda.synchronize()
    cl = np.stack([np.clip(wild[:, 0], 0, BW - 1), np.clip(wild[:, 1], 0, BH - 1)], 1)
    assert _same_bits(out.cpu().numpy(), ref[n][cl[:, 1], cl[:, 0]])


def _carve_frames():
    return {"rgba_45x38": load_input("rgba_45x38.npy"), "random_70x301": random_rgba((70, 301), 23)}


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("n", NS)
def test_seam_carve_device_steps(torch, actx, n, inplace):
    """12 steps: after each, the frame is the carved frame and the map is the
    full alpha map of it, bit for bit (every recomputed pixel is fp64)."""
    for name, img in _carve_frames().items():
        h, w = img.shape[:2]
        px = torch.from_numpy(img).cuda()
        emap = torch.empty((h, w), dtype=torch.float32, device="cuda")
        actx.energy_map_tensor(px, emap, n, E, T, semantics=ALPHA)
        host = img
        for k in range(12):
            wk = w - k
            seam = random_seams(h, wk, 300 + 7 * k + n, 4)[k % 4]
            sd = torch.from_numpy(seam).cuda()
            src, smap = px[:, :wk], emap[:, :wk]
            if inplace:
                dst, dmap = px[:, :wk - 1], emap[:, :wk - 1]
            else:
                dst = torch.full((h, wk - 1, 4), 0xA5, dtype=torch.uint8, device="cuda")
                dmap = torch.full((h, wk - 1), -1.0, dtype=torch.float32, device="cuda")
            actx.seam_carve_tensor(src, sd, smap, dst, dmap, n, E, T, semantics=ALPHA)
            torch.cuda.synchronize()
            host = carve(host, seam)
            assert np.array_equal(dst.cpu().numpy(), host), (name, k)
            assert _same_bits(dmap.cpu().numpy(), alpha_map(host, n, E, T, nthreads=NTHREADS)), (name, k)
            if not inplace:
                px, emap = dst, dmap


# ---- 8. dcte_carve ------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", [4, 8, 16])
def test_carve_equals_cpu_loop(actx, n, transposed):
    img = load_input("rgba_45x38.npy")
    fr = np.ascontiguousarray(np.swapaxes(img, 0, 1)) if transposed else img
    want, want_cols = cpu_carve_loop(fr, 10, n, E, T)
    if transposed:
        want = np.ascontiguousarray(np.swapaxes(want, 0, 1))
    out, cols = actx.carve(img, 10, n, E, T, semantics=ALPHA, transposed=transposed)
    for k in range(10):
        assert np.array_equal(cols[k], want_cols[k]), f"seam {k}"
    assert np.array_equal(out, want)
    actx.set_option(dctenergy.DCTE_OPT_DP_BANDWISE, 1)
    try:
        out_b, cols_b = actx.carve(img, 10, n, E, T, semantics=ALPHA, transposed=transposed)
    finally:
        actx.set_option(dctenergy.DCTE_OPT_DP_BANDWISE, 0)
    assert np.array_equal(out_b, want) and np.array_equal(cols_b, want_cols)


# ---- 9. resizer ----------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
def test_resizer(actx, transposed):
    img = load_input("rgba_45x38.npy")
    depth = 8
    fr = np.ascontiguousarray(np.swapaxes(img, 0, 1)) if transposed else img
    back = (lambda a: np.swapaxes(a, 0, 1)) if transposed else (lambda a: a)
    _, want_cols = cpu_carve_loop(fr, depth, 8, E, T)
    with actx.resizer(img, depth, 8, E, T, semantics=ALPHA, transposed=transposed) as r:
        assert np.array_equal(r.cols, want_cols)
        vm = r.vmap()
        v = vm.T if transposed else vm
        assert np.array_equal(v, V.vmap_model(want_cols, fr.shape[1]))
        for k in (depth, 3):
            assert np.array_equal(r.render(-k),
                                  actx.carve(img, k, 8, E, T, semantics=ALPHA, transposed=transposed)[0])
        for delta in (depth, 2, -5):
            assert np.array_equal(r.render(delta), back(V.render_model(fr, v, delta))), delta
        seams = r.seams_image()
        assert np.array_equal(seams, V.seams_model(img, vm, depth))
        assert np.array_equal(seams[..., 3], img[..., 3])


# ---- 10. the u8 energy image ---------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_energy_image_u8(actx, n):
    img = load_input("rgba_45x38.npy")
    ref = alpha_map(img, n, E, T)
    for ch in (1, 4):
        got = actx.energy_image_u8(img, n, E, T, dctenergy.DCTE_NORM_LQR, ch, semantics=ALPHA)
        assert np.array_equal(got, O.normalize_lqr(ref, ch)), ("lqr", ch)
        got = actx.energy_image_u8(img, n, E, T, dctenergy.DCTE_NORM_PREVIEW, ch, semantics=ALPHA)
        assert np.array_equal(got, O.normalize_preview(ref, ch)), ("preview", ch)


# ---- 11. the stream contract ---------------------------------------------------
SH, SW = 300, 400


@pytest.fixture(scope="module")
def delay(torch):
    d = Delay(torch)
    assert d.ms >= 20.0, (d.ms, d.trace)
    return d


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _io(torch, true, decoy):
    t = _dev(torch, true)
    return (torch.empty_like(t), t, _dev(torch, decoy))


def _ordered(torch, c, delay, case, check):
    alone = run_alone(torch, c, case)
    from_decoy = run_alone(torch, c, case, "decoy")
    got, host_s = run_ordered(torch, c, case, delay)
    # repeated calls of one size: nothing to allocate, nothing to wait for
    assert delay.ms * 1e-3 >= 10 * host_s, (delay.ms, host_s)
    assert not all(same(a, d) for a, d in zip(alone, from_decoy)), "the decoy is no decoy"
    for k, (g, a) in enumerate(zip(got, alone)):
        assert same(g, a), f"{case.name}: output {k} differs from the call made alone"
    check(got)


@pytest.mark.parametrize("n", [8, 16, 4])
def test_map_is_ordered_on_its_stream(torch, actx, delay, n):
    img, decoy = random_rgba((SH, SW), 5), random_rgba((SH, SW), 6)
    px = _io(torch, img, decoy)
    out = torch.empty((SH, SW), dtype=torch.float32, device="cuda")

    def call(c, st):
        c.energy_map_device(px[0].data_ptr(), px[0].stride(0), SW, SH, 4, 0, SH, 0, SH, n, E, T,
                            out.data_ptr(), out.stride(0), st, semantics=ALPHA)

    def check(res):
        assert _same_bits(res[0], alpha_map(img, n, E, T, nthreads=NTHREADS))
    _ordered(torch, actx, delay, Case(f"alpha map n={n}", [px], [(out, -1.0)], call), check)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("n", [8, 16])
def test_seam_carve_is_ordered_on_its_stream(torch, actx, delay, n, inplace):
    img, dimg = random_rgba((SH, SW), 7), random_rgba((SH, SW), 8)
    seams = random_seams(SH, SW, 3, 2)
    maps = [alpha_map(f, n, E, T, nthreads=NTHREADS) for f in (img, dimg)]
    px, sm, mp = _io(torch, img, dimg), _io(torch, seams[0], seams[1]), _io(torch, maps[0], maps[1])
    px_out = torch.empty((SH, SW - 1, 4), dtype=torch.uint8, device="cuda")
    map_out = torch.empty((SH, SW - 1), dtype=torch.float32, device="cuda")

    def call(c, st):
        if inplace:
            c.seam_carve_tensor(px[0], sm[0], mp[0], px[0][:, :SW - 1], mp[0][:, :SW - 1], n, E, T,
                                stream=st, semantics=ALPHA)
            px_out.copy_(px[0][:, :SW - 1], non_blocking=True)
            map_out.copy_(mp[0][:, :SW - 1], non_blocking=True)
        else:
            c.seam_carve_tensor(px[0], sm[0], mp[0], px_out, map_out, n, E, T, stream=st,
                                semantics=ALPHA)

    def check(res):
        host = carve(img, seams[0])
        assert np.array_equal(res[0], host)
        assert _same_bits(res[1], alpha_map(host, n, E, T, nthreads=NTHREADS))
    _ordered(torch, actx, delay, Case(f"alpha carve n={n} inplace={inplace}", [px, sm, mp],
                                      [(px_out, 0xA5), (map_out, -1.0)], call), check)


# ---- 12. the plug-in glue -------------------------------------------------------
def test_glue_opt_in():
    from test_alpha_cpu import CACHE_BYTES, PLUGIN_ALPHA, glue
    L = glue()
    img = load_input("rgba_45x38.npy")
    h, w = img.shape[:2]
    cache = ctypes.create_string_buffer(CACHE_BYTES)
    v = ctypes.c_float()
    # without the flag: as before
    assert L.dcte_plugin_build_ex(cache, img.ctypes.data, w, h, 4, w * 4, 8, E, T, 1, 0) == dctenergy.DCTE_EINVAL
    assert L.dcte_plugin_lookup(cache, 3, 4, w, h, 0, ctypes.byref(v)) == 0
    L.dcte_plugin_release(cache)
    # the seam hook stays bpp 1 / 3: with it, an RGBA build still serves the maps
    for flags in (PLUGIN_ALPHA, PLUGIN_ALPHA | 1):
        for n in (8, 16):
            assert L.dcte_plugin_build_ex(cache, img.ctypes.data, w, h, 4, w * 4, n, E, T, 1, flags) == dctenergy.DCTE_OK
            got = np.empty((h, w), np.float32)
            got_t = np.empty((w, h), np.float32)
            for y in range(h):
                for x in range(w):
                    assert L.dcte_plugin_lookup(cache, x, y, w, h, 0, ctypes.byref(v)) == 1
                    got[y, x] = v.value
                    assert L.dcte_plugin_lookup(cache, y, x, h, w, 1, ctypes.byref(v)) == 1
                    got_t[x, y] = v.value
            L.dcte_plugin_release(cache)
            assert _same_bits(got, alpha_map(img, n, E, T)), (flags, n)
            assert _same_bits(got_t, alpha_map(np.ascontiguousarray(np.swapaxes(img, 0, 1)), n, E, T)), (flags, n)
    # no effect on RGB
    rgb = np.ascontiguousarray(img[..., :3])
    assert L.dcte_plugin_build_ex(cache, rgb.ctypes.data, w, h, 3, w * 3, 8, E, T, 0, PLUGIN_ALPHA | 2) == dctenergy.DCTE_OK
    assert L.dcte_plugin_lookup(cache, 5, 6, w, h, 0, ctypes.byref(v)) == 1
    assert np.float32(v.value) == O.energy_map(rgb, 8, E, T)[6, 5]
    L.dcte_plugin_release(cache)
