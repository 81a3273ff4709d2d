"""Seam visibility map on the device (dcte_vmap_*_device, dcte_resizer_*)
against the numpy model of tests/vmap_util.py, Context.carve and the CPU
reference loop."""
import ctypes

import numpy as np
import pytest

import dctenergy
import oracle_py as O
import vmap_util as V
from golden_util import load_input
from seam_util import carve

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _synthetic_cols(h, w, depth, seed):
    """Random step columns in [0, w - k), a few outside it (the clamp)."""
    rng = np.random.default_rng(seed)
    if depth == 0:
        return np.empty((0, h), np.int32)
    cols = np.stack([rng.integers(0, w - k, h) for k in range(depth)]).astype(np.int32)
    cols[0, 0] = -1
    cols[depth // 2, h - 1] = w - depth // 2          # one past that step's last column
    cols[depth - 1, h // 2] = 2 ** 30
    if depth > 3:
        cols[1:3, 0] = 0                              # the same block again and again
    return cols


# (H, W, depth): down to one pixel across a word edge; exactly one word; one
# pixel past a word; no steps; either side of the one-word-per-lane limit
# (64 lanes x 64 bits = 4096) and of the four-word limit (16384); the general
# path with one 64-pixel pass per counted block (100003) and with several (300007)
VMAP_SHAPES = [(5, 70, 69), (3, 64, 10), (3, 65, 64), (4, 1, 0), (3, 4096, 33), (3, 4097, 300),
               (2, 16384, 40), (2, 16385, 40), (2, 100003, 40), (1, 300007, 30)]


@pytest.mark.parametrize("h,w,depth", VMAP_SHAPES)
def test_vmap_device_on_synthetic_seams(ctx, h, w, depth):
    torch = _torch()
    cols = _synthetic_cols(h, w, depth, 7 + w)
    vm = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    ctx.vmap_tensor(torch.from_numpy(cols).cuda(), vm)
    assert np.array_equal(vm.cpu().numpy(), V.vmap_model(cols, w))


@pytest.mark.parametrize("h,w,depth,pad", [(5, 70, 69, 3), (3, 4097, 50, 5), (2, 16500, 20, 1)])
def test_vmap_device_strided(ctx, h, w, depth, pad):
    torch = _torch()
    cols = _synthetic_cols(h, w, depth, 11)
    buf = torch.full((h, w + pad), -7, dtype=torch.int32, device="cuda")
    ctx.vmap_tensor(torch.from_numpy(cols).cuda(), buf[:, :w])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :w], V.vmap_model(cols, w))
    assert (got[:, w:] == -7).all()                   # nothing past the row


def test_vmap_device_bad_arguments(ctx):
    L = dctenergy.lib()
    torch = _torch()
    vm = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    s = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p
    E = dctenergy.DCTE_EINVAL
    assert L.dcte_vmap_device(ctx._h, 0, vp(s.data_ptr()), 8, 8, 4, vp(vm.data_ptr()), 8, None) == E
    assert L.dcte_vmap_device(ctx._h, 0, vp(s.data_ptr()), 2, 8, 4, vp(vm.data_ptr()), 7, None) == E
    assert L.dcte_vmap_device(ctx._h, 0, None, 2, 8, 4, vp(vm.data_ptr()), 8, None) == E
    assert L.dcte_vmap_device(ctx._h, 5, vp(s.data_ptr()), 2, 8, 4, vp(vm.data_ptr()), 8, None) == E


# ---- resizer against Context.carve and the model ---------------------------
@pytest.fixture(scope="module")
def natural(ctx):
    img = load_input("natural_rgb_97x41.npy")
    r = ctx.resizer(img, 12, 8)
    yield img, r, r.vmap()
    r.close()


def test_resizer_vmap_and_cols_equal_carve(ctx, natural):
    img, r, vm = natural
    _, cols = ctx.carve(img, 12, 8)
    assert r.depth == 12
    assert np.array_equal(r.cols, cols)
    assert np.array_equal(vm, V.vmap_model(cols, img.shape[1]))


@pytest.mark.parametrize("delta", [0, -1, -5, -12])
def test_resizer_shrink_equals_carve(ctx, natural, delta):
    img, r, _ = natural
    assert np.array_equal(r.render(delta), ctx.carve(img, -delta, 8)[0])


@pytest.mark.parametrize("delta", [1, 5, 12])
def test_resizer_enlarge_equals_model(ctx, natural, delta):
    img, r, vm = natural
    big = r.render(delta)
    assert big.shape == (img.shape[0], img.shape[1] + delta, 3)
    assert np.array_equal(big, V.render_model(img, vm, delta))
    mask = V.inserted_mask(vm, delta)
    assert np.array_equal(big[~mask].reshape(img.shape), img)


def test_resize_convenience(ctx, natural):
    img, r, _ = natural
    assert np.array_equal(ctx.resize(img, -5, 8), ctx.carve(img, 5, 8)[0])
    r5 = ctx.resizer(img, 5, 8)
    try:
        want = V.render_model(img, r5.vmap(), 5)
    finally:
        r5.close()
    assert np.array_equal(ctx.resize(img, 5, 8), want)


# ---- the reference's arithmetic --------------------------------------------
@pytest.fixture(scope="module")
def exact_ctx():
    c = dctenergy.Context(ngpus=1, exact=True)
    yield c
    c.close()


@pytest.mark.parametrize("n", [4, 8])
def test_resizer_exact_equals_cpu_reference_loop(exact_ctx, n):
    img = load_input("wilber_rgb_74x59.npy")
    with exact_ctx.resizer(img, 10, n, 0.3, 0.7) as r:
        host = img
        for k in range(10):
            ref_seam = O.seam_find(O.energy_map(host, n, 0.3, 0.7))
            assert np.array_equal(r.cols[k], ref_seam), f"seam {k}"
            host = carve(host, ref_seam)
        assert np.array_equal(r.render(-10), host)
        assert np.array_equal(r.vmap(), V.vmap_model(r.cols, img.shape[1]))


def test_resizer_keeps_the_mode_of_its_creation(ctx):
    """Everything a resizer computes with energies happens at creation."""
    img = load_input("wilber_rgb_74x59.npy")
    with ctx.resizer(img, 6, 8, 0.3, 0.7) as r:
        before = r.render(-6)
        ctx.set_option(dctenergy.DCTE_OPT_TIE_TAU, 1.0)
        try:
            assert np.array_equal(r.render(-6), before)
        finally:
            ctx.set_option(dctenergy.DCTE_OPT_TIE_TAU, -1)


# ---- transposed and formats --------------------------------------------------
def test_resizer_transposed(ctx):
    img = load_input("natural_rgb_73x59.npy")
    tr = np.ascontiguousarray(np.swapaxes(img, 0, 1))
    with ctx.resizer(img, 9, 8, 0.3, 0.7, transposed=True) as rt, \
            ctx.resizer(tr, 9, 8, 0.3, 0.7) as ru:
        assert np.array_equal(rt.cols, ru.cols)
        for delta in (9, -9, 4):
            got = rt.render(delta)
            assert got.shape == (img.shape[0] + delta, img.shape[1], 3)
            assert np.array_equal(got, np.swapaxes(ru.render(delta), 0, 1))
        vm = rt.vmap()
        assert vm.shape == img.shape[:2]
        assert np.array_equal(vm, ru.vmap().T)
        # the last row / column rule applies in the caller's orientation
        seams = rt.seams_image()
        assert np.array_equal(seams, V.seams_model(img, vm, 9))
        assert np.array_equal(seams[:-1, :-1],
                              np.swapaxes(ru.seams_image(), 0, 1)[:-1, :-1])


def test_resizer_rgba_preview(ctx):
    img = load_input("rgba_45x38.npy")
    assert img.shape[2] == 4 and len(np.unique(img[..., 3])) > 1
    for transposed in (False, True):
        with ctx.resizer(img, 6, 8, 0.3, 0.7, semantics=dctenergy.DCTE_PREVIEW,
                         transposed=transposed) as r:
            vm = r.vmap()
            fr, v = (np.swapaxes(img, 0, 1), vm.T) if transposed else (img, vm)
            back = (lambda a: np.swapaxes(a, 0, 1)) if transposed else (lambda a: a)
            for delta in (6, 2, -6):
                assert np.array_equal(r.render(delta), back(V.render_model(fr, v, delta)))
            # alpha is averaged like any channel
            big = back(r.render(6)) if transposed else r.render(6)
            mask = V.inserted_mask(v, 6)
            ys, xs = np.nonzero(mask)
            right = big[ys, xs + 1, 3].astype(int)
            left = big[ys, np.maximum(xs - 1, 0), 3].astype(int)
            left = np.where(xs == 0, right, left)
            assert np.array_equal(big[ys, xs, 3], (left + right) // 2)
            seams = r.seams_image()
            assert np.array_equal(seams, V.seams_model(img, vm, 6))
            assert np.array_equal(seams[..., 3], img[..., 3])


def test_resizer_grey_and_strided_source(ctx):
    img = load_input("natural_grey_200x120.npy")
    with ctx.resizer(img, 7, 8) as r:
        vm = r.vmap()
        assert np.array_equal(vm, V.vmap_model(r.cols, img.shape[1]))
        for delta in (7, -7, -3):
            assert np.array_equal(r.render(delta), V.render_model(img, vm, delta))
        assert np.array_equal(r.seams_image(), V.seams_model(img, vm, 7))
    view = img[:, 3:40]
    assert view.strides[0] != view.shape[1]
    dense = np.ascontiguousarray(view)
    with ctx.resizer(view, 5, 8, 0.3, 0.7) as rv, ctx.resizer(dense, 5, 8, 0.3, 0.7) as rd:
        assert np.array_equal(rv.cols, rd.cols)
        assert np.array_equal(rv.render(5), rd.render(5))
        assert np.array_equal(rv.render(-5), ctx.carve(dense, 5, 8, 0.3, 0.7)[0])
        assert np.array_equal(rv.seams_image(), V.seams_model(dense, rv.vmap(), 5))


# ---- seams image -------------------------------------------------------------
def test_seams_image_against_model(ctx, natural):
    img, r, vm = natural
    seams = r.seams_image()
    assert np.array_equal(seams, V.seams_model(img, vm, 12))
    assert np.array_equal(seams[-1], img[-1]) and np.array_equal(seams[:, -1], img[:, -1])
    with ctx.resizer(img, 1, 8) as r1:
        s1 = r1.seams_image()
        v1 = r1.vmap()
        assert np.array_equal(s1, V.seams_model(img, v1, 1))
        inner = v1[:-1, :-1] == 1
        assert inner.any() and (s1[:-1, :-1][inner] == (0, 255, 0)).all()


# ---- edges and errors --------------------------------------------------------
def test_resizer_edges(ctx):
    img = load_input("natural_grey_200x120.npy")
    with ctx.resizer(img, 0, 8) as r:
        assert r.depth == 0 and not r.vmap().any()
        assert np.array_equal(r.render(0), img)
        assert np.array_equal(r.seams_image(), img)
    view = np.ascontiguousarray(img[:40, 3:8])
    with ctx.resizer(view, 4, 8, 0.3, 0.7) as r:
        one = r.render(-4)
        assert one.shape == (40, 1)
        assert np.array_equal(one, ctx.carve(view, 4, 8, 0.3, 0.7)[0])
        assert (np.sort(r.vmap(), axis=1) == np.arange(5)).all()
        assert np.array_equal(r.render(4), V.render_model(view, r.vmap(), 4))


def test_resizer_errors_leave_it_usable(ctx, natural):
    img, r, vm = natural
    L = dctenergy.lib()
    E = dctenergy.DCTE_EINVAL
    out = np.empty(img.size * 2, np.uint8)
    assert L.dcte_resizer_render(r._h, 13, out.ctypes.data) == E
    assert L.dcte_resizer_render(r._h, -13, out.ctypes.data) == E
    assert L.dcte_resizer_render(r._h, 1, None) == E
    with pytest.raises(dctenergy.DcteError):
        r.render(-13)
    assert np.array_equal(r.render(3), V.render_model(img, vm, 3))
    h, w = img.shape[:2]
    h_ = ctypes.c_void_p()

    def create(bpp, n, depth, transposed=0):
        return L.dcte_resizer_create(ctx._h, img.ctypes.data, w, h, bpp, w * 3, n, 0.5, 0.5, 0,
                                     depth, transposed, None, ctypes.byref(h_))
    assert create(3, 8, w) == E and not h_.value          # depth >= W
    assert create(3, 8, h, 1) == E                        # transposed: W is h
    assert create(3, 8, -1) == E
    assert create(2, 8, 1) == E                           # bpp
    assert create(4, 8, 1) == E                           # RGBA is preview-only
    assert create(3, 6, 1) == E                           # N
    with pytest.raises(dctenergy.DcteError):
        ctx.resizer(img, w, 8)
    assert np.array_equal(r.render(-2), ctx.carve(img, 2, 8)[0])


# ---- the device render entry on its own ----------------------------------------
def _edge_vmap(h, w):
    """depth 2: the seams sit at x = 0 and x = w - 1, swapped in alternating rows."""
    vm = np.zeros((h, w), np.int32)
    vm[0::2, 0], vm[0::2, w - 1] = 1, 2
    vm[1::2, 0], vm[1::2, w - 1] = 2, 1
    return vm


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_render_device_edges_and_strides(ctx, bpp):
    torch = _torch()
    h, w = 6, 130                                     # no multiple of the wave's 64 pixels
    rng = np.random.default_rng(50 + bpp)
    img = rng.integers(0, 256, (h, w) + ((bpp,) if bpp > 1 else ()), dtype=np.uint8)
    vm = _edge_vmap(h, w)
    d_img, d_vm = torch.from_numpy(img).cuda(), torch.from_numpy(vm).cuda()
    for delta in (2, 1, 0, -1, -2):
        buf = torch.full((h, w + 9) + img.shape[2:], 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[:, :w + delta]
        assert out.stride(0) > (w + delta) * bpp
        ctx.vmap_render_tensor(d_img, d_vm, 2, delta, out)
        got = buf.cpu().numpy()
        assert np.array_equal(got[:, :w + delta], V.render_model(img, vm, delta)), delta
        assert (got[:, w + delta:] == 0xA5).all()
    # x = 0: the inserted pixel's left neighbour is the pixel itself; x = w - 1: the
    # insert is the mean of the last two pixels
    big = V.render_model(img, vm, 1)
    assert np.array_equal(big[0, 0], img[0, 0]) and np.array_equal(big[0, 1], img[0, 0])
    mean = ((img[1, w - 2].astype(int) + img[1, w - 1]) // 2).astype(np.uint8)
    assert np.array_equal(big[1, w - 1], mean) and np.array_equal(big[1, w], img[1, w - 1])


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_render_device_many_passes(ctx, bpp):
    """Rows of several 64-pixel passes and more than one trip of the kernel's
    loop: the running output offset is carried across them."""
    torch = _torch()
    h, w, depth = 9, 1000, 200
    rng = np.random.default_rng(80 + bpp)
    img = rng.integers(0, 256, (h, w) + ((bpp,) if bpp > 1 else ()), dtype=np.uint8)
    vm = V.vmap_model(_synthetic_cols(h, w, depth, 81), w)
    d_img, d_vm = torch.from_numpy(img).cuda(), torch.from_numpy(vm).cuda()
    for delta in (depth, 77, 0, -77, -depth):
        out = torch.empty((h, w + delta) + img.shape[2:], dtype=torch.uint8, device="cuda")
        ctx.vmap_render_tensor(d_img, d_vm, depth, delta, out)
        assert np.array_equal(out.cpu().numpy(), V.render_model(img, vm, delta)), delta


def test_render_device_rgba_unaligned(ctx):
    """RGBA frames that are not 4-byte aligned take the byte path."""
    torch = _torch()
    h, w = 5, 70
    img = np.random.default_rng(60).integers(0, 256, (h, w, 4), dtype=np.uint8)
    vm = _edge_vmap(h, w)
    flat = torch.zeros(h * w * 4 + 1, dtype=torch.uint8, device="cuda")
    d_img = flat[1:].view(h, w, 4)
    d_img.copy_(torch.from_numpy(img))
    oflat = torch.zeros(h * (w + 2) * 4 + 3, dtype=torch.uint8, device="cuda")
    out = oflat[3:].view(h, w + 2, 4)
    assert d_img.data_ptr() % 4 == 1 and out.data_ptr() % 4 == 3
    ctx.vmap_render_tensor(d_img, torch.from_numpy(vm).cuda(), 2, 2, out)
    assert np.array_equal(out.cpu().numpy(), V.render_model(img, vm, 2))


def test_device_entries_refuse_bad_arguments(ctx):
    torch = _torch()
    L = dctenergy.lib()
    E = dctenergy.DCTE_EINVAL
    vp = ctypes.c_void_p
    h, w = 4, 16
    px = torch.zeros((h, w + 4, 3), dtype=torch.uint8, device="cuda")
    vm = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    out = torch.zeros((h, w + 4, 3), dtype=torch.uint8, device="cuda")
    p, v, o = vp(px.data_ptr()), vp(vm.data_ptr()), vp(out.data_ptr())
    rs = (w + 4) * 3

    def render(src, dst, bpp=3, depth=2, delta=1, ors=rs):
        return L.dcte_vmap_render_device(ctx._h, 0, src, rs, w, h, bpp, v, w, depth, delta, dst, ors,
                                         None)
    assert render(p, o) == dctenergy.DCTE_OK
    assert render(p, p) == E                              # overlapping frames
    assert render(p, vp(px.data_ptr() + 3 * w)) == E      # interleaved rows overlap too
    assert render(p, o, bpp=2) == E
    assert render(p, o, delta=3) == E and render(p, o, delta=-3) == E
    assert render(p, o, depth=w) == E
    assert render(p, o, ors=w * 3) == E                   # out rows too short for w + 1
    assert L.dcte_vmap_seams_u8_device(ctx._h, 0, p, rs, w, h, 3, v, w, 2, p, rs, None) == E
    assert L.dcte_vmap_seams_u8_device(ctx._h, 0, p, rs, w, h, 5, v, w, 2, o, rs, None) == E
    torch.cuda.synchronize()


def test_seams_device_strided(ctx):
    torch = _torch()
    h, w = 7, 131
    img = np.random.default_rng(70).integers(0, 256, (h, w, 3), dtype=np.uint8)
    vm = _edge_vmap(h, w)
    vm[h - 1, 5] = 1                                  # last row: never painted
    buf = torch.full((h, w + 3, 3), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.vmap_seams_tensor(torch.from_numpy(img).cuda(), torch.from_numpy(vm).cuda(), 2,
                          buf[:, :w])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :w], V.seams_model(img, vm, 2))
    assert (got[:, w:] == 0xA5).all()
