"""GPU: the stream contract of the dcte_*_device entry points (include/dctenergy.h).

Every other GPU test passes the legacy null stream, which serialises with all
blocking streams, and reads back with a synchronising copy.  Here the calls go
to non-blocking side streams (torch.cuda.Stream()) behind a device-side delay:

  1. ordering, one case per entry point: delay | true input in | the call |
     event | decoy back, with no host sync -- the event must still be pending
     when the call returns (no wait inside the library), and the output must be
     the true input's, not the decoy's (read too early) or the sentinel (never);
  2. about 40 unsynchronised calls on one side stream whose scratch grows and
     shrinks in mid-sequence;
  3. calls overlapping on different streams of one context: the row-band
     pattern, a mixed load on four streams, min/max on two, and dcte_destroy
     with work in flight.

Each result is bit-equal to the same call made alone on the null stream and
synchronised; section 1 also checks it against the oracle at the suite's bar
(golden_util.within_tol; bit-equal for seams, vmap, render, u8 and windows).
A decoy is always another VALID input, so a premature read gives a wrong
answer, never an out-of-range access.
"""
import ctypes
import functools

import numpy as np
import pytest

import dctenergy
import oracle_py as O
import vmap_util as V
from golden_util import within_tol
from seam_util import carve, random_seams
from stream_util import (E, FIX_DIRECT, H, T, W, Case, Delay, run_alone, run_ordered, same,
                         strip_counts, tie_frame)

pytestmark = pytest.mark.gpu

LQR, PREVIEW = dctenergy.DCTE_LQR, dctenergy.DCTE_PREVIEW
OPTS = (dctenergy.DCTE_OPT_EXACT, dctenergy.DCTE_OPT_DP_BANDWISE)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "the stream tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def delay(torch):
    d = Delay(torch)
    print(f"delay: {d.kind}({d.arg}) calibrated to {d.ms:.1f} ms; steps {d.trace}")
    assert d.ms >= 20.0, (d.ms, d.trace)
    return d


@pytest.fixture(scope="module")
def sctx():
    """A context of this module's own: its options are switched between calls."""
    c = dctenergy.Context(ngpus=1)
    yield c
    c.close()


# ---------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def _frame(ch, seed, h=H, w=W):
    f = tie_frame(ch, seed, h, w)
    f.setflags(write=False)
    return f


def _decoy_frame(ch, seed, h=H, w=W):
    """Another valid frame (not 255 - frame: the negative has the same AC
    magnitudes, so its map would be nearly the true one)."""
    return np.ascontiguousarray(_frame(ch, seed + 50, h, w)[::-1])


def _oracle_of(img, n, e, t, sem):
    return (O.energy_map if sem == LQR else O.preview_map)(img, n, e, t, nthreads=4)


@functools.lru_cache(maxsize=None)
def _oracle(ch, seed, n, sem, e=E, t=T):
    return _oracle_of(_frame(ch, seed), n, e, t, sem)


def _assert_tol(got, ref, what):
    ok = within_tol(got, ref)
    assert ok.all(), f"{what}: {int((~ok).sum())} pixels off tolerance"


# ------------------------------------------------------------------- builders
# Each returns (Case, check): check(outputs) compares them with the oracle.
def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()     # a writable copy


def _io(torch, true, decoy):
    t = _dev(torch, true)
    return (torch.empty_like(t), t, _dev(torch, decoy) if decoy is not None else t)


def map_case(torch, n, sem, ch, seed=0, e=E, t=T, h=H, w=W, rows=None, exact=False):
    img = _frame(ch, seed, h, w)
    px = _io(torch, img, _decoy_frame(ch, seed, h, w))
    out = torch.empty((h, w), dtype=torch.float32, device="cuda")
    buf = px[0]
    if rows is None:
        def call(ctx, st):
            ctx.energy_map_device(buf.data_ptr(), buf.stride(0), w, h, ch, 0, h, 0, h, n, e, t,
                                  out.data_ptr(), out.stride(0), st, semantics=sem)
    else:
        a0, a1, b0, b1 = rows

        def call(ctx, st):
            ctx.energy_map_device2(buf.data_ptr(), buf.stride(0), w, h, ch, 0, h, a0, a1, b0, b1,
                                   n, e, t, out[a0:].data_ptr(), out.stride(0), st, semantics=sem)

    def check(res):
        ref = _oracle_of(img, n, e, t, sem) if (h, w, e, t) != (H, W, E, T) else \
            _oracle(ch, seed, n, sem)
        got = res[0]
        keep = np.ones(h, bool)
        if rows is not None:
            keep[:] = False
            keep[a0:a1] = keep[b0:b1] = True
        assert (got[~keep] == -1).all(), "rows outside the ranges were written"
        if exact:
            assert same(got[keep], ref[keep]), "exact mode: not the oracle's bits"
        else:
            _assert_tol(got[keep], ref[keep], f"map n={n} sem={sem} ch={ch}")
    return Case(f"map n={n} sem={sem} ch={ch} rows={rows}", [px], [(out, -1.0)], call), check


def carve_case(torch, ctx, n, sem, ch, inplace, seed=0, e=E, t=T, h=H, w=W):
    img, dimg = _frame(ch, seed, h, w), _decoy_frame(ch, seed, h, w)
    seams = random_seams(h, w, seed + 3, 2)
    maps = []
    for f in (img, dimg):                         # the maps the call updates: the library's own
        m = torch.empty((h, w), dtype=torch.float32, device="cuda")
        ctx.energy_map_tensor(_dev(torch, f), m, n, e, t, semantics=sem)
        torch.cuda.synchronize()
        maps.append(m.cpu().numpy())
    px, sm, mp = _io(torch, img, dimg), _io(torch, seams[0], seams[1]), _io(torch, maps[0], maps[1])
    px_out = torch.empty((h, w - 1) + img.shape[2:], dtype=torch.uint8, device="cuda")
    map_out = torch.empty((h, w - 1), dtype=torch.float32, device="cuda")

    def call(c, st):
        if inplace:                               # results stay in the input buffers: copy them out
            c.seam_carve_tensor(px[0], sm[0], mp[0], px[0][:, :w - 1], mp[0][:, :w - 1], n, e, t,
                                stream=st, semantics=sem)
            px_out.copy_(px[0][:, :w - 1], non_blocking=True)
            map_out.copy_(mp[0][:, :w - 1], non_blocking=True)
        else:
            c.seam_carve_tensor(px[0], sm[0], mp[0], px_out, map_out, n, e, t, stream=st,
                                semantics=sem)

    def check(res):
        host = carve(img, seams[0])
        assert np.array_equal(res[0], host), "carved frame"
        _assert_tol(res[1], _oracle_of(host, n, e, t, sem), f"carved map n={n}")
    return Case(f"carve n={n} sem={sem} ch={ch} inplace={inplace}", [px, sm, mp],
                [(px_out, 0xA5), (map_out, -1.0)], call), check


def points_case(torch, n, sem, ch, count=40000, seed=0, e=E, t=T, h=H, w=W):
    """count / 256 workgroups of dcte_points: 40000 points are 157."""
    img = _frame(ch, seed, h, w)
    rng = np.random.default_rng(seed + 9)
    xy = [np.stack([rng.integers(0, w, count), rng.integers(0, h, count)], 1).astype(np.int32)
          for _ in range(2)]
    px, pts = _io(torch, img, _decoy_frame(ch, seed, h, w)), _io(torch, xy[0], xy[1])
    out = torch.empty(count, dtype=torch.float32, device="cuda")

    def call(ctx, st):
        ctx.energy_points_tensor(px[0], pts[0], out, n, e, t, stream=st, semantics=sem)

    def check(res):
        ref = _oracle_of(img, n, e, t, sem) if (h, w, e, t) != (H, W, E, T) else \
            _oracle(ch, seed, n, sem)
        _assert_tol(res[0], ref[xy[0][:, 1], xy[0][:, 0]], f"points n={n}")
    return Case(f"points n={n} sem={sem} ch={ch} count={count}", [px, pts], [(out, -1.0)], call), check


def windows_case(torch, n, count=1500, seed=0, e=E, t=T):
    rng = np.random.default_rng(seed + 20 + n)
    wins = [np.concatenate([rng.random((count // 2, n, n)),
                            (rng.random((count - count // 2, n, n)) < 0.05) * (254 / 255) + 1 / 255])
            for _ in range(2)]
    win = _io(torch, wins[0], wins[1])
    out = torch.empty(count, dtype=torch.float32, device="cuda")

    def call(ctx, st):
        ctx._check(dctenergy.lib().dcte_energy_windows_device(
            ctx._h, 0, win[0].data_ptr(), count, n, e, t, out.data_ptr(), ctypes.c_void_p(st)))

    def check(res):
        ref = np.array([O.window_energy(x, e, t) for x in wins[0]], np.float32)
        assert same(res[0], ref), f"windows n={n}"
    return Case(f"windows n={n} count={count}", [win], [(out, -1.0)], call), check


def _energy(h, w, seed):
    """A cheap valley that wanders across tile borders, on noise."""
    rng = np.random.default_rng(seed)
    x = np.arange(w)[None, :]
    c = w / 2 + (w / 3) * np.sin(np.arange(h)[:, None] / 37.0 + seed)
    return (np.abs(x - c) / w + 0.01 * rng.random((h, w))).astype(np.float32)


def seam_find_case(torch, h=100, w=300, seed=0):
    maps = [_energy(h, w, seed), _energy(h, w, seed + 1)]
    mp = _io(torch, maps[0], maps[1])
    seam = torch.empty(h, dtype=torch.int32, device="cuda")

    def call(ctx, st):
        ctx.seam_find_tensor(mp[0], seam, stream=st)

    def check(res):
        assert np.array_equal(res[0], O.seam_find(maps[0])), "seam"
    return Case(f"seam_find {h}x{w}", [mp], [(seam, -7)], call), check


def norm_case(torch, mode, ch, count=(1 << 20) + 37, seed=0):
    rng = np.random.default_rng(seed + 30)
    e0 = rng.random(count, dtype=np.float32) * np.float32(8) - np.float32(3)
    e1 = rng.random(count, dtype=np.float32) * np.float32(0.5) + np.float32(7)
    en = _io(torch, e0, e1)
    mm = torch.empty(2, dtype=torch.float32, device="cuda")
    u8 = torch.empty(count * ch, dtype=torch.uint8, device="cuda")

    def call(ctx, st):
        ctx.minmax_device(en[0].data_ptr(), count, mm.data_ptr(), st)
        ctx.normalize_u8_device(en[0].data_ptr(), count, mm.data_ptr(), u8.data_ptr(), mode, ch, st)

    def check(res):
        assert res[0][0] == e0.min() and res[0][1] == e0.max(), res[0]
        restate = O.normalize_lqr if mode == dctenergy.DCTE_NORM_LQR else O.normalize_preview
        assert np.array_equal(res[1], np.repeat(restate(e0, 1), ch)), "u8 layer"
    return Case(f"minmax+u8 mode={mode} ch={ch}", [en], [(mm, -1.0), (u8, 0xA5)], call), check


def _cols(h, w, depth, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, w - k, h) for k in range(depth)]).astype(np.int32)


VH, VW, VDEPTH = 40, 300, 30


def vmap_case(torch, seed=0):
    cols = [_cols(VH, VW, VDEPTH, seed + 40), _cols(VH, VW, VDEPTH, seed + 41)]
    cl = _io(torch, cols[0], cols[1])
    vm = torch.empty((VH, VW), dtype=torch.int32, device="cuda")

    def call(ctx, st):
        ctx.vmap_tensor(cl[0], vm, stream=st)

    def check(res):
        assert np.array_equal(res[0], V.vmap_model(cols[0], VW)), "vmap"
    return Case("vmap", [cl], [(vm, -7)], call), check


def render_case(torch, kind, bpp, delta=0, seed=0):
    """kind: "render" (dcte_vmap_render_device) or "seams" (dcte_vmap_seams_u8_device)."""
    rng = np.random.default_rng(seed + 50 + bpp)
    imgs = [rng.integers(0, 256, (VH, VW) + ((bpp,) if bpp > 1 else ()), dtype=np.uint8)
            for _ in range(2)]
    vms = [V.vmap_model(_cols(VH, VW, VDEPTH, seed + 42 + k), VW) for k in range(2)]
    px, vm = _io(torch, imgs[0], imgs[1]), _io(torch, vms[0], vms[1])
    out = torch.empty((VH, VW + delta) + imgs[0].shape[2:], dtype=torch.uint8, device="cuda")

    def call(ctx, st):
        if kind == "render":
            ctx.vmap_render_tensor(px[0], vm[0], VDEPTH, delta, out, stream=st)
        else:
            ctx.vmap_seams_tensor(px[0], vm[0], VDEPTH, out, stream=st)

    def check(res):
        want = V.render_model(imgs[0], vms[0], delta) if kind == "render" else \
            V.seams_model(imgs[0], vms[0], VDEPTH)
        assert np.array_equal(res[0], want), kind
    return Case(f"{kind} bpp={bpp} delta={delta}", [px, vm], [(out, 0xA5)], call), check


# ------------------------------------------------- 1. ordering, per entry point
def _ordered(torch, ctx, delay, built, opts=()):
    case, check = built
    for o, v in opts:
        ctx.set_option(o, v)
    try:
        alone = run_alone(torch, ctx, case)
        from_decoy = run_alone(torch, ctx, case, "decoy")
        got, host_s = run_ordered(torch, ctx, case, delay)
    finally:
        for o, _ in opts:
            ctx.set_option(o, 0)
    print(f"{case.name}: host side of the call {host_s * 1e6:.0f} us, delay {delay.ms:.1f} ms")
    assert delay.ms * 1e-3 >= 10 * host_s, (delay.ms, host_s)
    # a premature read would show: the decoy gives another result
    assert not all(same(a, d) for a, d in zip(alone, from_decoy)), "the decoy is no decoy"
    for k, (g, a) in enumerate(zip(got, alone)):
        assert same(g, a), f"{case.name}: output {k} differs from the call made alone " \
                           f"({'the decoy result' if same(g, from_decoy[k]) else 'neither'})"
    check(got)


def test_frames_hold_sparse_and_dense_strips():
    """The frames of this module at N = 8: strips of at most kFixDirect flagged
    pixels next to strips of more (the host emulation's refinement mask)."""
    for ch, sem in ((1, LQR), (3, LQR), (4, PREVIEW)):
        c = strip_counts(_frame(ch, 0), 8, sem)
        assert ((c > 0) & (c <= FIX_DIRECT)).sum() >= 4 and (c > FIX_DIRECT).sum() >= 4, (ch, c)
        assert (c.sum(0) > 0).sum() >= 3 and c.shape[0] > 1      # several strips, tile rows


@pytest.mark.parametrize("n", [2, 4, 8, 16])
@pytest.mark.parametrize("sem,ch", [(LQR, 1), (LQR, 3), (PREVIEW, 4)],
                         ids=["lqr-grey", "lqr-rgb", "preview-rgba"])
def test_map_is_ordered_on_its_stream(torch, sctx, delay, n, sem, ch):
    _ordered(torch, sctx, delay, map_case(torch, n, sem, ch))


@pytest.mark.parametrize("sem,ch", [(LQR, 3), (PREVIEW, 4)], ids=["lqr-rgb", "preview-rgba"])
def test_exact_map_is_ordered_on_its_stream(torch, sctx, delay, sem, ch):
    _ordered(torch, sctx, delay, map_case(torch, 8, sem, ch, exact=True),
             [(dctenergy.DCTE_OPT_EXACT, 1)])


@pytest.mark.parametrize("n,sem,ch", [(8, LQR, 3), (16, LQR, 1), (8, PREVIEW, 4)])
def test_map2_is_ordered_on_its_stream(torch, sctx, delay, n, sem, ch):
    _ordered(torch, sctx, delay, map_case(torch, n, sem, ch, rows=(40, 47, 200, 263)))


@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("n,sem,ch", [(8, LQR, 3), (16, PREVIEW, 4), (4, LQR, 1)])
def test_seam_carve_is_ordered_on_its_stream(torch, sctx, delay, n, sem, ch, inplace):
    _ordered(torch, sctx, delay, carve_case(torch, sctx, n, sem, ch, inplace))


@pytest.mark.parametrize("n,sem,ch", [(8, LQR, 3), (16, PREVIEW, 4), (4, LQR, 1)])
def test_points_are_ordered_on_their_stream(torch, sctx, delay, n, sem, ch):
    _ordered(torch, sctx, delay, points_case(torch, n, sem, ch))


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_windows_are_ordered_on_their_stream(torch, sctx, delay, n):
    _ordered(torch, sctx, delay, windows_case(torch, n))


@pytest.mark.parametrize("bandwise", [0, 1], ids=["resident", "bandwise"])
def test_seam_find_is_ordered_on_its_stream(torch, sctx, delay, bandwise):
    _ordered(torch, sctx, delay, seam_find_case(torch),
             [(dctenergy.DCTE_OPT_DP_BANDWISE, bandwise)])


@pytest.mark.parametrize("mode,ch", [(dctenergy.DCTE_NORM_LQR, 1), (dctenergy.DCTE_NORM_PREVIEW, 3)])
def test_minmax_then_u8_are_ordered_on_their_stream(torch, sctx, delay, mode, ch):
    _ordered(torch, sctx, delay, norm_case(torch, mode, ch))


def test_vmap_is_ordered_on_its_stream(torch, sctx, delay):
    _ordered(torch, sctx, delay, vmap_case(torch))


@pytest.mark.parametrize("kind,bpp,delta", [("render", 3, 17), ("render", 4, -17), ("render", 1, 30),
                                            ("seams", 3, 0), ("seams", 1, 0)])
def test_vmap_render_and_seams_are_ordered_on_their_stream(torch, sctx, delay, kind, bpp, delta):
    _ordered(torch, sctx, delay, render_case(torch, kind, bpp, delta))


# ------------------------------- 2. unsynchronised sequences on one side stream
def _sequence(torch, ctx):
    """-> [(Case, {option: value})]: a fixed, seeded mix.  Shapes shrink and
    then grow past the first, so the fix lists, tile arrays and DP buffers are
    re-allocated in mid-sequence and pw changes between seam searches; e == t
    frames (no refinement launch) stand next to frames that refine."""
    rng = np.random.default_rng(2024)
    shapes = [(150, 200), (60, 90), (33, 70), (300, 400), (120, 333)]
    seam_shapes = [(100, 300), (40, 70), (120, 600), (64, 129)]
    fmt = [(LQR, 1), (LQR, 3), (PREVIEW, 4), (PREVIEW, 3), (PREVIEW, 1)]
    kinds = ["map", "map2", "seam_find", "carve", "points", "windows"]
    seq = []
    for k in range(40):
        kind = kinds[k % 6] if k < 12 else kinds[int(rng.integers(0, 6))]
        h, w = shapes[(k // 7) % len(shapes)]                 # a new shape every 7 calls
        n = (2, 4, 8, 16)[int(rng.integers(0, 4))]
        sem, ch = fmt[int(rng.integers(0, len(fmt)))]
        e, t = ((0.3, 0.7), (0.5, 0.5), (0.85, 0.15))[int(rng.integers(0, 3))]
        opts = {dctenergy.DCTE_OPT_EXACT: int(rng.integers(0, 2)),
                dctenergy.DCTE_OPT_DP_BANDWISE: int(rng.integers(0, 2))}
        if kind == "map":
            case = map_case(torch, n, sem, ch, k, e, t, h, w)[0]
        elif kind == "map2":
            a1 = h // 3
            case = map_case(torch, n, sem, ch, k, e, t, h, w, rows=(2, a1, a1 + 5, h - 1))[0]
        elif kind == "seam_find":
            sh = seam_shapes[(k // 5) % len(seam_shapes)]
            case = seam_find_case(torch, sh[0], sh[1], k)[0]
        elif kind == "carve":
            case = carve_case(torch, ctx, n, sem, ch, bool(k & 1), k, e, t, h, w)[0]
        elif kind == "points":
            case = points_case(torch, n, sem, ch, (500, 9000, 70000)[k % 3], k, e, t, h, w)[0]
        else:
            case = windows_case(torch, n, 700, k, e, t)[0]
        seq.append((case, opts))
    return seq


def _set(ctx, opts):
    for o, v in opts.items():
        ctx.set_option(o, v)


def test_unsynchronised_sequence_on_one_stream(torch, delay):
    """40 calls behind one delay, no host sync until the end, scratch growing
    in mid-sequence (which may wait: the only thing not asserted here is the
    pending event).  Every output equals the same call alone in a fresh context."""
    with dctenergy.Context(ngpus=1) as build_ctx:
        seq = _sequence(torch, build_ctx)
    assert len({c.name.split()[0] for c, _ in seq}) == 5          # map(2), seam_find, carve, ...
    want = []
    for case, opts in seq:
        with dctenergy.Context(ngpus=1) as fresh:
            _set(fresh, opts)
            want.append(run_alone(torch, fresh, case))
    for case, _ in seq:
        case.fill("true")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with dctenergy.Context(ngpus=1) as c:
        with torch.cuda.stream(side):
            delay.enqueue()
            for case, opts in seq:
                _set(c, opts)
                case.call(c, side.cuda_stream)
        side.synchronize()
    for k, ((case, opts), ref) in enumerate(zip(seq, want)):
        for j, (g, a) in enumerate(zip(case.results(), ref)):
            assert same(g, a), f"call {k} ({case.name}, {opts}): output {j} differs from the call alone"


# --------------------------- 3. calls overlapping on different streams of a context
def _gate(torch, delay, streams):
    """One delay, then every stream released at the same moment: the work
    enqueued behind the gate really overlaps."""
    g = torch.cuda.Stream()
    ev = torch.cuda.Event()
    with torch.cuda.stream(g):
        delay.enqueue()
        ev.record(g)
    for s in streams:
        s.wait_event(ev)
    return g


@pytest.mark.parametrize("n", [8, 16])
def test_band_pattern_on_two_streams(torch, sctx, delay, n):
    """A middle rank's band (dist.make_band): the interior rows on stream A, both
    edge ranges in one dcte_energy_map_device2 call on stream B, back to back
    with no sync, several bands in a row -- bit-equal to those rows of the full map."""
    from dctenergy import dist as D
    img = _frame(3, 0)
    band = D.make_band(H, 1, 3, n)
    (e0, e1), (f0, f1) = band.edges()
    i0, i1 = band.interior()
    frame = _dev(torch, img)
    full = torch.empty((H, W), dtype=torch.float32, device="cuda")
    sctx.energy_map_tensor(frame, full, n, E, T)
    torch.cuda.synchronize()
    buf = frame[band.row0:band.row0 + band.rows].clone()      # only band + halos are readable
    rounds = 8
    outs = torch.full((rounds, band.own, W), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    _gate(torch, delay, (a, b))
    for r in range(rounds):
        out = outs[r]
        sctx.energy_map_device(buf.data_ptr(), buf.stride(0), W, H, 3, band.row0, band.rows, i0, i1,
                               n, E, T, out[i0 - band.Y0:].data_ptr(), out.stride(0), a.cuda_stream)
        sctx.energy_map_device2(buf.data_ptr(), buf.stride(0), W, H, 3, band.row0, band.rows, e0, e1,
                                f0, f1, n, E, T, out.data_ptr(), out.stride(0), b.cuda_stream)
    a.synchronize()
    b.synchronize()
    want = full[band.Y0:band.Y1].cpu().numpy()
    _assert_tol(want, _oracle(3, 0, n, LQR)[band.Y0:band.Y1], "the full map itself")
    for r in range(rounds):
        assert same(outs[r].cpu().numpy(), want), f"band {r} differs from the full map's rows"


def _carve_chain(torch, ctx, px, emap, rounds, n, stream, seams, frames, maps):
    """seam find, then carve in place, `rounds` times; every round's seam,
    frame and map are copied out (on the current stream)."""
    h, w = emap.shape
    for r in range(rounds):
        cur = w - r
        ctx.seam_find_tensor(emap[:, :cur], seams[r], stream=stream)
        ctx.seam_carve_tensor(px[:, :cur], seams[r], emap[:, :cur], px[:, :cur - 1],
                              emap[:, :cur - 1], n, E, T, stream=stream)
        frames[r].copy_(px, non_blocking=True)
        maps[r].copy_(emap, non_blocking=True)


def test_mixed_load_on_four_streams(torch, sctx, delay):
    """20 rounds enqueued round-robin with no sync: A maps F1 at N = 8, B maps
    F2 at N = 16, C finds and carves seams in place (w <= 512: its DP tiles
    are always resident), D runs windows and points.  Every round's output is
    bit-equal to the same call made alone."""
    rounds = 20
    A = map_case(torch, 8, LQR, 3, seed=1)[0]
    B = map_case(torch, 16, LQR, 1, seed=2)[0]
    Dw = windows_case(torch, 8, 1500, seed=3)[0]
    Dp = points_case(torch, 16, PREVIEW, 4, 40000, seed=4)[0]
    ch, cw = 100, 300
    f3 = _dev(torch, _frame(3, 5, ch, cw))
    m3 = torch.empty((ch, cw), dtype=torch.float32, device="cuda")
    sctx.energy_map_tensor(f3, m3, 8, E, T)
    torch.cuda.synchronize()

    def chain_bufs():
        return (torch.full((rounds, ch), -7, dtype=torch.int32, device="cuda"),
                torch.zeros((rounds, ch, cw, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros((rounds, ch, cw), dtype=torch.float32, device="cuda"))

    # alone: each call on the null stream of a fresh context, synchronised
    with dctenergy.Context(ngpus=1) as fresh:
        alone = {k: run_alone(torch, fresh, c) for k, c in (("A", A), ("B", B), ("Dw", Dw), ("Dp", Dp))}
        want_c = chain_bufs()
        _carve_chain(torch, fresh, f3.clone(), m3.clone(), rounds, 8, 0, *want_c)
        torch.cuda.synchronize()
    for c in (A, B, Dw, Dp):
        c.fill("true")
    outs = {k: [torch.full_like(c.outputs[0][0], -1.0) for _ in range(rounds)]
            for k, c in (("A", A), ("B", B), ("Dw", Dw), ("Dp", Dp))}
    got_c = chain_bufs()
    px, emap = f3.clone(), m3.clone()
    torch.cuda.synchronize()
    st = [torch.cuda.Stream() for _ in range(4)]
    _gate(torch, delay, st)
    for r in range(rounds):
        for k, c, s in (("A", A, st[0]), ("B", B, st[1])):
            with torch.cuda.stream(s):
                c.call(sctx, s.cuda_stream)
                outs[k][r].copy_(c.outputs[0][0], non_blocking=True)
        with torch.cuda.stream(st[2]):
            _carve_chain(torch, sctx, px[:, :cw - r], emap[:, :cw - r], 1, 8, st[2].cuda_stream,
                         got_c[0][r:], [got_c[1][r][:, :cw - r]], [got_c[2][r][:, :cw - r]])
        with torch.cuda.stream(st[3]):
            for k, c in (("Dw", Dw), ("Dp", Dp)):
                c.call(sctx, st[3].cuda_stream)
                outs[k][r].copy_(c.outputs[0][0], non_blocking=True)
    for s in st:
        s.synchronize()
    for k in outs:
        for r in range(rounds):
            assert same(outs[k][r].cpu().numpy(), alone[k][0]), f"stream {k}, round {r}"
    for r in range(rounds):
        assert torch.equal(got_c[0][r], want_c[0][r]), f"seam of round {r}"
        keep = cw - r - 1
        assert torch.equal(got_c[1][r][:, :keep], want_c[1][r][:, :keep]), f"frame after round {r}"
        assert same(got_c[2][r][:, :keep].cpu().numpy(), want_c[2][r][:, :keep].cpu().numpy()), \
            f"map after round {r}"
    assert (want_c[0].cpu().numpy() >= 0).all()               # every search found its seam


def test_minmax_on_two_streams(torch, sctx, delay):
    """Two streams, each reducing its own array of 3 million floats, 50
    interleaved rounds: every {min, max} equals numpy's (key scratch is per
    stream; one shared pair of keys mixes the two ranges)."""
    count, rounds = 3_000_001, 50
    rng = np.random.default_rng(7)
    host = [rng.random(count, dtype=np.float32), rng.random(count, dtype=np.float32) * 9 + 10]
    arr = [_dev(torch, x) for x in host]
    mm = [torch.full((rounds, 2), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    st = [torch.cuda.Stream(), torch.cuda.Stream()]
    _gate(torch, delay, st)
    for r in range(rounds):
        for k in range(2):
            sctx.minmax_device(arr[k].data_ptr(), count, mm[k][r].data_ptr(), st[k].cuda_stream)
    for s in st:
        s.synchronize()
    for k in range(2):
        got = mm[k].cpu().numpy()
        want = np.array([host[k].min(), host[k].max()], np.float32)
        assert (got == want).all(), (k, want, got[(got != want).any(1)][:5])


def test_destroy_with_work_in_flight(torch, delay):
    """A delayed map on a side stream, the context closed at once: dcte_destroy
    waits for the stream before it frees the scratch; the output is complete."""
    case, check = map_case(torch, 8, LQR, 3)
    with dctenergy.Context(ngpus=1) as fresh:
        alone = run_alone(torch, fresh, case)
    case.fill("true")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    c = dctenergy.Context(ngpus=1)
    with torch.cuda.stream(side):
        delay.enqueue()
        case.call(c, side.cuda_stream)
    c.close()
    side.synchronize()
    got = case.results()
    assert same(got[0], alone[0])
    check(got)
