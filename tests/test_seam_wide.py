"""GPU: dcte_seam_shift past its first pass and off its aligned bases.

The shift kernel moves a row in passes of 16 * 256 * DCTE_SHIFT_VEC frame
bytes and 4 * 256 * DCTE_SHIFT_VEC map floats (8192 bytes / 2048 floats at
the default, half / twice that at the other knob values), splits each row
into an unaligned head, 16-byte destination blocks and a tail, and reads its
sources at any byte offset from the dword below the frame's base.  The
frames of test_seam.py are at most 600 bytes wide and start where the
allocator put them: one pass, iofs = 0.  Here every row takes several frame
and map passes at DCTE_SHIFT_VEC 1, 2 and 4, and the frames and maps are
also sub-rectangles of larger buffers -- frame column offset 1..3, a row
stride that is odd in bytes (bpp 1, 3; 4 mod 8 for bpp 4, whose stride
cannot be odd), so every row has its own source and destination alignment;
map column offset 1..3 in rows of w + 7 floats.

Bar, the one of test_seam.py: after every step the frame equals numpy's
carve and the map equals, bit for bit, the full map of the carved frame;
after the last step the map is within RTOL / ATOL of the oracle.  On top of
it, bitwise, nothing but the contract's bytes is written: everything around
the views holds sentinels before a step and after it (see _wide_run).
"""
import os

import numpy as np
import pytest

import dctenergy
import oracle_py as O
from golden_util import within_tol
from seam_util import carve, random_seams, seam_span

pytestmark = pytest.mark.gpu

NT = max(1, min(16, len(os.sched_getaffinity(0))))
E, T = 0.15, 0.85
SENT_B = 0xA5                       # bytes around the frame views
SENT_F = 0x7FC0A5A5                 # bit pattern (a NaN) around the map views, compared as int32

# (bpp, semantics, N, h, w, frame column offset, map column offset of the view mode)
CASES = [(1, dctenergy.DCTE_LQR, 16, 37, 20011, 1, 3),
         (3, dctenergy.DCTE_LQR, 8, 24, 6007, 2, 1),
         (4, dctenergy.DCTE_PREVIEW, 4, 9, 4600, 3, 2),
         (1, dctenergy.DCTE_PREVIEW, 2, 1, 9001, 2, 3),
         (3, dctenergy.DCTE_PREVIEW, 16, 40, 5501, 1, 2)]
_IDS = [f"bpp{c[0]}-sem{c[1]}-n{c[2]}-{c[3]}x{c[4]}" for c in CASES]


def _torch():
    import torch
    return torch


def _frame(bpp, h, w, seed):
    """Random content with every fifth column flattened: the recomputed band
    holds ties, so the update's refinement runs."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w) + ((bpp,) if bpp > 1 else ()), dtype=np.uint8)
    img[:, ::5] //= 9
    return img


def _zigzag(h, centre, width):
    return np.clip(centre + np.array([-1, 0, 1, 0])[np.arange(h) % 4], 0, width - 1)


def _wide_seams(h, bpp, seed):
    """The 8 steps, each drawn for the width it is applied at."""
    return [lambda k, hh, wk: np.zeros(hh, np.int64),               # in place: the whole row moves
            lambda k, hh, wk: np.full(hh, wk - 1),
            lambda k, hh, wk: np.full(hh, wk - 2),
            lambda k, hh, wk: random_seams(hh, wk, seed, 4)[0],     # connected walk
            lambda k, hh, wk: random_seams(hh, wk, seed + 1, 4)[1],  # arbitrary jumps
            lambda k, hh, wk: _zigzag(hh, 2048, wk),                # the map pass edge (aligned rows)
            lambda k, hh, wk: _zigzag(hh, 8192 // bpp, wk),         # the frame pass edge
            lambda k, hh, wk: np.ones(hh, np.int64)]


def _wide_run(ctx, img, n, sem, seams, inplace, offs):
    """Carve seams one by one on the device and check every step.

    offs None: dense tensors as the allocator returns them.  offs (c0, m0):
    the frame is buf[:, c0:c0 + w] of an (h, w + pad[, bpp]) uint8 buffer
    (w + pad odd), the map mbuf[:, m0:m0 + w] of an (h, w + 7) float buffer;
    in copy mode the outputs are views of the same kind at the next offsets,
    so source and destination alignments differ.

    Before a step everything outside the views is filled with sentinels.
    After it, bitwise:
      copy      outside [0, w_k - 1) of the output views nothing changed,
                and the input buffers did not change at all;
      in place  the frame buffer changed only inside [s[y], w_k - 1) of the
                view's row y (the vacated pixel and the guards keep their
                bytes); the map buffer only inside columns
                [max(0, lo(y) - HR), w_k - 1) of the view's row y.
    """
    torch = _torch()
    dev = torch.device("cuda")
    h, w = img.shape[:2]
    tail = img.shape[2:]
    nbuf = 1 if inplace else 2
    F, M, C0, M0 = [], [], [], []
    for j in range(nbuf):
        if offs is None:
            c0 = m0 = 0
            fw = mw = w
        else:
            c0, m0 = (offs[0] - 1 + j) % 3 + 1, (offs[1] - 1 + j) % 3 + 1
            fw, mw = w + 5 - (w & 1), w + 7
        F.append(torch.full((h, fw) + tail, SENT_B, dtype=torch.uint8, device=dev))
        M.append(torch.full((h, mw), SENT_F, dtype=torch.int32, device=dev).view(torch.float32))
        C0.append(c0)
        M0.append(m0)
    cur = 0
    F[0][:, C0[0]:C0[0] + w] = torch.from_numpy(img).to(dev)
    first = torch.empty((h, w), dtype=torch.float32, device=dev)
    ctx.energy_map_tensor(torch.from_numpy(img).to(dev), first, n, E, T, semantics=sem)
    M[0][:, M0[0]:M0[0] + w] = first
    host = img
    for k, s in enumerate(seams):
        wk = w - k
        if callable(s):
            s = s(k, h, wk)
        s = np.clip(s, 0, wk - 1).astype(np.int32)
        src, dst = cur, (cur if inplace else 1 - cur)
        cs, ms, cd, md = C0[src], M0[src], C0[dst], M0[dst]
        # sentinels everywhere outside the views
        for buf, a in ((F[src], cs), (M[src].view(torch.int32), ms)):
            sent = SENT_B if buf.dtype == torch.uint8 else SENT_F
            buf[:, :a] = sent
            buf[:, a + wk:] = sent
        if not inplace:
            F[dst].fill_(SENT_B)
            M[dst].view(torch.int32).fill_(SENT_F)
        pre_f, pre_m = F[src].cpu().numpy(), M[src].view(torch.int32).cpu().numpy()
        pin, min_ = F[src][:, cs:cs + wk], M[src][:, ms:ms + wk]
        pout, mout = F[dst][:, cd:cd + wk - 1], M[dst][:, md:md + wk - 1]
        if offs is not None:
            assert pin.data_ptr() % 16 != 0 or pin.stride(0) % 16 != 0
            assert min_.data_ptr() % 16 != 0
        ctx.seam_carve_tensor(pin, torch.from_numpy(s).to(dev), min_, pout, mout, n, E, T,
                              semantics=sem)
        full = torch.empty((h, wk - 1), dtype=torch.float32, device=dev)
        ctx.energy_map_tensor(pout.contiguous(), full, n, E, T, semantics=sem)
        torch.cuda.synchronize()
        host = carve(host, s)
        post_f, post_m = F[dst].cpu().numpy(), M[dst].view(torch.int32).cpu().numpy()
        what = f"seam {k} (width {wk})"

        # the frame: the carved pixels in the view, every other byte as before
        want_f = pre_f.copy() if inplace else np.full_like(post_f, SENT_B)
        want_f[:, cd:cd + wk - 1] = host
        if not np.array_equal(post_f, want_f):
            bad = np.argwhere(post_f != want_f)[:5]
            raise AssertionError(f"{what}: {int((post_f != want_f).sum())} frame-buffer bytes "
                                 f"wrong, first {bad.tolist()} (view starts at column {cd})")

        # the map: the view equals the full map of the carved frame ...
        got = post_m[:, md:md + wk - 1].view(np.float32)
        want = full.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)[:5]
            raise AssertionError(f"{what}: {int((got != want).sum())} pixels differ from the "
                                 f"full map, first {bad.tolist()}")
        # ... and nothing around it was written
        keep = np.ones(post_m.shape, bool)
        keep[:, md:md + wk - 1] = False
        before = pre_m if inplace else np.full_like(post_m, SENT_F)
        if inplace:
            lo, _, _, hr = seam_span(s, wk, n, sem)
            left = np.arange(wk - 1)[None, :] < np.maximum(0, lo - hr)[:, None]
            keep[:, md:md + wk - 1] = left
        if not np.array_equal(post_m[keep], before[keep]):
            bad = np.argwhere(keep & (post_m != before))[:5]
            raise AssertionError(f"{what}: map-buffer floats outside the step's range written, "
                                 f"first {bad.tolist()} (view starts at column {md})")
        if not inplace:
            assert np.array_equal(F[src].cpu().numpy(), pre_f), f"{what}: input frame changed"
            assert np.array_equal(M[src].view(torch.int32).cpu().numpy(), pre_m), \
                f"{what}: input map changed"
        cur = dst
    return host, got.copy()


_REF = {}


def _final_ref(key, host, n, sem):
    """The oracle's map of the final frame: one per case (the seams do not
    depend on the mode, so all four runs of a case end on the same frame)."""
    if key not in _REF:
        fn = O.energy_map if sem == dctenergy.DCTE_LQR else O.preview_map
        _REF[key] = (host.copy(), fn(host, n, E, T, nthreads=NT))
    frame, ref = _REF[key]
    assert np.array_equal(frame, host)
    return ref


@pytest.mark.parametrize("view", [False, True], ids=["dense", "view"])
@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_wide_carve(ctx, case, inplace, view):
    bpp, sem, n, h, w, c0, m0 = case
    assert w > 4 * 256 * 4 and w * bpp > 16 * 256 * 2           # several passes at SHIFT_VEC 1, 2, 4
    img = _frame(bpp, h, w, seed=w)
    host, Emap = _wide_run(ctx, img, n, sem, _wide_seams(h, bpp, seed=n + w), inplace,
                           (c0, m0) if view else None)
    assert host.shape[1] == w - 8
    assert within_tol(Emap, _final_ref(case, host, n, sem)).all()


@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
def test_narrow_carve_on_offset_view(ctx, inplace):
    """The narrow end of the same code: a 15-byte-wide RGB row on an offset
    view carved to 2 pixels -- d0 clamps to o1, the row is all head."""
    img = _frame(3, 9, 5, seed=5)
    seams = [np.full(9, k, np.int32) for k in range(3)]         # first, inner, last column
    host, Emap = _wide_run(ctx, img, 8, dctenergy.DCTE_LQR, seams, inplace, (3, 1))
    assert host.shape[1] == 2
    assert within_tol(Emap, O.energy_map(host, 8, E, T)).all()
