"""GPU: dcte_minmax / dcte_to_u8 past one grid stride and on float-aligned bases.

Both kernels run a grid capped at 4096 workgroups of 256: one stride is
4 194 304 floats for min/max (float4 per thread) and 1 048 576 for u8.  The
maps of test_gpu_parity.py stay below 1.4 M floats, so the min/max loop
never ran a second time there; a 16384^2 energy layer runs it 64 times.
Here n = 2 * 4194304 + 4099: two whole min/max strides, a partial third,
n % 4 == 3 (a scalar tail), 9 u8 strides -- with the extrema placed where
only a later iteration, the tail or the first element sees them, and the
base 0..3 floats off 16-byte alignment (a row slice of an odd-width map is
contiguous and only 4-byte aligned; dcte_minmax peels the floats below the
first 16-byte boundary).  Everything is equality: min/max against numpy,
the bytes against the numpy restatements of both normalisations.
"""
import numpy as np
import pytest

import dctenergy
import oracle_py as O

pytestmark = pytest.mark.gpu

STRIDE = 4096 * 256 * 4
N = 2 * STRIDE + 4099
MODES = ((dctenergy.DCTE_NORM_LQR, O.normalize_lqr), (dctenergy.DCTE_NORM_PREVIEW, O.normalize_preview))
LAYOUTS = ["extrema_in_second_stride", "extrema_in_scalar_tail", "min_first_max_last",
           "signed_with_both_zeros", "constant"]


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def base():
    b = np.random.default_rng(77).random(N, dtype=np.float32)
    b.setflags(write=False)
    return b


def _layout(base, name):
    if name == "constant":
        return np.full(N, 0.25, np.float32)
    if name == "signed_with_both_zeros":
        e = base * np.float32(8) - np.float32(3)          # [-3, 5)
        e[[5, STRIDE + 1, N - 2]] = np.float32(-0.0)
        e[[6, STRIDE + 2, N - 1]] = np.float32(0.0)
        return e
    # values strictly inside (0, 1), so the two planted extrema are the only ones
    e = np.clip(base, np.float32(2.0 ** -10), np.float32(1 - 2.0 ** -10))
    lo, hi = np.float32(0.0), np.nextafter(np.float32(1), np.float32(0))
    at = {"extrema_in_second_stride": (STRIDE + 123457, 2 * STRIDE - 2),
          "extrema_in_scalar_tail": (N - 1, N - 2),
          "min_first_max_last": (0, N - 1)}[name]
    e[at[0]], e[at[1]] = lo, hi
    assert e.argmin() == at[0] and e.argmax() == at[1]
    return e


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("name", LAYOUTS)
def test_minmax_and_u8_past_one_stride(ctx, base, name, off):
    torch = _torch()
    E = _layout(base, name)
    buf = torch.empty(N + 3, dtype=torch.float32, device="cuda")
    dE = buf[off:off + N]
    dE.copy_(torch.from_numpy(E))
    assert dE.data_ptr() % 16 == 4 * off
    st = torch.cuda.current_stream().cuda_stream
    mm = torch.full((2,), np.nan, dtype=torch.float32, device="cuda")
    ctx.minmax_device(dE.data_ptr(), N, mm.data_ptr(), st)
    torch.cuda.synchronize()
    got = mm.cpu().numpy()
    # ==, not bits: which zero a map with -0.0 and +0.0 reports is not specified
    assert got[0] == E.min() and got[1] == E.max(), (got, E.min(), E.max())
    minmax = (E.min(), E.max())
    for mode, restate in MODES:
        one = restate(E, 1, minmax)
        for ch in (1, 2, 3, 4):
            out = torch.full((N * ch + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            ctx.normalize_u8_device(dE.data_ptr(), N, mm.data_ptr(), out.data_ptr(), mode, ch, st)
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            want = np.repeat(one, ch)          # restate(E, ch, minmax): it replicates the same bytes
            if not np.array_equal(o[:N * ch], want):
                bad = np.flatnonzero(o[:N * ch] != want)
                k = bad[0] // ch
                raise AssertionError(f"mode {mode} channels {ch}: {len(bad)} bytes differ, first at "
                                     f"element {k}: E = {E[k]!r}, got {o[bad[0]]}, want {want[bad[0]]}, "
                                     f"host C entry {dctenergy.normalize_u8_host(E, mode)[k]}")
            assert (o[N * ch:] == 0xA5).all(), (mode, ch)
            if name == "constant":
                assert not want.any()


def test_host_normalize_past_four_strides(ctx):
    """dcte_normalize_u8 (upload, both kernels, download) on a 3000 x 1401 map,
    more than 4 u8 strides: the numpy restatements' and the host C entry's bytes."""
    rng = np.random.default_rng(78)
    Emap = (rng.random((3000, 1401), dtype=np.float32) * np.float32(0.37)).astype(np.float32)
    Emap[2999, 1400], Emap[1500, 7] = np.float32(0.5), np.float32(-0.125)   # max last, min mid-map
    for mode, restate in MODES:
        for ch in (1, 3):
            got = ctx.normalize_u8(Emap, mode, ch)
            assert np.array_equal(got, restate(Emap, ch)), (mode, ch)
            assert np.array_equal(got, dctenergy.normalize_u8_host(Emap, mode, ch)), (mode, ch)


def test_sharded_u8_on_a_float_aligned_band(ctx):
    """dist.energy_image_u8 on one rank with band_map = E2d[1:] of a
    301-column map: contiguous, 4 bytes past 16-byte alignment.  The frame's
    min and max lie in the band, so its bytes are those rows of the
    full-frame layer."""
    torch = _torch()
    from dctenergy import dist as D
    rng = np.random.default_rng(79)
    E2 = rng.random((40, 301), dtype=np.float32)
    E2[0] = np.float32(0.5)
    E2[5, 7], E2[39, 300] = np.float32(-1), np.float32(2)
    dE = torch.from_numpy(E2).cuda()
    band = dE[1:]
    assert band.is_contiguous() and band.data_ptr() % 16 == 4
    for mode, restate in MODES:
        for ch in (1, 3):
            out = torch.empty((39, 301) + ((ch,) if ch > 1 else ()), dtype=torch.uint8, device="cuda")
            D.energy_image_u8(ctx, band, out, mode, ch)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got, restate(E2[1:], ch, (E2.min(), E2.max()))), (mode, ch)
            assert np.array_equal(got, ctx.normalize_u8(E2, mode, ch)[1:]), (mode, ch)
