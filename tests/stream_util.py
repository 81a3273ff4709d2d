"""Helpers for tests/test_streams.py: frames that make the refinement lists
work, a calibrated device-side delay, and the enqueue pattern that shows
whether a library call is ordered on the caller's stream (test
infrastructure; the GPU parts import torch lazily)."""
import time

import numpy as np

import emu_py as EM

H, W = 300, 400              # several 64-column strips, more than one tile row
STRIP_W, TILE_H = 64, 16     # a refinement strip of frames this small (pick_tile_h
#                              takes the shortest tile while every tile is resident)
FIX_DIRECT = 16              # kFixDirect<8>: more flagged pixels make a strip dense
E, T = 0.3, 0.7              # e != t: the refinement launch runs
DELAY_MS = 30.0


def natural(h, w, channels, seed):
    """The bench's natural-like frame (dctenergy.synth), drawn with numpy."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 128.0 + 60.0 * np.sin(x / 17.0) + 40.0 * np.cos(y / 11.0)
    img = base[..., None] + 20.0 * rng.standard_normal((h, w, channels))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img[..., 0].copy() if channels == 1 else img


def tie_frame(channels, seed=0, h=H, w=W):
    """Left half natural; right half tie-prone as in test_gpu_parity's
    _stress_frames: 1-pixel line art on white, then random dots on flat
    ground -- sparse and dense strips side by side.  RGBA: a random alpha."""
    rng = np.random.default_rng(1000 + seed)
    img = natural(h, w, min(channels, 3), seed)
    yy, xx = np.mgrid[0:h, 0:w]
    art = np.where((yy % 23 == 0) | (xx % 31 == 0) | ((xx + 2 * yy) % 97 == 0), 0, 255)
    dots = np.where(rng.random((h, w)) < 1 / 64, 255, 16)
    a, b = w // 2, w // 2 + w // 4
    right = np.where(xx < b, art, dots).astype(np.uint8)
    if channels == 1:
        img[:, a:] = right[:, a:]
        return img
    img[:, a:] = right[:, a:, None]
    if channels == 4:
        img = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
    return np.ascontiguousarray(img)


def strip_counts(img, n, sem=0, e=E, t=T):
    """Flagged pixels per refinement strip (STRIP_W columns x TILE_H rows)
    from the host emulation of the fast path."""
    _, me, mt = EM.energy_map(img, n, e, t, sem=sem)
    m = EM.refine_mask(me, mt, e, t, n)
    h, w = m.shape
    ph, pw = -h % TILE_H, -w % STRIP_W
    m = np.pad(m, ((0, ph), (0, pw)))
    return m.reshape(m.shape[0] // TILE_H, TILE_H, m.shape[1] // STRIP_W, STRIP_W).sum((1, 3))


class Delay:
    """A piece of device work of a known minimum duration, enqueued on the
    current stream: torch.cuda._sleep, calibrated with events; a chain of
    element-wise passes over a large tensor where _sleep is unusable."""

    def __init__(self, torch, ms=DELAY_MS):
        self.torch = torch
        self.trace = []                            # (kind, arg, measured ms) of every step
        self.kind, self.arg = "sleep", 1_000_000
        try:
            self.ms = self._calibrate(ms)
        except (RuntimeError, AttributeError):
            self.ms = 0.0
        if not 0.9 * ms <= self.ms <= 3 * ms:
            self.kind, self.arg = "chain", 4
            self.big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
            self.ms = self._calibrate(ms)

    def _calibrate(self, ms):
        """Scale the argument until the measured duration is ms .. 1.5 ms; the
        first, untimed run takes the kernel's loading out of the figures.
        -> the shortest of three timings of the final argument."""
        self.enqueue()
        for _ in range(8):
            got = self._time(self.enqueue)
            self.trace.append((self.kind, self.arg, got))
            if ms <= got <= 1.5 * ms:
                break
            self.arg = min(1 << 40 if self.kind == "sleep" else 4096, max(1, int(np.ceil(self.arg * 1.2 * ms / max(got, 1e-3)))))
        got = min(self._time(self.enqueue) for _ in range(3))
        self.trace.append((self.kind, self.arg, got))
        return got

    def _time(self, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def enqueue(self):
        if self.kind == "sleep":
            self.torch.cuda._sleep(self.arg)
        else:
            for _ in range(self.arg):
                self.big.add_(1.0)


class Case:
    """One library call with its device buffers.

    inputs:   [(buffer the call reads, true contents, decoy contents)], device
              tensors of one shape each -- the decoy is another valid input
    outputs:  [(tensor the call writes, sentinel)]
    call:     call(ctx, stream pointer) enqueues the library call(s)
    """

    def __init__(self, name, inputs, outputs, call):
        self.name, self.inputs, self.outputs, self.call = name, inputs, outputs, call

    def fill(self, which):
        for buf, true, decoy in self.inputs:
            buf.copy_(true if which == "true" else decoy)
        for out, sentinel in self.outputs:
            out.fill_(sentinel)

    def results(self):
        return [out.cpu().numpy().copy() for out, _ in self.outputs]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run_alone(torch, ctx, case, which="true"):
    """The call alone on the null stream, synchronised -> its outputs."""
    torch.cuda.synchronize()
    case.fill(which)
    torch.cuda.synchronize()
    case.call(ctx, 0)
    torch.cuda.synchronize()
    return case.results()


def run_ordered(torch, ctx, case, delay, side=None, warm=True):
    """delay | the call on the decoy | true input in | the call | event | decoy back, all on a
    non-blocking side stream with no host sync in between.  Returns (outputs,
    host seconds of the call)."""
    side = side or torch.cuda.Stream()
    if warm:                       # scratch for this stream and shape exists
        case.fill("true")
        torch.cuda.synchronize()
        case.call(ctx, side.cuda_stream)
        side.synchronize()
    case.fill("decoy")
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(side):
        delay.enqueue()
        # the same call on the decoy first: the call under test must also be
        # ordered after an earlier one that is still queued (its counters and
        # lists are that call's until it has run)
        case.call(ctx, side.cuda_stream)
        for buf, true, _ in case.inputs:
            buf.copy_(true, non_blocking=True)
        t0 = time.perf_counter()
        case.call(ctx, side.cuda_stream)
        host_s = time.perf_counter() - t0
        ev.record(side)
        for buf, _, decoy in case.inputs:
            buf.copy_(decoy, non_blocking=True)
    pending = not ev.query()
    side.synchronize()
    # the call returned without waiting, and the delay outlasted the host side
    assert pending, f"{case.name}: the call's work had finished when it returned"
    for buf, _, decoy in case.inputs:
        assert torch.equal(buf, decoy), f"{case.name}: decoy not restored"
    return case.results(), host_s
