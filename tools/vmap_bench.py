"""Seam visibility map kernels on real seams: dcte_vmap_device and
dcte_vmap_render_device (delta = -depth, +depth, 0), each beside the yardstick
it is to be read against ("Seam visibility map").

    python tools/vmap_bench.py [--cases 4096:512,16384:2048] [--n 8] [--reps 5]

Per case (a size x size RGB frame, `depth` seams) the seams come from one
dcte_carve-style loop on the device (map, then seam search + in-place carve per
step), timed as a whole.  Times are HIP events after one warm-up, the median of
--reps.  Yardsticks:
  vmap    the duration of the carve loop that produced its input (the fraction
          is printed);
  render  its own HBM traffic, W*H*(bpp + 4) + (W + delta)*H*bpp bytes, at the
          bandwidth a device-to-device copy of half as many bytes (so the same
          read + write traffic) reaches in the same run.
One JSON line per measurement.  (tools/resize_bench.py is the plug-in hook's
bench; this one has no liblqr in it.)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dct-carver_amd")]


def timed(torch, fn, reps):
    fn()                                        # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="4096:512,16384:2048", help="size:depth,...")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import dctenergy
    from dctenergy import synth
    if not torch.cuda.is_available():
        raise SystemExit("vmap_bench needs a HIP device")
    bpp = 3
    with dctenergy.Context(ngpus=1) as ctx:
        for case in a.cases.split(","):
            size, depth = (int(v) for v in case.split(":"))
            W = H = size
            frame = synth.natural_rows(0, H, W, bpp, seed=0, device="cuda")
            cur = frame.clone()
            emap = torch.empty((H, W), dtype=torch.float32, device="cuda")
            seams = torch.empty((depth, H), dtype=torch.int32, device="cuda")
            # the loop of dcte_carve, seams kept in HBM
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ctx.energy_map_tensor(cur, emap, a.n, 0.5, 0.5)
            for k in range(depth):
                wk = W - k
                ctx.seam_find_tensor(emap[:, :wk], seams[k])
                ctx.seam_carve_tensor(cur[:, :wk], seams[k], emap[:, :wk], cur[:, :wk - 1],
                                      emap[:, :wk - 1], a.n, 0.5, 0.5)
            t1.record()
            t1.synchronize()
            loop_ms = t0.elapsed_time(t1)
            if int(seams[:, 0].min()) < 0:
                raise SystemExit("a seam search timed out; run on an idle device")
            del cur, emap
            tag = {"frame": f"{W}x{H} RGB", "depth": depth, "n": a.n}
            vmap = torch.empty((H, W), dtype=torch.int32, device="cuda")
            ms = timed(torch, lambda: ctx.vmap_tensor(seams, vmap), a.reps)
            print(json.dumps({**tag, "kernel": "dcte_vmap_device", "ms": round(ms, 4),
                              "carve_loop_ms": round(loop_ms, 2),
                              "fraction_of_carve_loop": round(ms / loop_ms, 6)}), flush=True)
            for delta in (-depth, depth, 0):
                out = torch.empty((H, W + delta, bpp), dtype=torch.uint8, device="cuda")
                nbytes = W * H * (bpp + 4) + (W + delta) * H * bpp
                src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
                dst = torch.empty_like(src)
                copy_ms = timed(torch, lambda: dst.copy_(src), a.reps)     # hipMemcpyDtoD
                bw = 2 * src.numel() / (copy_ms * 1e-3)
                ms = timed(torch, lambda: ctx.vmap_render_tensor(frame, vmap, depth, delta, out),
                           a.reps)
                floor_ms = nbytes / bw * 1e3
                print(json.dumps({**tag, "kernel": "dcte_vmap_render_device", "delta": delta,
                                  "ms": round(ms, 4), "bytes": nbytes,
                                  "copy_GBps": round(bw / 1e9, 1),
                                  "floor_ms": round(floor_ms, 4),
                                  "times_floor": round(ms / floor_ms, 2)}), flush=True)
                del out, src, dst
            del frame, vmap, seams


if __name__ == "__main__":
    main()
