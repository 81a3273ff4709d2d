"""DCTE_LQR_ALPHA maps and carves beside their yardstick ("RGBA
layers"): the exact-mode RGB map / carve (DCTE_OPT_EXACT, DCTE_LQR) of the same
frame's colour channels, in the same process and run -- only the same-run ratio
is to be read (box-to-box spread is several per cent).

    python tools/alpha_bench.py [--maps 4096:8,16384:8,8192:16] [--carve 4096:64:8] [--reps 5]

Maps: dcte_energy_map_device on a natural size x size RGBA frame in HBM, HIP
events after one warm-up, the median of --reps.  Carve: the host entry
dcte_carve (upload, map, seams x (search + in-place carve + band update),
download), wall clock after one warm-up, the median of --reps.  One JSON line
per measurement.
"""
import argparse
import json
import os
import sys
import time

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


def wall(fn, reps):
    fn()                                        # warm-up
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="4096:8,16384:8,8192:16", help="size:N,...")
    ap.add_argument("--carve", default="4096:64:8", help="size:seams:N,... (empty: none)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import dctenergy
    from dctenergy import synth
    if not torch.cuda.is_available():
        raise SystemExit("alpha_bench needs a HIP device")
    ALPHA, E, T = dctenergy.DCTE_LQR_ALPHA, 0.3, 0.7
    with dctenergy.Context(ngpus=1) as actx, dctenergy.Context(ngpus=1, exact=True) as ex:
        for case in filter(None, a.maps.split(",")):
            size, n = (int(v) for v in case.split(":"))
            rgba = synth.natural_rows(0, size, size, 4, seed=0, device="cuda")
            rgb = rgba[..., :3].contiguous()
            out = torch.empty((size, size), dtype=torch.float32, device="cuda")
            alpha_ms = timed(torch, lambda: actx.energy_map_tensor(rgba, out, n, E, T, semantics=ALPHA),
                             a.reps)
            rgb_ms = timed(torch, lambda: ex.energy_map_tensor(rgb, out, n, E, T), a.reps)
            print(json.dumps({"what": "map", "frame": f"{size}x{size}", "n": n,
                              "alpha_ms": round(alpha_ms, 4), "exact_rgb_ms": round(rgb_ms, 4),
                              "ratio": round(alpha_ms / rgb_ms, 4),
                              "alpha_Gpx_s": round(size * size / alpha_ms / 1e6, 2)}), flush=True)
            del rgba, rgb, out
        for case in filter(None, a.carve.split(",")):
            size, seams, n = (int(v) for v in case.split(":"))
            rgba = synth.natural_rows(0, size, size, 4, seed=1, device="cuda").cpu().numpy()
            rgb = rgba[..., :3].copy()
            alpha_ms = wall(lambda: actx.carve(rgba, seams, n, E, T, semantics=ALPHA), a.reps)
            rgb_ms = wall(lambda: ex.carve(rgb, seams, n, E, T), a.reps)
            print(json.dumps({"what": "carve", "frame": f"{size}x{size}", "seams": seams, "n": n,
                              "alpha_ms": round(alpha_ms, 2), "exact_rgb_ms": round(rgb_ms, 2),
                              "ratio": round(alpha_ms / rgb_ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
