"""Device time of ECC registration (sg_register_ecc_u16_device) on frames resident in HBM.

  python scripts/ecc_profile.py --all [--out-dir profiles]          both configurations below, one child
                                                                   process each under its own time limit
  python scripts/ecc_profile.py --frames N --height H --width W [--reps 3] [--warmup 1]

Configurations of --all: 64 x 4096^2 (a few large frames) and 2000 x 640 x 480 (a planetary sequence).
The frames are 8-bit scenes rendered on the device: a field of Gaussian blobs (amplitude <= 230 on a
pedestal of 12) sampled at a known sub-pixel shift per frame (|s| <= 4), noise sigma 2.  Frame 0 is the
reference.  Per configuration the log records, median of `reps` calls after `warmup`:
  ms per call            HIP events on the stream around the whole synchronous call
  prepare / iterate ms   the library's own HIP events around its prepare launches and its iteration
                         launches (sg_register_ecc_last_times; the second span holds the host's reads of
                         the unfinished-frame count every few launches)
  mean iterations per frame, iteration launches
  the iteration kernel's bytes 4 B * W * H * sum(iterations) against 8 TB/s
  max |dx - planted|, |dy - planted| and the number of failed frames."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(64, 4096, 4096, 420), (2000, 480, 640, 300)]   # frames, H, W, time limit (s)
HBM_BW = 8.0e12


def run_all(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for n, h, w, limit in CONFIGS:
        log = os.path.join(out_dir, f"ecc_{n}x{h}x{w}.log")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--frames", str(n),
               "--height", str(h), "--width", str(w)]
        with open(log, "w") as f:
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT).returncode
        print(f"{log}: exit {rc}", flush=True)
        if rc != 0:     # nothing more is started on the device after a step that failed
            return rc
    return 0


def scene(torch, n, H, W, seed):
    """[n][H][W] int16 (u16 bits) on the device, and the planted (sx, sy) per frame"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    M = 8
    field = torch.zeros(1, 1, H + 2 * M, W + 2 * M, device="cuda")
    nb = max(8, (H * W) // 400)
    iy = torch.randint(0, H + 2 * M, (nb,), device="cuda", generator=g)
    ix = torch.randint(0, W + 2 * M, (nb,), device="cuda", generator=g)
    field[0, 0, iy, ix] = 40 + 190 * torch.rand(nb, device="cuda", generator=g)
    sig = 2.5
    t = torch.arange(-8, 9, device="cuda", dtype=torch.float32)
    k = torch.exp(-t * t / (2 * sig * sig))     # peak 1: an isolated blob keeps its amplitude
    field = torch.nn.functional.conv2d(field, k.view(1, 1, 1, -1), padding=(0, 8))
    field = torch.nn.functional.conv2d(field, k.view(1, 1, -1, 1), padding=(8, 0))
    base = (12 + field[0, 0]).clamp(max=242)
    frames = torch.empty(n, H, W, dtype=torch.int16, device="cuda")
    shifts = (torch.rand(n, 2, generator=torch.Generator().manual_seed(seed)) * 8 - 4).tolist()
    shifts[0] = [0.0, 0.0]
    for f, (sx, sy) in enumerate(shifts):
        # content moved by +s: frame(x) = base(x - s), bilinear
        fx, fy = int(sx // 1), int(sy // 1)
        ax, ay = sx - fx, sy - fy
        y0, x0 = M - fy, M - fx

        def at(dy, dx):
            return base[y0 - dy:y0 - dy + H, x0 - dx:x0 - dx + W]
        v = (1 - ay) * ((1 - ax) * at(0, 0) + ax * at(0, 1)) + ay * ((1 - ax) * at(1, 0) + ax * at(1, 1))
        v = v + 2.0 * torch.randn(H, W, device="cuda", generator=g)
        frames[f] = v.round().clamp(0, 255).to(torch.int16)
    return frames, shifts


def run_one(a):
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    import sirilgpu as sg
    N, H, W = a.frames, a.height, a.width
    frames, shifts = scene(torch, N, H, W, 1)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    print(f"ecc: {N} frames of {H} x {W} (8-bit scenes, planted |s| <= 4, noise sigma 2), reference frame 0", flush=True)
    with sg.Context([0]) as ctx:
        ms, prep, it, res, launches = [], [], [], None, 0
        for r in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc, res = ctx.register_ecc_device(frames.data_ptr(), N, H, W, stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError(f"rc {rc}: {ctx.error()}")
            if r >= a.warmup:
                p, i, launches = ctx.register_ecc_last_times()
                ms.append(e0.elapsed_time(e1))
                prep.append(p)
                it.append(i)
    med, mp, mi = statistics.median(ms), statistics.median(prep), statistics.median(it)
    total_it = int(res["iterations"].sum())
    ok = res["failed"] == 0
    ok[0] = False
    want = np.array(shifts)
    err = np.abs(np.stack([res["dx"], res["dy"]], axis=1) - want)[ok]
    print(f"call: median of {a.reps}: {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), {med / N * 1e3:.1f} us per frame")
    print(f"prepare launches: {mp:.3f} ms ({4.0 * N * H * W / mp / 1e6:.0f} GB/s at 4 B per pixel: 2 read, 2 written)")
    print(f"iteration launches: {mi:.3f} ms over {launches} launches, {total_it} frame-iterations, "
          f"mean {total_it / (N - 1):.2f} iterations per frame (max {int(res['iterations'].max())})")
    nbytes = 4.0 * W * H * total_it
    print(f"iteration bytes 4 B * W * H * sum(iterations) = {nbytes / 1e9:.3f} GB: {nbytes / mi / 1e6:.0f} GB/s, "
          f"{100.0 * nbytes / (mi * 1e-3) / HBM_BW:.1f} % of 8 TB/s")
    print(f"failed frames: {int((res['failed'] != 0).sum())}; max |dx - planted| {err[:, 0].max():.4f}, "
          f"max |dy - planted| {err[:, 1].max():.4f} px", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.out_dir))
    run_one(a)


if __name__ == "__main__":
    main()
