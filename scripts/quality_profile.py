"""Device time of the quality estimate (sg_quality_u16_device) on frames resident in HBM.

  python scripts/quality_profile.py --all [--out-dir profiles]     the five configurations below, one child
                                                                   process each under its own time limit
  python scripts/quality_profile.py --frames N --height H --width W [--reps 10] [--warmup 2]

Configurations of --all: 8192 x (240 x 320) and 4096 x (480 x 640) (planetary sequences), 1024 x (960 x 1280), 128 x 2048^2 and
64 x 4096^2.  The frames are rendered on the device: a soft disk with a texture, a per-frame gain and a
small deterministic noise on a pedestal, as tests/quality_cases.py draws them.  Both routes run in the same
process, alternating call by call (the resident route only where a frame fits one workgroup's LDS), through
two contexts made with SG_QUALITY_ROUTE.  Per route the log records, over `reps` calls after `warmup`:
  device ms              the library's own HIP events around the call's launches (sg_quality_last_times):
                         median, smallest, largest
  call ms                HIP events on the stream around the whole synchronous call (with the list upload
                         and the result copy)
  achieved bytes/s       2 * W * H bytes per frame (the frame is read once) over the median device time
and the route the rule of DESIGN §2 makes the default here: a route only if its median is below the other
route's smallest time.  Both routes must give the same bits for every frame, and the oracle's for the first
and the last frame."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(8192, 240, 320, 240), (4096, 480, 640, 240), (1024, 960, 1280, 240), (128, 2048, 2048, 240), (64, 4096, 4096, 300)]   # frames, H, W, limit (s)
HBM_BW = 8.0e12


def run_all(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for n, h, w, limit in CONFIGS:
        log = os.path.join(out_dir, f"quality_{n}x{h}x{w}.log")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--frames", str(n),
               "--height", str(h), "--width", str(w)]
        with open(log, "w") as f:
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT).returncode
        print(f"{log}: exit {rc}", flush=True)
        if rc != 0:     # nothing more is started on the device after a step that failed
            return rc
    return 0


def scene(torch, n, H, W):
    """[n][H][W] int16 (u16 bits) on the device"""
    y = torch.arange(H, device="cuda", dtype=torch.float32).view(H, 1)
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, W)
    r = torch.hypot(x - (W * 0.5 + 0.3), y - (H * 0.5 - 0.4))
    disk = 1.0 / (1.0 + torch.exp((r - min(H, W) * 0.3).clamp(max=60.0)))
    noise = ((x * 73 + y * 151) % 7) - 3
    frames = torch.empty(n, H, W, dtype=torch.int16, device="cuda")
    for f in range(n):
        tex = 0.25 * torch.sin(x * 0.9 + f) * torch.cos(y * 0.7)
        v = 20 + (200 + 17 * (f % 13)) * disk * (0.75 + tex) + torch.roll(noise, f % 7, 1)
        frames[f] = v.round().clamp(0, 65535).to(torch.int32).to(torch.int16)
    return frames


def make_context(sg, route):
    os.environ["SG_QUALITY_ROUTE"] = str(route)
    try:
        return sg.Context([0])
    finally:
        del os.environ["SG_QUALITY_ROUTE"]


def run_one(a):
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as orc
    import sirilgpu as sg
    N, H, W = a.frames, a.height, a.width
    frames = scene(torch, N, H, W)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    print(f"quality: {N} frames of {H} x {W} rendered on the device, {(W - 1) // 3} x {(H - 1) // 3} samples per frame", flush=True)
    ctx = {r: make_context(sg, r) for r in (1, 2)}
    dev, call, took, q = {1: [], 2: []}, {1: [], 2: []}, {}, {}
    try:
        for rep in range(a.warmup + a.reps):
            for r in (1, 2):
                if r == 1 and took.get(1, 1) != 1:
                    continue        # the frame does not fit the resident route: the context fell back to the tiled one
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc, q[r] = ctx[r].quality_device(frames.data_ptr(), N, H, W, stream=stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize()
                if rc != 0:
                    raise RuntimeError(f"rc {rc}: {ctx[r].error()}")
                ms, took[r], launches = ctx[r].quality_last_times()
                if rep >= a.warmup and took[r] == r:
                    dev[r].append(ms)
                    call[r].append(e0.elapsed_time(e1))
    finally:
        for c in ctx.values():
            c.close()
    nbytes = 2.0 * W * H * N
    med = {}
    for r, name in ((1, "resident"), (2, "tiled")):
        if not dev[r]:
            print(f"route {r} ({name}): a frame does not fit one workgroup's LDS, not run")
            continue
        med[r] = statistics.median(dev[r])
        print(f"route {r} ({name}): device median of {len(dev[r])}: {med[r]:.3f} ms (min {min(dev[r]):.3f}, max {max(dev[r]):.3f}), "
              f"{med[r] / N * 1e3:.2f} us per frame; call median {statistics.median(call[r]):.3f} ms "
              f"(min {min(call[r]):.3f}, max {max(call[r]):.3f})")
        print(f"route {r} ({name}): 2 * W * H * N = {nbytes / 1e9:.3f} GB read: {nbytes / med[r] / 1e6:.0f} GB/s, "
              f"{100.0 * nbytes / (med[r] * 1e-3) / HBM_BW:.1f} % of 8 TB/s")
    if 1 in med:
        same = q[1].tobytes() == q[2].tobytes()
        print(f"both routes the same bits for all {N} frames: {same}")
        default = 1 if med[1] < min(dev[2]) else 2
        print(f"default by the rule (a route only if its median is below the other's smallest time): route {default} "
              f"(resident median {med[1]:.3f} ms against tiled min {min(dev[2]):.3f} ms; tiled median {med[2]:.3f} ms against "
              f"resident min {min(dev[1]):.3f} ms)")
        if not same:
            raise RuntimeError("the routes differ")
    host = frames[[0, N - 1]].cpu().numpy().view(np.uint16)
    want = [orc.quality(host[0]), orc.quality(host[1])]
    got = [float(q[2][0]), float(q[2][N - 1])]
    print(f"frames 0 and {N - 1}: {got} against the oracle's {want}", flush=True)
    if got != want:
        raise RuntimeError("the device differs from the oracle")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.out_dir))
    run_one(a)


if __name__ == "__main__":
    main()
