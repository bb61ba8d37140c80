"""Device time of the sequence warp (sg_warp_frames_u16_device) on frames resident in HBM, against one
sg_warp_u16_device call per frame.

  python scripts/warp_profile.py --all [--out-dir profiles]    the two configurations below, one child process
                                                               each under its own time limit, into
                                                               <out-dir>/warp_frames_64x4096.log
  python scripts/warp_profile.py --frames N --layers C --side S [--interps 0,1,3,4] [--reps 10] [--warmup 2]

Configurations of --all: 64 mono frames of 4096^2 and 16 RGB frames of 4096^2, random u16 rendered on the
device.  Every frame has its own similarity homography about the image centre, rotation within +-1 degree
and translation within +-30 pixels, from a seeded generator; the output has the source's size.  Per
interpolation four ways run in one process, alternating turn by turn, each on one caller stream between two
HIP events with a single synchronise after the second:
  (a) frames   one sg_warp_u16_device call per frame (k_warp, the homography in the kernel argument)
  (b) seq      one sg_warp_frames_u16_device call (k_warp_seq, the plan's default route for the interpolation)
  (c) gather   the same call on a context made with SG_WARP_ROUTE=1 (every tile reads global memory)
  (d) lds      the same call on a context made with SG_WARP_ROUTE=2 (every tile whose box fits stages it in LDS)
The log gives the median, smallest and largest of `reps` turns after `warmup`, for (b), (c) and (d) also the
library's own span of the launches (sg_warp_frames_last_times) and the route counters, the algorithmic bytes
(4 per destination pixel, layer and frame: one u16 read, one written) over the median as a share of the
8 TB/s peak, and two verdicts: (b) is accepted if its median is not above (a)'s by more than (a)'s own
largest - smallest; and which of (c) and (d) has the lower median, which is what the plan's default for that
interpolation has to be (sg_warp_plan.hpp).  All four must give the same bytes."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(64, 1, 4096, 480), (16, 3, 4096, 360)]      # frames, layers, side, limit (s)
HBM_BW = 8.0e12
NAMES = {0: "nearest", 1: "linear", 3: "cubic", 4: "lanczos4"}
WAYS = "abcd"


def run_all(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    log = os.path.join(out_dir, "warp_frames_64x4096.log")
    with open(log, "w") as f:
        for n, c, s, limit in CONFIGS:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--frames", str(n),
                   "--layers", str(c), "--side", str(s)]
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT).returncode
            f.flush()
            print(f"{log}: {n} x {c} x {s}^2: exit {rc}", flush=True)
            if rc != 0:     # nothing more is started on the device after a step that failed
                return rc
    return 0


def homographies(np, n, side, seed=20):
    rng = np.random.default_rng(seed)
    c = (side - 1) / 2.0
    out = np.empty((n, 3, 3))
    for f in range(n):
        a = np.deg2rad(rng.uniform(-1.0, 1.0))
        tx, ty = rng.uniform(-30.0, 30.0, 2)
        co, si = np.cos(a), np.sin(a)
        out[f] = [[co, -si, c - co * c + si * c + tx], [si, co, c - si * c - co * c + ty], [0, 0, 1]]
    return out


def make_context(sg, route):
    os.environ["SG_WARP_ROUTE"] = str(route)
    try:
        return sg.Context([0])
    finally:
        del os.environ["SG_WARP_ROUTE"]


def run_one(a):
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    import sirilgpu as sg
    N, C, S = a.frames, a.layers, a.side
    fe = C * S * S
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    frames = torch.randint(-32768, 32768, (N * fe,), dtype=torch.int16, device="cuda", generator=gen)
    outs = {k: torch.zeros(N * fe, dtype=torch.int16, device="cuda") for k in WAYS}
    homs = homographies(np, N, S)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    nbytes = 4.0 * S * S * C * N
    print(f"warp: {N} frames of {C} x {S} x {S} on the device, one similarity each (|rotation| <= 1 degree, |translation| <= 30 px); "
          f"algorithmic bytes {nbytes / 1e9:.3f} GB per call", flush=True)
    ctx = {"b": make_context(sg, 0), "c": make_context(sg, 1), "d": make_context(sg, 2)}
    ctx["a"] = ctx["b"]

    def turn(k, interp):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if k == "a":
            for f in range(N):
                ctx[k].warp_device(frames.data_ptr() + 2 * f * fe, S, S, C, outs[k].data_ptr() + 2 * f * fe, S, S, homs[f], interp,
                                   stream=stream.cuda_stream)
        else:
            rc = ctx[k].warp_frames_device(frames.data_ptr(), N, S, S, C, outs[k].data_ptr(), S, S, homs, interp,
                                           stream=stream.cuda_stream)
            if rc != 0:
                raise RuntimeError(f"rc {rc}: {ctx[k].error()}")
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    try:
        for interp in a.interps:
            t = {k: [] for k in WAYS}
            lib, ctrs = {"b": [], "c": [], "d": []}, {}
            for rep in range(a.warmup + a.reps):
                for k in WAYS:
                    ms = turn(k, interp)
                    if k != "a":
                        own, launches, lds, gather, stray = ctx[k].warp_frames_last_times()
                        ctrs[k] = (launches, lds, gather, stray)
                    if rep >= a.warmup:
                        t[k].append(ms)
                        if k != "a":
                            lib[k].append(own)
            med = {k: statistics.median(t[k]) for k in WAYS}
            print(f"{NAMES[interp]}:")
            for k, what in (("a", f"{N} sg_warp_u16_device calls"), ("b", "one sg_warp_frames_u16_device call"),
                            ("c", "the same, SG_WARP_ROUTE=1"), ("d", "the same, SG_WARP_ROUTE=2")):
                line = (f"  ({k}) {what}: median of {len(t[k])}: {med[k]:.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f}), "
                        f"{nbytes / med[k] / 1e6:.0f} GB/s algorithmic, {100.0 * nbytes / (med[k] * 1e-3) / HBM_BW:.1f} % of 8 TB/s")
                if k != "a":
                    line += (f"; launches' own span median {statistics.median(lib[k]):.3f} ms; launches {ctrs[k][0]}, tiles_lds {ctrs[k][1]}, "
                             f"tiles_gather {ctrs[k][2]}, pixels_stray {ctrs[k][3]}")
                print(line)
            same = all(torch.equal(outs["a"], outs[k]) for k in "bcd")
            spread = max(t["a"]) - min(t["a"])
            print(f"  the four give the same bytes: {same}; non-zero output: {bool(outs['a'].any())}")
            print(f"  acceptance: (b) - (a) = {med['b'] - med['a']:+.3f} ms against (a)'s max - min = {spread:.3f} ms: "
                  f"{'met' if med['b'] - med['a'] <= spread else 'NOT met'}")
            print(f"  routes: (c) gather median {med['c']:.3f} ms (min {min(t['c']):.3f}), (d) LDS median {med['d']:.3f} ms (min {min(t['d']):.3f}): "
                  f"{'gather' if med['c'] < med['d'] else 'LDS'} is the faster; the default took "
                  f"{'LDS' if ctrs['b'][1] else 'gather'}", flush=True)
            if not same:
                raise RuntimeError("the ways differ")
    finally:
        for k in "bcd":
            ctx[k].close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--interps", type=lambda s: [int(v) for v in s.split(",")], default=[0, 1, 3, 4])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.out_dir))
    run_one(a)


if __name__ == "__main__":
    main()
