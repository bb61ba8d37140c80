"""Device time of one-star registration (sg_seqpsf_u16_device) on frames resident in HBM, and the A/B of its
workgroup size.

  python scripts/seqpsf_profile.py --all [--out-dir profiles]      the workload below once per library given
                                                                   by --libs, one child process each under
                                                                   its own time limit
  python scripts/seqpsf_profile.py --frames N --height H --width W --side S [--reps 10] [--warmup 2]

Workload of --all: 4096 frames of 480 x 640 rendered on the device with a 40 x 40 area: one elongated star
that drifts by (0.11, 0.07) pixels per frame on a pedestal with a small deterministic noise.  The workgroup
size is a compile-time constant (SGQ_THREADS of sg_seqpsf_plan.hpp), so --libs names one library per size,
built with `make BUILD=build_abN LIBDIR=lib_abN EXTRA=-DSGQ_THREADS=N`:
  --libs 64=siril-0.9_amd/lib_ab64/libsirilgpu.so,256=siril-0.9_amd/lib/libsirilgpu.so,1024=...
Per library the log records, over `reps` calls after `warmup`, for ORIGINAL framing (one workgroup per frame),
REGISTERED framing (the same kernel, per-frame areas) and FOLLOW_STAR (one workgroup walks the chain):
  device ms          the library's own HIP events around the launch (sg_seqpsf_last_times): median, min, max
  per frame          the median over the frames
  call ms            HIP events on the stream around the whole synchronous call (table upload, record copy)
and, in the same run, what the sequential dependence costs: the chain's median over ORIGINAL's.  The host
comparison is tests/seqpsf_ref.py (the numpy restatement, base variant) on the first `--sample` frames with
the same area; its records must agree with the device's (integers equal, fp within seqpsf_ref.TOL).  The rule
for the default size: a size only if its median is below the others' smallest time."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD = (4096, 480, 640, 40, 420)    # frames, H, W, side, limit (s)


def run_all(out_dir, libs):
    os.makedirs(out_dir, exist_ok=True)
    n, h, w, side, limit = WORKLOAD
    log = os.path.join(out_dir, f"seqpsf_{n}x{h}x{w}.log")
    with open(log, "w") as f:
        for item in libs.split(","):
            threads, path = item.split("=")
            f.write(f"== workgroup of {threads} threads ({path})\n")
            f.flush()
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--frames", str(n),
                   "--height", str(h), "--width", str(w), "--side", str(side)]
            env = dict(os.environ, SG_LIB_PATH=os.path.abspath(path))
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT, env=env).returncode
            print(f"{log}: {threads} threads: exit {rc}", flush=True)
            if rc != 0:     # nothing more is started on the device after a step that failed
                return rc
    return 0


def scene(torch, n, H, W):
    """[n][H][W] int16 (u16 bits) on the device, memory order; the star near the middle"""
    y = torch.arange(H, device="cuda", dtype=torch.float32).view(H, 1)
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, W)
    noise = ((x * 73 + y * 151) % 11) - 5
    frames = torch.empty(n, H, W, dtype=torch.int16, device="cuda")
    c, s = 0.8660254, 0.5
    for f in range(n):
        dx, dy = x - (W * 0.5 + 0.3 + 0.11 * f % 9.0), y - (H * 0.5 - 0.4 + 0.07 * f % 7.0)
        u, v = c * dx + s * dy, -s * dx + c * dy
        star = 20000.0 * torch.exp(-(u * u / 11.0 + v * v / 3.7))
        val = 800 + star + torch.roll(noise, f % 11, 1)
        frames[f] = val.round().clamp(0, 65535).to(torch.int32).to(torch.int16)
    return frames


def run_one(a):
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seqpsf_ref as sr
    import sirilgpu as sg
    N, H, W, S = a.frames, a.height, a.width, a.side
    frames = scene(torch, N, H, W)
    torch.cuda.synchronize()
    area = (W // 2 - S // 2 + 3, H // 2 - S // 2 + 2, S, S)
    rng = np.random.default_rng(5)
    shifts = (rng.integers(-3, 4, size=N).astype(np.int32), rng.integers(-3, 4, size=N).astype(np.int32))
    stream = torch.cuda.Stream()
    print(f"seqpsf: {N} frames of {H} x {W} rendered on the device, area {area}")
    med = {}
    with sg.Context([0]) as ctx:
        for label, kw in (("ORIGINAL", dict(framing=sg.SEQPSF_ORIGINAL)),
                          ("REGISTERED", dict(framing=sg.SEQPSF_REGISTERED, reg_shifts=shifts)),
                          ("FOLLOW_STAR", dict(framing=sg.SEQPSF_FOLLOW_STAR))):
            dev, call, rec = [], [], None
            for it in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc, rec, carry = ctx.seqpsf_device(frames.data_ptr(), N, H, W, area, stream=stream.cuda_stream, **kw)
                e1.record(stream)
                e1.synchronize()
                assert rc == 0, ctx.error()
                if it >= a.warmup:
                    dev.append(ctx.seqpsf_last_times()[0])
                    call.append(e0.elapsed_time(e1))
            m = statistics.median(dev)
            med[label] = (m, min(dev))
            st = np.bincount(rec["status"], minlength=8)
            print(f"{label}: device median of {a.reps}: {m:.3f} ms (min {min(dev):.3f}, max {max(dev):.3f}), "
                  f"{1e3 * m / N:.2f} us per frame; call median {statistics.median(call):.3f} ms (min {min(call):.3f}, "
                  f"max {max(call):.3f}); statuses {st.tolist()}, iterations mean {rec['iters'].mean():.2f} + "
                  f"{rec['iters_angle'].mean():.2f}, carry {carry}")
            if label == "ORIGINAL":
                first = rec
        print(f"the chain against ORIGINAL in this run: {med['FOLLOW_STAR'][0] / med['ORIGINAL'][0]:.1f} x "
              f"({1e3 * med['FOLLOW_STAR'][0] / N:.2f} us against {1e3 * med['ORIGINAL'][0] / N:.2f} us per frame)")
        host = frames[:a.sample].cpu().numpy().view(np.uint16)
        t = time.perf_counter()
        want, _ = sr.seqpsf(host, area)
        dt = time.perf_counter() - t
        ok = True
        for f, w in enumerate(want):
            ok = ok and all(int(first[k][f]) == int(w[k]) for k in sr.INT_FIELDS)
            ok = ok and all(abs(first[k][f] - float(w[k])) <= sr.TOL * max(abs(float(w[k])), 1.0) for k in sr.FIELDS)
        print(f"host restatement (tests/seqpsf_ref.py, numpy) on the first {a.sample} frames: {1e3 * dt / a.sample:.1f} ms per frame, "
              f"{1e3 * dt / a.sample / (med['ORIGINAL'][0] / N):.0f} x the device's ORIGINAL per-frame time; records agree: {ok}")
    return 0 if ok else 1


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--all", action="store_true")
    p.add_argument("--out-dir", default="profiles")
    p.add_argument("--libs", default="256=siril-0.9_amd/lib/libsirilgpu.so")
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--side", type=int, default=40)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sample", type=int, default=8)
    a = p.parse_args()
    return run_all(a.out_dir, a.libs) if a.all else run_one(a)


if __name__ == "__main__":
    sys.exit(main())
