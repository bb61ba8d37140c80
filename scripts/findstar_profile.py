"""Device time of star-candidate detection (sg_findstar_device) on frames resident in HBM.

  python scripts/findstar_profile.py [--frames 64] [--side 4096] [--reps 10] [--warmup 2]
                                     [--radius 10] [--sigma 1.0] [--host-ref] [--kernel-stats DIR]

`frames` mono frames of side^2 of the synthetic star field (sg_synth_fill_device).  The whole call
(statistics, detection plane, peak test, candidate list and boxes back on the host; it is synchronous)
is timed by HIP events on the stream the library is given, after `warmup` calls, median of `reps`,
with and without the boxes, and stated against the traffic model per pixel and frame: 2 B read by the
histogram, 2 B read + 2 B written by the detection plane, 2 B read by the peak test, plus the boxes.

--kernel-stats DIR reads the kernel statistics a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/findstar_profile.py ...`
left in DIR and prints each findstar kernel's time per call and per frame, grouped into the
statistics / plane / peak / gather parts.
--host-ref times tests/findstar_ref.py's vectorised detection plane of one frame on the host: that is
numpy, not the reference program, and is printed for scale only."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARTS = {"k_findstar_hist": "statistics", "k_findstar_stat": "statistics", "k_findstar_plane": "plane",
         "k_findstar_copy": "plane", "k_findstar_peak": "peak", "k_findstar_scan": "peak", "k_findstar_emit": "peak",
         "k_findstar_boxes": "gather"}


def kernel_stats(d, calls, frames, npix):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        print(f"no kernel statistics under {d}")
        return
    parts = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Name"].split("(")[0]
        base = next((k for k in PARTS if k in name), None)
        if base is None:
            continue
        ns = float(row["TotalDurationNs"])
        if PARTS[base] == "gather":
            ns *= 2                     # only the calls with boxes launch it
        print(f"  {base}: {int(row['Calls'])} launches, {ns / calls / 1e6:.3f} ms per call, "
              f"{ns / calls / frames / 1e3:.2f} us per frame")
        parts[PARTS[base]] = parts.get(PARTS[base], 0.0) + ns
    model = {"statistics": 2, "plane": 4, "peak": 2}
    for part, ns in parts.items():
        line = f"{part}: {ns / calls / 1e6:.3f} ms per call, {ns / calls / frames / 1e3:.2f} us per frame"
        if part in model:
            line += f", {model[part] * npix * frames / (ns / calls):.0f} GB/s of its {model[part]} B per pixel and frame"
        print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--max-candidates", type=int, default=2000)
    ap.add_argument("--host-ref", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    N, S = a.frames, a.side
    npix = S * S
    if a.kernel_stats:
        # the traced run makes 2 * (warmup + reps) calls: with and without the boxes
        kernel_stats(a.kernel_stats, 2 * (a.warmup + a.reps), N, npix)
        return
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    import sirilgpu as sg
    frames = torch.empty(N * npix, dtype=torch.int16, device="cuda")
    wave = torch.empty(N * npix, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    with sg.Context([0]) as ctx:
        ctx.synth_fill(frames.data_ptr(), N, 1, S, S, 0, S, 7, 6)
        torch.cuda.synchronize()

        def timed(label, boxes):
            ms, rec = [], None
            for r in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc, rec, xy, bx = ctx.findstar_device(frames.data_ptr(), N, 1, S, S, a.radius, a.sigma,
                                                      max_candidates=a.max_candidates, want_boxes=boxes,
                                                      d_wave=wave.data_ptr(), stream=stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize()
                if rc != 0:
                    raise RuntimeError(f"{label}: rc {rc}: {ctx.error()}")
                if r >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            stored = sum(q.nstored for q in rec)
            gb = (8 * npix * N + (stored * 4 * a.radius * a.radius * 4 if boxes else 0)) / 1e9
            print(f"{label}: {N} x {S}^2, r = {a.radius}, k = {a.sigma}, median of {a.reps}: {med:.3f} ms per call, "
                  f"{med / N * 1e3:.1f} us per frame (min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
            print(f"  model 8 B/pixel/frame{' + boxes' if boxes else ''} = {gb:.3f} GB: {gb / med * 1e3:.0f} GB/s for the whole "
                  f"call (its host steps and three synchronises included)", flush=True)
            return rec

        rec = timed("findstar with boxes", True)
        timed("findstar without boxes", False)
        nc = [q.ncand for q in rec]
        print(f"  candidates per frame: min {min(nc)}, median {statistics.median(nc)}, max {max(nc)}; frame 0: threshold "
              f"{rec[0].threshold}, median {rec[0].median}, sigma {rec[0].sigma:.3f}, flags wavelet {rec[0].wavelet_applied} "
              f"ratio {rec[0].ratio_applied} host-sigma {rec[0].sigma_on_host} wrapped {rec[0].threshold_wrapped}", flush=True)
        if a.host_ref:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import findstar_ref as fr
            f0 = frames[:npix].cpu().numpy().view(np.uint16).reshape(S, S)
            t0 = time.perf_counter()
            want = fr.detection_plane(f0)[0]
            dt = time.perf_counter() - t0
            got = wave[:npix].cpu().numpy().view(np.uint16).reshape(S, S)
            print(f"host numpy restatement (tests/findstar_ref.py, not the reference program), detection plane of one "
                  f"{S}^2 frame: {dt:.2f} s; the device plane of frame 0 is "
                  + ("equal" if np.array_equal(got, want) else "DIFFERENT"), flush=True)
            cands, want_rec, _ = fr.candidates(f0, a.sigma, a.radius)
            print(f"  frame 0 candidates: device {rec[0].ncand}, restatement {len(cands)}; threshold {rec[0].threshold} / "
                  f"{want_rec['threshold']}", flush=True)


if __name__ == "__main__":
    main()
