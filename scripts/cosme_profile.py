"""Device time of the automatic cosmetic correction (sg_cosme_autodetect_device) on frames resident in HBM.

  python scripts/cosme_profile.py [--frames 64] [--side 4096] [--reps 5] [--warmup 1] [--sig 3 3] [--amount 1]
  python scripts/cosme_profile.py --kernel-stats DIR [--frames ..] [--reps ..] [--warmup ..]

`frames` synthetic mono frames of side^2 (sg_synth_fill_device) are corrected in place, plain and CFA,
after a fresh copy of the pristine frames per call.  Each call is timed by HIP events on the stream the
library is given (median of `reps` after `warmup`); the library's own event spans split it into the
statistics (histogram + finish), the main pass and the dependence resolution (rounds + commit, with
the host's looks at the active count).  Printed too: the corrected pixels, the rounds, the pixels the
rounds re-examined, and the achieved GB/s against the byte model of 4 B per pixel and layer (2 read for
the statistics, 2 for the scan).
--kernel-stats reads the *kernel_stats.csv a
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/cosme_profile.py ...`
left in DIR and prints each kernel's time per call; the traced run makes 2 * (warmup + reps) calls."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ["k_cosme_hist", "k_cosme_stat", "k_cosme_main", "k_cosme_round", "k_cosme_commit"]


def kernel_stats(d, calls, frames, npix):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        print(f"no kernel statistics under {d}")
        return
    total = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Name"].split("(")[0]
        base = next((k for k in KERNELS if k in name), None)
        if base is None:
            continue
        total[base] = total.get(base, 0.0) + float(row["TotalDurationNs"])
        print(f"  {base}: {int(row['Calls'])} launches, {float(row['TotalDurationNs']) / calls / 1e6:.3f} ms per call")
    all_ns = sum(total.values())
    for k in KERNELS:
        if k in total:
            print(f"{k}: {total[k] / calls / 1e6:.3f} ms per call (plain and CFA averaged), {100 * total[k] / all_ns:.1f} % of the kernels")
    if "k_cosme_main" in total:
        print(f"k_cosme_main: {2 * npix * frames / (total['k_cosme_main'] / calls):.0f} GB/s of its 2 B per pixel")
    if "k_cosme_hist" in total:
        print(f"k_cosme_hist: {2 * npix * frames / (total['k_cosme_hist'] / calls):.0f} GB/s of its 2 B per pixel")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sig", type=float, nargs=2, default=(3.0, 3.0))
    ap.add_argument("--amount", type=float, default=1.0)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    N, S = a.frames, a.side
    npix = S * S
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, 2 * (a.warmup + a.reps), N, npix)
        return
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    import sirilgpu as sg
    pristine = torch.empty(N * npix, dtype=torch.int16, device="cuda")
    work = torch.empty_like(pristine)
    stream = torch.cuda.Stream()
    with sg.Context([0]) as ctx:
        ctx.synth_fill(pristine.data_ptr(), N, 1, S, S, 0, S, 7, 0)
        torch.cuda.synchronize()
        for is_cfa in (False, True):
            label = "CFA" if is_cfa else "plain"
            ms, parts, rec = [], [], None
            for r in range(a.warmup + a.reps):
                work.copy_(pristine)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc, rec = ctx.cosme_autodetect_device(work.data_ptr(), N, 1, S, S, sig=tuple(a.sig), amount=a.amount,
                                                      is_cfa=is_cfa, stream=stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize()
                if rc != 0:
                    raise RuntimeError(f"{label}: rc {rc}: {ctx.error()}")
                if r >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
                    parts.append(ctx.cosme_last_times())
            med = statistics.median(ms)
            st, mn, rs = (statistics.median(p[i] for p in parts) for i in range(3))
            rounds, reex = parts[-1][3], parts[-1][4]
            cold, hot = sum(x.icold for x in rec), sum(x.ihot for x in rec)
            print(f"{label}: {N} x {S}^2, sig {tuple(a.sig)}, amount {a.amount}: median of {a.reps}: {med:.3f} ms per call, "
                  f"{med / N * 1e3:.1f} us per frame (min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
            print(f"  statistics {st:.3f} ms, main pass {mn:.3f} ms, dependence resolution {rs:.3f} ms "
                  f"({100 * rs / (st + mn + rs):.1f} % of the three)", flush=True)
            print(f"  corrected {cold} cold + {hot} hot = {100.0 * (cold + hot) / (N * npix):.4f} % of the pixels; "
                  f"{rounds} rounds re-examined {reex} pixels ({100.0 * reex / (N * npix):.4f} %)", flush=True)
            print(f"  byte model 4 B/pixel = {4 * npix * N / 1e9:.3f} GB: {4 * npix * N / med / 1e6:.0f} GB/s over the call; "
                  f"statistics {2 * npix * N / st / 1e6:.0f} GB/s, main pass {2 * npix * N / mn / 1e6:.0f} GB/s of 2 B/pixel each; "
                  f"bkg {rec[0].bkg[0]:.0f}, avgDev {rec[0].avg_dev[0]:.3f}", flush=True)


if __name__ == "__main__":
    main()
