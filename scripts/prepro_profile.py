"""Device time of sequence preprocessing (sg_prepro_frames_device) on frames resident in HBM.

  python scripts/prepro_profile.py [--frames 64] [--side 4096] [--reps 10] [--warmup 2] [--check]

Three regimes on `frames` mono frames of side^2, each timed by HIP events on the stream the
library is given, after `warmup` calls, median of `reps`:
  calibrate           offset + dark + flat (k_prepro_calibrate alone)
  calibrate+cosmetic  the same with a 0.1 % deviant list that includes one full hot column
  dark fit            dark optimization: 13 golden-section iterations of k_prepro_noise over the
                      batch (host median and bookkeeping between them included), then the calibration
The calibrate line states the achieved GB/s against the kernel's 4 B per pixel and frame (2 read,
2 written; the masters are read once per batch).  --check compares frame 0's fitted k with
tests/prepro_ref.py (slow: Python rows)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    import sirilgpu as sg
    N, S = a.frames, a.side
    npix = S * S
    g = torch.Generator(device="cuda").manual_seed(1)
    # thermal signal (gamma(2, 150) as a sum of two exponentials) with 1 % hot pixels; dark = T + N(0, 3);
    # frame f = 500 + k_f T + N(0, 12) with 2 % zeros, k_f spread over [0.6, 1.4]
    T = -150.0 * (torch.log(torch.rand(npix, device="cuda", generator=g).clamp_min(1e-9))
                  + torch.log(torch.rand(npix, device="cuda", generator=g).clamp_min(1e-9)))
    hot = torch.rand(npix, device="cuda", generator=g) < 0.01
    T = T + hot * (3000 + 17000 * torch.rand(npix, device="cuda", generator=g))

    def u16(x):
        return x.round().clamp(0, 32767).to(torch.int16)

    dark = u16(T + 3 * torch.randn(npix, device="cuda", generator=g))
    k_true = np.linspace(0.6, 1.4, N)
    pristine = torch.empty(N * npix, dtype=torch.int16, device="cuda")
    for f in range(N):
        fr = u16(500 + float(k_true[f]) * T + 12 * torch.randn(npix, device="cuda", generator=g))
        fr[torch.rand(npix, device="cuda", generator=g) < 0.02] = 0
        pristine[f * npix:(f + 1) * npix] = fr
    del T, hot
    work = torch.empty_like(pristine)
    dark_h = dark.cpu().numpy().view(np.uint16).reshape(1, S, S)
    rng = np.random.default_rng(2)
    off_h = rng.integers(90, 110, size=(1, S, S)).astype(np.uint16)
    flat_h = rng.normal(30000, 2000, size=(1, S, S)).clip(1, 65535).astype(np.uint16)
    # cosmetic regime: a quiet dark with 0.1 % hot pixels and one full hot column
    cdark_h = rng.normal(400, 6, size=(1, S, S)).clip(1, 65535).astype(np.uint16)
    cdark_h[0][rng.random((S, S)) < 0.001 - 1.0 / S] = 60000
    cdark_h[0, :, S // 3] = 60000
    stream = torch.cuda.Stream()

    def timed(ctx, pp, label):
        ms, ks = [], None
        for r in range(a.warmup + a.reps):
            work.copy_(pristine)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc, ks = ctx.prepro_frames_device(pp, work.data_ptr(), N, stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError(f"{label}: rc {rc}: {ctx.error()}")
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        print(f"{label}: {N} x {S}^2, median of {a.reps}: {med:.3f} ms per call, {med / N * 1e3:.1f} us per frame "
              f"(min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
        return med, ks

    with sg.Context([0]) as ctx:
        with sg.Prepro(ctx, S, S, 1, offset=off_h, dark=dark_h, flat=flat_h, autolevel=True) as pp:
            med, _ = timed(ctx, pp, "calibrate (offset, dark, flat)")
            print(f"  k_prepro_calibrate model 4 B/pixel/frame = {4 * npix * N / 1e9:.3f} GB: {4 * npix * N / med / 1e6:.0f} GB/s "
                  f"(the call: one launch and its synchronise)", flush=True)
        with sg.Prepro(ctx, S, S, 1, offset=off_h, dark=cdark_h, flat=flat_h, autolevel=True, cosmetic=True,
                       cosme_sigma=(-1.0, 3.0)) as pp:
            i = pp.info()
            print(f"cosmetic list: {i.ihot} hot + {i.icold} cold = {100.0 * (i.ihot + i.icold) / npix:.3f} % of the pixels, "
                  f"{i.components} components, the longest {i.longest_component}", flush=True)
            timed(ctx, pp, "calibrate + cosmetic")
        with sg.Prepro(ctx, S, S, 1, offset=off_h, dark=dark_h, flat=flat_h, autolevel=True, dark_optimization=True) as pp:
            med, ks = timed(ctx, pp, "dark fit + calibrate")
            err = np.abs(ks - k_true)
            print(f"  fitted k: max |k - k_true| = {err.max():.4f}; the fit costs {med / N:.3f} ms per frame", flush=True)
            if a.check:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import prepro_ref as pr
                f0 = pristine[:npix].cpu().numpy().view(np.uint16).reshape(S, S)
                k_ref, it = pr.search_rule(lambda k: pr.objective(f0, dark_h[0], k))
                print(f"  frame 0: k = {ks[0]!r}, reference {k_ref!r} ({it} iterations): "
                      + ("equal" if ks[0] == k_ref else "DIFFERENT"), flush=True)


if __name__ == "__main__":
    main()
