"""Device time of the CFA demosaicing kernels against the host-to-device copy of their batch.

  rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o run -- \
      python scripts/debayer_profile.py run [--frames 64] [--side 2048] [--loads 12]
  python scripts/debayer_profile.py report DIR [--warmup 2]

`run` writes a 16-bit CFA SER of random samples to $TMPDIR, reads it once (page cache) and
loads it `loads` times with sg_seq_load_device under each interpolation (bilinear, nearest
neighbour, VNG).  `report` reads the traces: per kernel the median dispatch time without the
first `warmup` loads, per frame, with its register and LDS use, and the median time of the
batches' host-to-device copies (the copies of at least half the largest size seen)."""
import argparse
import csv
import glob
import os
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_debayer_frames", "k_debayer_nn", "k_debayer_vng"]


def run(a):
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "siril-0.9_amd", "python"))
    import sirilgpu as sg
    N, S = a.frames, a.side
    path = os.path.join(tempfile.gettempdir(), f"debayer_profile_{os.getpid()}.ser")
    hdr = bytearray(178)
    hdr[0:14] = b"LUCAM-RECORDER"
    struct.pack_into("<7i", hdr, 14, 0, 8, 0, S, S, 16, N)       # ColorID 8 = RGGB, little-endian
    rng = np.random.default_rng(1)
    try:
        with open(path, "wb") as f:
            f.write(hdr)
            for _ in range(N):
                f.write(rng.integers(0, 65536, size=S * S, dtype=np.uint16).tobytes())
            f.write(b"\0" * 8 * N)
        with open(path, "rb") as f:
            while f.read(1 << 26):
                pass
        d = torch.zeros(N * 3 * S * S, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        with sg.Context([0]) as ctx, sg.Seq.open_ser(path) as seq:
            for name, inter in [("bilinear", sg.BAYER_INTER_BILINEAR), ("nearest", sg.BAYER_INTER_NEARESTNEIGHBOR),
                                ("vng", sg.BAYER_INTER_VNG)]:
                seq.set_debayer(-1, inter)
                ms = []
                for _ in range(a.loads):
                    t0 = time.perf_counter()
                    ctx.load_seq_device(seq, d.data_ptr())
                    ms.append((time.perf_counter() - t0) * 1e3)
                print(f"{name}: load of {N} x {S}^2 from the page cache, ms per load: "
                      + " ".join(f"{v:.1f}" for v in ms), flush=True)
    finally:
        if os.path.exists(path):
            os.unlink(path)


def rows(d, suffix):
    out = []
    for p in glob.glob(os.path.join(d, "**", f"*{suffix}.csv"), recursive=True):
        with open(p, newline="") as f:
            out += list(csv.DictReader(f))
    return out


def report(a):
    kt = rows(a.dir, "kernel_trace")
    for k in KERNELS:
        r = [x for x in kt if x["Kernel_Name"].split("(")[0].split("<")[0].split()[-1] == k]
        if not r:
            continue
        r.sort(key=lambda x: int(x["Start_Timestamp"]))
        # frames of a dispatch: the grid's y (one thread per pixel) or z (tiles) extent
        fr = [int(x["Grid_Size_Z"]) if k == "k_debayer_vng" else int(x["Grid_Size_Y"]) for x in r]
        per_load = len(r) // a.loads
        r, fr = r[a.warmup * per_load:], fr[a.warmup * per_load:]
        us = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 / n for x, n in zip(r, fr)]
        print(f"{k}: {len(r)} dispatches of {fr[0]} frames, median {statistics.median(us):.1f} us per frame "
              f"(min {min(us):.1f}, max {max(us):.1f}); VGPRs {r[0]['VGPR_Count']}, LDS {r[0]['LDS_Block_Size']} B")
    mc = [x for x in rows(a.dir, "memory_copy_trace") if "HOST_TO_DEVICE" in x.get("Direction", "").upper()]
    dur = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in mc]
    if dur and "Bytes" in mc[0]:
        size = [int(x["Bytes"]) for x in mc]
        big = [t for t, b in zip(dur, size) if 2 * b >= max(size)]
        print(f"host-to-device copies of >= {max(size) // 2} B: {len(big)}, median {statistics.median(big):.1f} us "
              f"for {max(size)} B ({max(size) / statistics.median(big) / 1e3:.1f} GB/s)")
    elif dur:
        big = [t for t in dur if 2 * t >= max(dur)]
        print(f"host-to-device copies (the long ones): {len(big)}, median {statistics.median(big):.1f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("run")
    p.add_argument("--frames", type=int, default=64)
    p.add_argument("--side", type=int, default=2048)
    p.add_argument("--loads", type=int, default=12)
    p = sub.add_parser("report")
    p.add_argument("dir")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--loads", type=int, default=12)
    a = ap.parse_args()
    run(a) if a.cmd == "run" else report(a)
