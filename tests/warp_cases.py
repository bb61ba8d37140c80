"""Shared cases of the sequence warp's tests (test_warp_plan_cpu.py, test_gpu_warp_frames.py): the
homographies the footprint bound is tried against, for a W x H source, and the source frames."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "siril-0.9_amd", "csrc")
W, H = 96, 80                      # source frames
OUT_SIZES = [(150, 40), (150, 9), (64, 16), (65, 17), (1, 1)]      # (out_width, out_height); 150 x 9 has bw = 113
HORIZON_X = 75.0                   # where the horizon case's denominator changes sign


def rotation(deg, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0, scale=1.0):
    a = np.deg2rad(deg)
    c, s = np.cos(a) * scale, np.sin(a) * scale
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]])


def translation(dx, dy):
    return np.array([[1.0, 0, dx], [0, 1.0, dy], [0, 0, 1.0]])


def horizon():
    """the inverse map's denominator is 1 - x / HORIZON_X: it crosses 0 inside a 150-wide destination"""
    M = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0 / HORIZON_X, 0, 1.0]])
    return np.linalg.inv(M)


HOMS = {
    "identity": np.eye(3),
    "shift_int": translation(7.0, -4.0),
    "shift_frac": translation(-3.37, 5.81),
    "rot0_5": rotation(0.5),
    "rot5": rotation(5.0),
    "rot45": rotation(45.0),
    "rot90": rotation(90.0),
    "rot180": rotation(180.0),
    "scale0_8": rotation(0.0, scale=0.8),
    "scale1_25": rotation(0.0, scale=1.25),
    "perspective": np.array([[1.01, 0.02, 1.5], [-0.015, 0.99, -2.25], [1e-5, -1.2e-5, 1.0]]),
    "horizon": horizon(),
    "singular": np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, 0.25, 1.0]]),
}
REGULAR = [k for k in HOMS if k not in ("horizon", "singular")]


def frames(n, C, h=H, w=W, seed=3):
    """n frames that differ from one another: a smooth field, noise and a few bright points each"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((n, C, h, w), dtype=np.uint16)
    for f in range(n):
        for c in range(C):
            v = 9000 + 6000 * np.sin(x * (0.11 + 0.02 * f) + c) * np.cos(y * (0.07 + 0.01 * c) - f) + rng.normal(0, 700, (h, w))
            for _ in range(12):
                v[rng.integers(0, h), rng.integers(0, w)] = rng.integers(30000, 65536)
            out[f, c] = np.clip(np.rint(v), 0, 65535).astype(np.uint16)
    return out
