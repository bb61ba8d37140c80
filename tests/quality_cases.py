"""Scenes, shapes and content cases of the quality estimate tests (sg_quality_u16*): no random
numbers, so nothing here depends on a numpy version.  The expectations come from
oracle_lib.quality at run time; the literals below only show that the generator was reproduced."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "siril-0.9_amd", "csrc")


def planet(H, W, seed, ped=20, amp=230):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rad = min(H, W) * 0.3
    r = np.hypot(x - (W * 0.5 + 0.3), y - (H * 0.5 - 0.4))
    disk = 1.0 / (1.0 + np.exp(r - rad))
    tex = 0.25 * np.sin(x * 0.9 + seed) * np.cos(y * 0.7)
    noise = ((x * 73 + y * 151 + seed * 31) % 7) - 3
    return np.clip(np.rint(ped + amp * disk * (0.75 + tex) + noise), 0, 65535).astype(np.uint16)


GENERATOR_CHECKS = [((48, 64, 1), {}, 3209.637656297393), ((10, 10, 1), {}, 13148.079707698764),
                    ((480, 640, 1), {}, 1401.5104883112683), ((48, 64, 2), {"amp": 58880}, 3635.591245003523)]


def constant(name):
    """an integer #define of sg_quality.h / sg_quality_plan.hpp"""
    for fn in ("sg_quality.h", "sg_quality_plan.hpp"):
        m = re.search(r"^#define\s+%s\s+\(?(\d+)" % name, open(os.path.join(CSRC, fn)).read(), re.M)
        if m:
            return int(m.group(1))
    raise KeyError(name)


TILE_X, TILE_Y = constant("SGQ_TILE_X"), constant("SGQ_TILE_Y")


def side(samples):
    """the smallest side with that many samples: (side - 1) // 3 == samples"""
    return 3 * samples + 1


# (H, W)
SHAPES_ZERO = [(6, 20), (20, 6)]                 # xs < 2 or ys < 2: 0.0, no launch
SHAPES_NAN = [(7, 7), (9, 10)]                   # the margins leave no row
SHAPES = [(10, 10), (10, 13), (13, 10), (16, 19), (17, 21), (18, 20), (24, 32), (31, 47), (37, 61), (48, 64), (97, 131),
          (190, 193), (193, 196), (196, 199)]
# one sample fewer and one more than each tile dimension of the tiled route, both ways
SHAPES_TILE = sorted({s for t in (TILE_X - 1, TILE_X + 1) for s in ((40, side(t)), (side(t), 40))} |
                     {s for t in (TILE_Y - 1, TILE_Y + 1) for s in ((side(t), 100), (100, side(t)))})
SHAPE_BIG = (480, 640)


def shape_frames(H, W):
    """the two scenes every shape is tested with"""
    return np.stack([planet(H, W, 1), planet(H, W, 2, amp=58880)])


def _block(sy, sx):
    a = np.full((48, 64), 10, dtype=np.uint16)
    a[3 * sy:3 * sy + 6, 3 * sx:3 * sx + 6] = 200
    return a


def _rect():
    a = np.full((48, 64), 65534, dtype=np.uint16)
    a[10:30, 10:40] = 65000
    return a


def _clamp():
    a = planet(48, 64, 5)
    a[:3] = 60000
    a[-5:] = 60000
    return a


BLOCKS = {(6, 9): 3166.600002368471, (1, 2): 3166.600002368471, (12, 17): 3166.600002368471, (1, 9): 3166.600002368471,
          (6, 2): 3166.600002368471, (6, 17): 3166.600002368471, (2, 3): 3102.6325768074225, (11, 16): 3799.9777806367943,
          (0, 1): float("nan"), (0, 0): float("nan"), (13, 18): float("nan")}

# name -> (frame, the value the issue quotes for it or None)
CONTENT = {
    "zero": (np.zeros((48, 64), dtype=np.uint16), float("nan")),
    "const20": (np.full((48, 64), 20, dtype=np.uint16), 0.0),
    "const65535": (np.full((48, 64), 65535, dtype=np.uint16), 0.0),
    "rect": (_rect(), 32.78764549292457),
    "clamp": (_clamp(), 3325.1434158711277),
    "noclamp": (planet(48, 64, 5), 3229.7660908166226),
}
for (_sy, _sx), _v in BLOCKS.items():
    CONTENT["block_%d_%d" % (_sy, _sx)] = (_block(_sy, _sx), _v)


def same(a, b):
    """exact equality of doubles, NaN matching NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
