"""numpy / plain-Python restatement of the automatic cosmetic correction (include/sirilgpu.h,
sg_cosme_autodetect*): autoDetect (src/algos/cosmetic_correction.c:384-435) as
cosmetic_image_hook (:297-313) applies it to every layer of a frame.

Two forms:
  autodetect_literal  the reference loop line by line: statistics() (src/algos/statistics.c:207-326)
                      for bkg and avgDev, then for every pixel getAverage3x3 (:102-126) and
                      getMedian5x5 (:34-67) of the buffer as it stands, the hot and the cold test,
                      the in-place store;
  autodetect_rule     the form the kernels implement (siril-0.9_amd/csrc/sg_cosme.h, sg_cosme.hip):
                      integer thresholds per layer, a lazy median behind a counting bound, one pass
                      against the original image, then rounds over the active pixels until the
                      serial result (the unique fixed point) is reached.
Frames are [C][H][W] uint16 in memory order; index 0 is the first pixel of the scan.
"""
import math

import numpy as np

import prepro_ref as pr

NONE, HOT, COLD = 0, 1, 2


# ---------------------------------------------------------------------------- statistics

def statistics(plane):
    """(ngood, bkg, avgDev) of statistics(fit, layer, NULL, STATS_BASIC | STATS_AVGDEV,
    STATS_ZERO_NULLCHECK), None when no pixel is non-zero (:247-250)"""
    g = np.asarray(plane).reshape(-1)
    nz = g[g != 0]
    ngood = int(nz.size)
    if ngood == 0:
        return None
    bkg = pr.hist_median(g, ngood)                              # siril_stats_ushort_median (:255)
    s = 0.0
    s = float(np.abs(nz.astype(np.float64) - bkg).sum())        # integers below 2^53: the order is free
    return ngood, bkg, s / ngood                                # gsl_stats_ushort_absdev_m (:267)


def statistics_hist(plane):
    """the kernels' route to the same three numbers: everything from the 65536-bin histogram"""
    h = np.bincount(np.asarray(plane).reshape(-1), minlength=65536).astype(np.int64)
    ngood = int(h[1:].sum())
    if ngood == 0:
        return None
    run = np.cumsum(h[1:65535])
    over = np.nonzero(2 * run > ngood)[0]
    med = int(over[0]) + 1 if over.size else 0
    sumabs = int((h[1:] * np.abs(np.arange(1, 65536, dtype=np.int64) - med)).sum())
    return ngood, float(med), float(sumabs) / float(ngood)


# ---------------------------------------------------------------------------- the literal loop

def _window(get, W, H, xx, yy, radius, step):
    out = []
    for y in range(yy - radius, yy + radius + 1, step):
        for x in range(xx - radius, xx + radius + 1, step):
            if 0 <= y < H and 0 <= x < W and (x != xx or y != yy):
                out.append(get(x, y))
    return out


def average3x3(get, W, H, x, y, is_cfa):
    """getAverage3x3 (:102-126); without any neighbour the reference converts 0 / 0: taken as 0"""
    step = 2 if is_cfa else 1
    return pr.average3x3(_window(get, W, H, x, y, step, step))


def median5x5(get, W, H, x, y, is_cfa, median=pr.median24_literal):
    """getMedian5x5 (:34-67), start = 24 - n - 1 included"""
    step = 2 if is_cfa else 1
    return median(_window(get, W, H, x, y, 2 * step, step))


def autodetect_layer_literal(buf, sig, amount, is_cfa):
    """autoDetect (:384-435) on one layer, a list of rows of ints changed in place;
    returns None (return 1) or (icold, ihot, bkg, avgDev)"""
    H, W = len(buf), len(buf[0])
    st = statistics(np.array(buf, dtype=np.uint16))
    if st is None:
        return None
    _, bkg, avgDev = st
    f0 = amount
    f1 = 1 - f0
    icold = ihot = 0
    get = lambda x, y: buf[y][x]
    for y in range(H):
        for x in range(W):
            pixel = buf[y][x]
            a = average3x3(get, W, H, x, y, is_cfa)
            m = median5x5(get, W, H, x, y, is_cfa)
            if sig[1] != -1.0:
                k1 = avgDev
                k2 = k1 / 2
                k3 = sig[1] * k1
                if (a < bkg + k2) and (pixel > bkg + k1) and (pixel > m + k3):
                    ihot += 1
                    buf[y][x] = int(a * f0 + pixel * f1)
            if sig[0] != -1.0:
                k = avgDev * sig[0]
                if ((pixel + k) < bkg) and ((pixel + k) < m):
                    icold += 1
                    buf[y][x] = int(m * f0 + pixel * f1)
    return icold, ihot, bkg, avgDev


def _result():
    return {"status": 0, "failed_layer": -1, "icold": 0, "ihot": 0, "bkg": [0.0] * 3, "avg_dev": [0.0] * 3}


def autodetect_literal(frame, sig, amount, is_cfa):
    """cosmetic_image_hook (:297-313): the layers in turn, the first failure ends the frame.
    Returns (corrected frame, result dict)"""
    out = np.array(frame, dtype=np.uint16)
    res = _result()
    for c in range(out.shape[0]):
        buf = out[c].tolist()
        r = autodetect_layer_literal(buf, sig, float(amount), is_cfa)
        if r is None:
            res["status"], res["failed_layer"] = 1, c
            break
        out[c] = np.array(buf, dtype=np.uint16)
        res["icold"] += r[0]
        res["ihot"] += r[1]
        res["bkg"][c], res["avg_dev"][c] = r[2], r[3]
    return out, res


# ---------------------------------------------------------------------------- the kernels' form

class Rule:
    """sgc_rule_make: the layer's integer thresholds"""

    def __init__(self, ngood, bkg, avg_dev, sig, amount, is_cfa):
        self.bkg, self.avg_dev = bkg, avg_dev
        self.f0 = amount
        self.f1 = 1 - amount
        self.step = 2 if is_cfa else 1
        self.hot_min, self.a_max, self.cold_max, self.k3, self.kc = 65536, -1, -1, 0.0, 0.0
        if sig[1] != -1.0:
            k1 = avg_dev
            k2 = k1 / 2
            self.k3 = sig[1] * k1
            t1, t2 = bkg + k1, bkg + k2
            self.hot_min = 65536 if t1 >= 65535.0 else int(math.floor(t1)) + 1
            self.a_max = min(int(math.ceil(t2)) - 1, 65535)
        if sig[0] != -1.0:
            k = avg_dev * sig[0]
            self.kc = k
            lo, hi = -1, 65535
            while lo < hi:
                mid = lo + (hi - lo + 1) // 2
                if (mid + k) < bkg:
                    lo = mid
                else:
                    hi = mid - 1
            self.cold_max = lo

    def own(self, pixel):
        return HOT if pixel >= self.hot_min else (COLD if pixel <= self.cold_max else NONE)


def _average_rule(vals):
    """sgc_average: the integer sum; (sum + 4) >> 3 with all 8 neighbours"""
    if len(vals) == 8:
        return (sum(vals) + 4) >> 3
    return pr.rtw(float(sum(vals)) / len(vals)) if vals else 0


def _hot_maybe(vals, r, pixel):
    """sgc_hot_maybe: at least r0 + 1 neighbours not above floor(pixel - k3) + 2"""
    lim = math.floor(pixel - r.k3) + 2.0
    if lim < 0.0:
        return False
    vmax = 65535 if lim > 65535.0 else int(lim)
    return sum(1 for v in vals if v <= vmax) >= (len(vals) - 1) // 2


def _decide(get, W, H, x, y, r, pixel, own, stats):
    """sgc_decide behind sgc_hot_maybe: (kind, value)"""
    if own == HOT:
        a = _average_rule(_window(get, W, H, x, y, r.step, r.step))
        if a > r.a_max:
            return NONE, pixel
        vals = _window(get, W, H, x, y, 2 * r.step, r.step)
        if not _hot_maybe(vals, r, pixel):
            return NONE, pixel
        stats["medians"] += 1
        m = pr.median24_rule(vals)
        if not (pixel > m + r.k3):
            return NONE, pixel
        return HOT, int(a * r.f0 + pixel * r.f1)
    if own == COLD:
        stats["medians"] += 1
        m = pr.median24_rule(_window(get, W, H, x, y, 2 * r.step, r.step))
        if not ((pixel + r.kc) < m):
            return NONE, pixel
        return COLD, int(m * r.f0 + pixel * r.f1)
    return NONE, pixel


def _later(x, y, W, H, step):
    """the pixels after (x, y) in scan order that have it in their 5x5 window (sgc_later)"""
    for i in range(13, 25):
        xx, yy = x + (i % 5 - 2) * step, y + (i // 5 - 2) * step
        if 0 <= yy < H and 0 <= xx < W:
            yield xx, yy


def autodetect_layer_rule(plane, sig, amount, is_cfa, max_rounds=None):
    """one layer the kernels' way; returns None or (corrected plane, icold, ihot, bkg, avgDev, info);
    info: rounds, re-examined pixels, medians sorted, the one-pass counts"""
    plane = np.asarray(plane, dtype=np.uint16)
    H, W = plane.shape
    st = statistics_hist(plane)
    if st is None:
        return None
    ngood, bkg, avg_dev = st
    r = Rule(ngood, bkg, avg_dev, sig, float(amount), is_cfa)
    orig = plane.tolist()
    state = {}                                   # scan position -> (kind, value)
    stats = {"medians": 0}
    info = {"rounds": 0, "reexamined": 0}
    active = set()
    # the main pass: every pixel against the original image
    cand = np.nonzero((plane >= r.hot_min) | (plane.astype(np.int64) <= r.cold_max))
    get0 = lambda x, y: orig[y][x]
    for y, x in zip(cand[0].tolist(), cand[1].tolist()):
        pixel = orig[y][x]
        kind, val = _decide(get0, W, H, x, y, r, pixel, r.own(pixel), stats)
        if kind != NONE:
            state[y * W + x] = (kind, val)
            if val != pixel:
                active.update(yy * W + xx for xx, yy in _later(x, y, W, H, r.step) if r.own(orig[yy][xx]) != NONE)
    info["one_pass"] = (sum(1 for k, _ in state.values() if k == COLD), sum(1 for k, _ in state.values() if k == HOT))
    info["one_pass_plane"] = plane.copy()
    for p, (_, v) in state.items():
        info["one_pass_plane"][p // W, p % W] = v
    # the rounds: a listed pixel reads corrected values before it, original ones after it
    while active and (max_rounds is None or info["rounds"] < max_rounds):
        info["rounds"] += 1
        info["reexamined"] += len(active)
        nxt = set()
        snapshot = dict(state)                   # every pixel of a round may read the round's start
        for p in sorted(active):
            y, x = divmod(p, W)
            pixel = orig[y][x]

            def get(xx, yy, p=p):
                q = yy * W + xx
                return snapshot[q][1] if q < p and q in snapshot else orig[yy][xx]
            kind, val = _decide(get, W, H, x, y, r, pixel, r.own(pixel), stats)
            old = state.get(p, (NONE, pixel))
            if (kind, val) == old:
                continue
            if kind == NONE:
                state.pop(p, None)
            else:
                state[p] = (kind, val)
            nxt.update(yy * W + xx for xx, yy in _later(x, y, W, H, r.step) if r.own(orig[yy][xx]) != NONE)
        active = nxt
    out = plane.copy()
    for p, (_, v) in state.items():
        out[p // W, p % W] = v
    info["medians"] = stats["medians"]
    icold = sum(1 for k, _ in state.values() if k == COLD)
    ihot = sum(1 for k, _ in state.values() if k == HOT)
    return out, icold, ihot, bkg, avg_dev, info


def autodetect_rule(frame, sig, amount, is_cfa):
    """the whole frame the kernels' way: (corrected frame, result dict, per-layer info)"""
    out = np.array(frame, dtype=np.uint16)
    res, infos = _result(), []
    for c in range(out.shape[0]):
        r = autodetect_layer_rule(out[c], sig, amount, is_cfa)
        if r is None:
            res["status"], res["failed_layer"] = 1, c
            break
        out[c] = r[0]
        res["icold"] += r[1]
        res["ihot"] += r[2]
        res["bkg"][c], res["avg_dev"][c] = r[3], r[4]
        infos.append(r[5])
    return out, res, infos


# ---------------------------------------------------------------------------- seeded frames

def noise_plane(H, W, seed, level=1000, spread=30):
    rng = np.random.default_rng(seed)
    return rng.integers(level - spread, level + spread + 1, size=(H, W)).astype(np.uint16)


def run_level(plane):
    """bkg + int(3 avgDev): between 4 and 8 half-deviations, so a pixel of a run is hot while one
    of its 3x3 neighbours is at the run's level and not while two are"""
    _, bkg, avg = statistics(plane)
    return int(bkg) + int(3 * avg)


def chain_plane(H, W, seed, runs, share=0.1, clear=5):
    """runs [(kind, x, y, length)] at run_level, kind 'h', 'v', 'd' (down-right) or 'a' (down-left),
    on a plane of 1000 +- 2 in which `share` of the pixels, none within `clear` pixels of a run,
    lie at 1000 +- 400.  Those single outliers set avgDev (about 40), so next to a run the 3x3
    average is decided by the run alone: (3 avgDev) / 8 < avgDev / 2 <= 2 (3 avgDev) / 8.  A run's
    first pixel is corrected, then the next sees the correction, and so on down the whole run."""
    p = noise_plane(H, W, seed, spread=2)
    rng = np.random.default_rng(seed + 1000)
    step = {"h": (1, 0), "v": (0, 1), "d": (1, 1), "a": (-1, 1)}
    cells = []
    for kind, x, y, n in runs:
        dx, dy = step[kind]
        cells += [(x + i * dx, y + i * dy) for i in range(n) if 0 <= x + i * dx < W and 0 <= y + i * dy < H]
    near = np.zeros((H, W), dtype=bool)
    for x, y in cells:
        near[max(0, y - clear):y + clear + 1, max(0, x - clear):x + clear + 1] = True
    mask = (rng.random((H, W)) < share) & ~near
    p[mask] = np.where(rng.random((H, W)) < 0.5, 1400, 600)[mask].astype(np.uint16)
    lvl = run_level(p)
    for x, y in cells:
        p[y, x] = lvl
    return p


def dependence_case():
    """the pinned 24 x 48 case: single outliers, a 40-pixel horizontal, an 8-pixel vertical and an
    8-pixel diagonal run"""
    return chain_plane(24, 48, 11, [("h", 4, 2, 40), ("v", 3, 9, 8), ("d", 20, 10, 8)], share=0.2)


def dense_plane(H, W, seed, share=0.05):
    """`share` of the pixels random outliers of both signs"""
    p = noise_plane(H, W, seed)
    rng = np.random.default_rng(seed + 7)
    mask = rng.random((H, W)) < share
    vals = np.where(rng.random((H, W)) < 0.5, rng.integers(1500, 60000, size=(H, W)), rng.integers(1, 700, size=(H, W)))
    p[mask] = vals[mask].astype(np.uint16)
    return p
