"""numpy / Python restatement of Siril 0.9's sequence preprocessing (seqpreprocess,
src/core/siril.c:1019-1169), the oracle of sg_prepro_* (include/sirilgpu.h).

Each piece is written twice, as tests/debayer_vng_ref.py does: a *literal* form that follows the
reference line by line, and the *rule* the plan and the kernels implement.  tests/test_prepro_cpu.py
holds the two equal; the GPU tests compare the library with the rule forms (which are vectorised).

  piece                    literal                      rule
  5x5 cold median          median24_literal             median24_rule
  in-place correction      cosmetic_literal             cosmetic_rule (components, list order inside)
  noise of one row         noise_row_literal            noise_row_rule (predecessor differences,
                                                        nested clip masks over the uncompacted row)
  golden-section search    search_literal               Golden (state machine, one new point a step)

Images are [H][W] (or [C][H][W]) uint16 arrays in memory order.  Python floats are IEEE doubles and
CPython never fuses a multiply with an add, so the double expressions below round as the C ones.
"""
import math

import numpy as np

GR = (math.sqrt(5) - 1) / 2
NITER, SIGMA_CLIP = 3, 5.


def rtw(x):
    """round_to_WORD (src/core/utils.c:68-74) of a double"""
    if x <= 0.0:
        return 0
    if x > 65535.0:
        return 65535
    return int(x + 0.5)


def rtw_v(x):
    """round_to_WORD of a float64 array"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x <= 0.0, 0, np.where(x > 65535.0, 65535, np.floor(np.minimum(x, 65535.0) + 0.5))).astype(np.uint16)


# ---------------------------------------------------------------------------- statistics

def mean_sigma_u16(a):
    """FnMeanSigma_ushort, nullcheck with null value 0: (ngood, mean, sigma); sequential double sums"""
    g = np.asarray(a).reshape(-1)
    g = g[g != 0].astype(np.float64)
    n = int(g.size)
    if n == 0:
        return 0, 0.0, 0.0
    s = float(np.add.accumulate(g)[-1])             # accumulate adds in order, like the C loop
    s2 = float(np.add.accumulate(g * g)[-1])
    if n == 1:
        return 1, s, 0.0
    m = s / n
    return n, m, math.sqrt((s2 / n) - (m * m))


def mean_sigma_sums(n, s, s2):
    """FnMeanSigma_int without nullcheck from the exact integer sums: (mean, sigma)"""
    if n > 1:
        m = float(s) / float(n)
        v = (float(s2) / float(n)) - (m * m)
        return m, (math.sqrt(v) if v >= 0 else float("nan"))
    if n == 1:
        return float(s), 0.0
    return 0.0, 0.0


def hist_median(a, ngood):
    """siril_stats_ushort_median on computeHisto's 65536 bins over [0, 65535): 65535 is not counted"""
    g = np.asarray(a).reshape(-1)
    h = np.bincount(g[g < 65535], minlength=65536)
    run = 0.0
    for i in range(1, 65536):
        run += float(h[i])
        if run > ngood * 0.5:
            return float(i)
    return 0.0


def auto_level(flat):
    """(float)mean of the non-zero pixels of the flat's layer 0, as a double; None: no statistics"""
    n, m, _ = mean_sigma_u16(np.asarray(flat).reshape(-1, flat.shape[-2], flat.shape[-1])[0])
    return None if n == 0 else float(np.float32(m))


def thresholds(dark, sig):
    """(sigma, median, thresCold, thresHot) of find_deviant_pixels; None without a non-zero pixel"""
    n, _, sigma = mean_sigma_u16(dark)
    if n == 0:
        return None
    median = hist_median(dark, n)
    if sig[0] == -1.0:
        cold = -1.0
    else:
        val = median - (sig[0] * sigma)
        cold = val if val > 0 else 0.0
    if sig[1] == -1.0:
        hot = 65535.0 + 1
    else:
        val = median + (sig[1] * sigma)
        hot = 65535.0 if val > 65535.0 else val
    return sigma, median, cold, hot


def find_deviant(dark, sig):
    """[(x, y, cold)] in the reference's raster order of the one-layer memory-order dark"""
    t = thresholds(dark, sig)
    if t is None:
        return []
    _, _, cold, hot = t
    d = np.asarray(dark).astype(np.float64)
    is_hot = d >= hot
    is_cold = (~is_hot) & (d <= cold)
    ys, xs = np.nonzero(is_hot | is_cold)         # row-major: raster order
    return [(int(x), int(y), bool(is_cold[y, x])) for x, y in zip(xs, ys)]


# ---------------------------------------------------------------------------- cosmetic correction

def _neighbours(buf, xx, yy, cold, is_cfa):
    H, W = buf.shape
    step = 2 if is_cfa else 1
    radius = 2 * step if cold else step
    out = []
    for y in range(yy - radius, yy + radius + 1, step):
        for x in range(xx - radius, xx + radius + 1, step):
            if 0 <= y < H and 0 <= x < W and (x != xx or y != yy):
                out.append(int(buf[y, x]))
    return out


def median24_literal(vals):
    """getMedian5x5's tail: a calloc'ed array of 24, the n values at its front, sorted whole, the
    gsl median of value[24 - n - 1 ...][:n]; value[-1] (n = 24) is read as 0 (include/sirilgpu.h)"""
    n = len(vals)
    value = [0] * 24
    for i, v in enumerate(vals):
        value[i] = v
    start = 24 - n - 1
    value.sort()
    if n == 0:
        return 0
    at = lambda i: 0 if start + i < 0 else value[start + i]
    lhs, rhs = (n - 1) // 2, n // 2
    med = float(at(lhs)) if lhs == rhs else (at(lhs) + at(rhs)) / 2.0
    return rtw(med)


def median24_rule(vals):
    """the median of {0} and the n - 1 smallest values"""
    n = len(vals)
    if n == 0:
        return 0
    m = [0] + sorted(vals)[:n - 1]
    return rtw(float(m[(n - 1) // 2]) if n & 1 else (m[(n - 1) // 2] + m[n // 2]) / 2.0)


def average3x3(vals):
    """getAverage3x3's tail (no neighbour at all: 0, include/sirilgpu.h)"""
    if not vals:
        return 0
    value = 0.0
    for v in vals:
        value += float(v)
    return rtw(value / len(vals))


def correct_one(buf, x, y, cold, is_cfa, median=median24_rule):
    vals = _neighbours(buf, x, y, cold, is_cfa)
    return median(vals) if cold else average3x3(vals)


def cosmetic_literal(frame, dev, is_cfa):
    """cosmeticCorrection: in place, in list order"""
    buf = np.array(frame, dtype=np.uint16)
    for x, y, cold in dev:
        buf[y, x] = correct_one(buf, x, y, cold, is_cfa, median24_literal)
    return buf


def components(dev, W, H, is_cfa):
    """the schedule: lists of indices into dev, one per connected component of "lies in the other's
    window", each in list order, components ordered by their first pixel"""
    where = {(x, y): i for i, (x, y, _) in enumerate(dev)}
    parent = list(range(len(dev)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    step = 2 if is_cfa else 1
    for i, (x, y, cold) in enumerate(dev):
        r = 2 * step if cold else step
        for yy in range(y - r, y + r + 1, step):
            for xx in range(x - r, x + r + 1, step):
                j = where.get((xx, yy))
                if j is not None and j != i:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    groups = {}
    for i in range(len(dev)):
        groups.setdefault(find(i), []).append(i)
    return [groups[r] for r in sorted(groups)]


def cosmetic_rule(frame, dev, is_cfa, order=None):
    """the correction walked component by component (any component order gives the same image)"""
    buf = np.array(frame, dtype=np.uint16)
    comps = components(dev, buf.shape[1], buf.shape[0], is_cfa)
    for c in (comps if order is None else [comps[i] for i in order]):
        for i in c:
            x, y, cold = dev[i]
            buf[y, x] = correct_one(buf, x, y, cold, is_cfa, median24_rule)
    return buf


# ---------------------------------------------------------------------------- background noise

def dark_subtracted(raw, dark, k):
    """imoper(fit, soper(dark, k, MUL), SUB): max(raw - round_to_WORD(dark * k), 0) as int64"""
    dk = rtw_v(np.asarray(dark).astype(np.float64) * float(k)).astype(np.int64)
    return np.maximum(np.asarray(raw).astype(np.int64) - dk, 0)


def noise_row_literal(rowpix):
    """one row of FnNoise1_ushort (nullcheck, null value 0): the final stdev, or None when the row
    does not contribute"""
    nx = len(rowpix)
    rowpix = [int(v) for v in rowpix]
    ii = 0
    while ii < nx and rowpix[ii] == 0:
        ii += 1
    if ii == nx:
        return None
    v1 = rowpix[ii]
    differences = []
    ii += 1
    while ii < nx:
        while ii < nx and rowpix[ii] == 0:
            ii += 1
        if ii == nx:
            break
        differences.append(v1 - rowpix[ii])
        v1 = rowpix[ii]
        ii += 1
    nvals = len(differences)
    if nvals < 2:
        return None
    mean, stdev = mean_sigma_sums(nvals, sum(differences), sum(d * d for d in differences))
    if stdev > 0.:
        for _ in range(NITER):
            kk = 0
            for ii in range(nvals):
                if abs(differences[ii] - mean) < SIGMA_CLIP * stdev:
                    if kk < ii:
                        differences[kk] = differences[ii]
                    kk += 1
            if kk == nvals:
                break
            nvals = kk
            mean, stdev = mean_sigma_sums(nvals, sum(differences[:nvals]), sum(d * d for d in differences[:nvals]))
    return stdev


def noise_row_rule(rowpix, passes=None, dropped=None):
    """the kernel's form: a difference per non-zero pixel with a non-zero predecessor, integer sums,
    clip pass j keeping what satisfies the conditions of passes 0 .. j (nested sets); `passes`
    (a list) receives the number of clip passes that ran, `dropped` what each of them dropped"""
    g = np.asarray(rowpix).astype(np.int64)
    g = g[g != 0]
    d = g[:-1] - g[1:]
    if d.size < 2:
        return None
    nvals = int(d.size)
    mean, stdev = mean_sigma_sums(nvals, int(d.sum()), int((d * d).sum()))
    conds = []
    ran = 0
    if stdev > 0.:
        for _ in range(NITER):
            ran += 1
            conds.append((mean, stdev))
            keep = np.ones(d.size, dtype=bool)
            for m, s in conds:
                keep &= np.abs(d - m) < SIGMA_CLIP * s
            kk = int(keep.sum())
            if dropped is not None:
                dropped.append(nvals - kk)
            if kk == nvals:
                break
            nvals = kk
            mean, stdev = mean_sigma_sums(nvals, int(d[keep].sum()), int((d[keep] * d[keep]).sum()))
    if passes is not None:
        passes.append(ran)
    return stdev


def noise_image(p, row=noise_row_rule):
    """FnNoise1_ushort of the image p [H][W]"""
    H, W = p.shape
    if W < 3:
        return 0.0
    diffs = [s for s in (row(p[y]) for y in range(H)) if s is not None]
    if not diffs:
        xnoise = 0.0
    elif len(diffs) == 1:
        xnoise = diffs[0]
    else:
        diffs.sort()
        xnoise = (diffs[(len(diffs) - 1) // 2] + diffs[len(diffs) // 2]) / 2.
    return .70710678 * xnoise


def objective(raw, dark, k, row=noise_row_rule):
    """evaluateNoiseOfCalibratedImage on layer 0 (0.0 when nothing is left: statistics() is NULL,
    which the row loop gives as well)"""
    return noise_image(dark_subtracted(raw, dark, k), row)


def has_nan_row(raw, dark, k):
    p = dark_subtracted(raw, dark, k)
    return any(isinstance(s, float) and math.isnan(s) for s in (noise_row_rule(r) for r in p))


# ---------------------------------------------------------------------------- golden-section search

def search_literal(f, a=0.0, b=2.0, tol=1E-3):
    """goldenSectionSearch: (k, iterations); both points evaluated afresh every iteration"""
    c = b - GR * (b - a)
    d = a + GR * (b - a)
    it = 0
    while True:
        fc = f(c)
        fd = f(d)
        if fc < fd:
            b = d
            d = c
            c = b - GR * (b - a)
        else:
            a = c
            c = d
            d = a + GR * (b - a)
        it += 1
        if not abs(c - d) > tol:
            break
    return (b + a) / 2, it


class Golden:
    """the same search as a state machine (SgGolden of sg_prepro_plan.hpp)"""

    def __init__(self, a=0.0, b=2.0, tol=1E-3):
        self.a, self.b, self.tol = a, b, tol
        self.c = b - GR * (b - a)
        self.d = a + GR * (b - a)
        self.fc = self.fd = None
        self.done, self.iters = False, 0

    def want(self):
        if self.done:
            return []
        return ([self.c] if self.fc is None else []) + ([self.d] if self.fd is None else [])

    def feed(self, vals):
        vals = list(vals)
        if self.fc is None:
            self.fc = vals.pop(0)
        if self.fd is None:
            self.fd = vals.pop(0)
        if self.fc < self.fd:
            self.b, self.d, self.fd = self.d, self.c, self.fc
            self.c, self.fc = self.b - GR * (self.b - self.a), None
        else:
            self.a, self.c, self.fc = self.c, self.d, self.fd
            self.d, self.fd = self.a + GR * (self.b - self.a), None
        self.iters += 1
        if not abs(self.c - self.d) > self.tol:
            self.done = True

    def result(self):
        return (self.b + self.a) / 2


def search_rule(f):
    g = Golden()
    while not g.done:
        g.feed([f(k) for k in g.want()])
    return g.result(), g.iters


# ---------------------------------------------------------------------------- the whole frame

def calibrate(raw, offset=None, dark=None, flat=None, level=1.0, optd_k=None):
    """preprocess() on [C][H][W] (after darkOptimization's subtraction when optd_k is given);
    level: the float level as a double"""
    v = np.asarray(raw).astype(np.int64)
    if optd_k is not None:
        dk = np.asarray(dark).astype(np.int64)
        if offset is not None:
            dk = np.maximum(dk - np.asarray(offset).astype(np.int64), 0)      # round_to_WORD(dark - offset)
        v = np.maximum(v - rtw_v(dk.astype(np.float64) * float(optd_k)).astype(np.int64), 0)
    if offset is not None:
        v = np.maximum(v - np.asarray(offset).astype(np.int64), 0)
    if dark is not None and optd_k is None:
        v = np.maximum(v - np.asarray(dark).astype(np.int64), 0)
    if flat is not None:
        f = np.where(np.asarray(flat) == 0, 1, flat).astype(np.float64)
        v = rtw_v(float(np.float32(level)) * (v.astype(np.float64) / f)).astype(np.int64)
    return v.astype(np.uint16)


def preprocess(frames, offset=None, dark=None, flat=None, dark_optimization=False, cosmetic=False,
               cosme_sigma=(-1.0, -1.0), is_cfa=False, autolevel=False, normalisation=1.0):
    """the sequence branch of seqpreprocess on frames [N][C][H][W]: (calibrated frames, k per frame)"""
    frames = np.asarray(frames)
    N, C, H, W = frames.shape
    level = float(np.float32(normalisation))
    if flat is not None and autolevel:
        level = auto_level(flat)
        assert level is not None
    dev = []
    if cosmetic and dark is not None and C == 1:
        dev = find_deviant(np.asarray(dark).reshape(H, W), cosme_sigma)
    out = np.empty_like(frames)
    ks = np.ones(N)
    for i in range(N):
        k = None
        if dark_optimization:
            assert C == 1 and dark is not None
            k, _ = search_rule(lambda kk: objective(frames[i, 0], np.asarray(dark).reshape(H, W), kk))
            ks[i] = k
        cal = calibrate(frames[i], offset, dark, flat, level, optd_k=k)
        if dev:
            cal = cosmetic_rule(cal[0], dev, is_cfa)[None]
        out[i] = cal
    return out, ks


# ---------------------------------------------------------------------------- test inputs

def fit_case(H, W, k_true, seed):
    """a dark (gamma thermal signal + 1 % hot pixels, N(0, 3) read noise) and frames
    rtw(500 + k_true * T + N(0, 12)) with 2 % zeros, one frame per entry of k_true"""
    rng = np.random.default_rng(seed)
    T = rng.gamma(2.0, 150.0, size=(H, W))
    hot = rng.random((H, W)) < 0.01
    T[hot] += rng.uniform(3000, 20000, size=int(hot.sum()))
    dark = rtw_v(T + rng.normal(0, 3, size=(H, W)))
    frames = []
    for kt in k_true:
        f = rtw_v(500 + kt * T + rng.normal(0, 12, size=(H, W)))
        f[rng.random((H, W)) < 0.02] = 0
        frames.append(f)
    return np.stack(frames)[:, None], dark


BATCH_FRAMES = 257              # two chunks of sg_prepro_frames_device and one frame
BATCH_SHAPE = (9, 67)
BATCH_FRAMES_RGB = 129          # one chunk and one frame, three layers, no fit
# (H, W, gap) of one-layer frames that k_prepro_calibrate's capped grid sweeps twice: through the 128-bit
# body (stride a multiple of 8 samples, the frame not) and through the scalar loop
SWEEP_VECTOR = (2050, 4101, 6)
SWEEP_SCALAR = (1025, 1025, 3)


def batch_fit_case():
    """fit_case for a call of more than two chunks: (frames [257][1][9][67], dark [9][67], k_true), every
    frame with a k_true of its own over [0.2, 1.7]"""
    k_true = np.linspace(0.2, 1.7, BATCH_FRAMES)
    frames, dark = fit_case(*BATCH_SHAPE, k_true, seed=sum(BATCH_SHAPE))
    return frames, dark, k_true


def edge_rows():
    """noise rows: (name, row, clip passes expected or None)"""
    rng = np.random.default_rng(5)
    rows = [("zeros", np.zeros(70, dtype=np.int64), None)]
    for nz in (1, 2, 3):
        r = np.zeros(130, dtype=np.int64)
        r[rng.choice(130, nz, replace=False)] = rng.integers(1, 65536, nz)
        rows.append((f"{nz} non-zero", r, None))
    g = rng.normal(1000, 20, 200).astype(np.int64)
    z = g.copy()
    z[:5] = 0
    z[-7:] = 0
    z[60:70] = 0           # a run across the 64-lane boundary
    z[127:129] = 0
    rows.append(("edge zeros and runs", z, None))
    rows.append(("constant", np.full(90, 777, dtype=np.int64), 0))
    rows.append(("gauss", g, None))
    # 0 .. 3 clip passes: outliers at growing distance, each pass exposing the next
    base = 1000 + (np.arange(400) % 2)          # differences of +-1
    one = base.copy()
    one[100] = 1200
    two = one.copy()
    two[200] = 30000
    three = two.copy()
    three[300] = 1020
    three[50] = 1012
    rows += [("clip0", base, 1), ("clip1", one, None), ("clip2", two, None), ("clip3", three, None)]
    return rows


CLUSTER_SIG = (0.01, 1.0)


def cluster_dark(H, W, seed, every=False):
    """a one-layer dark whose deviant pixels form the awkward clusters: a full hot column, a full
    hot row, a 6x6 hot block, isolated hot pixels, cold pixels within two of hot ones, all four
    corners and the edges (as far as the shape has room)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(400, 6, size=(H, W)).clip(1, 65535).astype(np.uint16)
    if every:
        # sigma 0 and median 30000: every 30000 is hot (>= thresHot), every 0 is cold (<= thresCold)
        d[:] = np.where(rng.random((H, W)) < 0.5, 30000, 0)
        return d
    hot, cold = 65000, 0                       # deviant with CLUSTER_SIG at every shape used
    d[:, W // 3] = hot                         # column
    d[H // 3, :] = hot                         # row
    y0, x0 = (H // 2, W // 2) if min(H, W) >= 16 else (H - 3, W - 3)
    d[y0:y0 + 6, x0:x0 + 6] = hot              # block (clipped by the corner on a small image)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        d[y, x] = hot if (x + y) % 2 == 0 else cold
    d[0, W // 2], d[H - 1, W // 2 + 1 if W // 2 + 1 < W else 0] = cold, hot
    d[H // 2, 0], d[H // 2 - 1, W - 1] = hot, cold
    for _ in range(max(2, H * W // 200)):
        y, x = int(rng.integers(H)), int(rng.integers(W))
        d[y, x] = hot
        yy, xx = min(H - 1, y + int(rng.integers(3))), min(W - 1, x + int(rng.integers(3)))
        if (yy, xx) != (y, x):
            d[yy, xx] = cold
    return d
