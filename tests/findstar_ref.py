"""numpy / Python restatement of the whole-image part of Siril 0.9's peaker
(src/algos/star_finder.c:103-255), the oracle of sg_findstar* (include/sirilgpu.h).

  piece                 literal                    rule (vectorised, what the GPU tests compare with)
  B3-spline smooth      smooth_literal             smooth
  3x3 peak test         peaks_literal              peaks
plus two deliberately wrong variants the tests must be able to tell from the right ones:
smooth_separable (the same filter as two 1-D passes) and peaks(rule="gt_only" / "ge_all").

Planes are [H][W] uint16 arrays in memory order (bottom-up); candidates are (x, y) in display
(top-down) coordinates, top[y] = plane[H - 1 - y].  Every float32 / float64 step is written with
explicit numpy types: Python floats are weakly typed against numpy scalars.
"""
import math

import numpy as np

from prepro_ref import hist_median, mean_sigma_u16, rtw_v

F32, F64 = np.float32, np.float64
# pave.c:250-279: the group constants, in source order
K1, K2, K3, K4, K5, K6 = (F64(0.00390625), F64(0.015625), F64(0.0234375), F64(0.06250), F64(0.09375),
                          F64(0.140625))
MIN_SIDE = 32       # wavelet_transform_data refuses min(Nl, Nc) < pow(2, Nbr_Plan + 2) (transform.c:194-201)
NORM = 65535


# ---------------------------------------------------------------------------- threshold

def to_word(x):
    """(WORD)x of a double on x86-64: cvttsd2si to int32 (0x80000000 out of range / NaN), low 16 bits"""
    x = float(x)
    if math.isnan(x) or not (-2147483649.0 < x < 2147483648.0):
        return 0
    return int(x) & 0xFFFF


def threshold(plane, k):
    """Compute_threshold (:39-57): dict(ngood, median, sigma, threshold, wrapped, no_data)"""
    n, _, sigma = mean_sigma_u16(plane)
    if n == 0:
        return dict(ngood=0, median=0.0, sigma=0.0, threshold=0, wrapped=0, no_data=1)
    median = hist_median(plane, n)
    t = float(to_word(median)) + float(k) * float(to_word(sigma))
    return dict(ngood=n, median=median, sigma=sigma, threshold=to_word(t), wrapped=int(t >= 65536.0), no_data=0)


def sigma_from_sums(plane):
    """the reference's expression on the exact integer sums (what the device path evaluates when
    the sum of squares stays below 2^53): (sigma, sum2)"""
    g = np.asarray(plane).reshape(-1).astype(np.uint64)
    g = g[g != 0]
    n, s, s2 = int(g.size), int(g.sum(dtype=np.uint64)), int((g * g).sum(dtype=np.uint64))
    if n <= 1:
        return 0.0, s2
    m = float(s) / float(n)
    return math.sqrt((float(s2) / float(n)) - (m * m)), s2


# ---------------------------------------------------------------------------- detection plane

def _ind(i, n):
    """test_ind (pave.c:88-102)"""
    return 0 if i < 0 else (n - 1 if i >= n else i)


def smooth_literal(img, step):
    """pave_2d_bspline_smooth (pave.c:227-284), one pixel at a time in the source's operand order"""
    img = np.asarray(img, dtype=F32)
    nl, nc = img.shape
    out = np.zeros((nl, nc), dtype=F32)
    for i in range(nl):
        i1, i2, i3, i4 = _ind(i - step, nl), _ind(i + step, nl), _ind(i - 2 * step, nl), _ind(i + 2 * step, nl)
        for j in range(nc):
            j1, j2, j3, j4 = _ind(j - step, nc), _ind(j + step, nc), _ind(j - 2 * step, nc), _ind(j + 2 * step, nc)
            g1 = F32(F32(F32(img[i3, j3] + img[i3, j4]) + img[i4, j3]) + img[i4, j4])
            g2 = img[i4, j2]
            for a, b in ((i3, j2), (i4, j1), (i3, j1), (i2, j3), (i2, j4), (i1, j3), (i1, j4)):
                g2 = F32(g2 + img[a, b])
            g3 = F32(F32(F32(img[i3, j] + img[i4, j]) + img[i, j3]) + img[i, j4])
            g4 = F32(F32(F32(img[i1, j1] + img[i1, j2]) + img[i2, j1]) + img[i2, j2])
            g5 = F32(F32(F32(img[i1, j] + img[i2, j]) + img[i, j1]) + img[i, j2])
            s = K1 * F64(g1)
            for kk, g in ((K2, g2), (K3, g3), (K4, g4), (K5, g5), (K6, img[i, j])):
                s = F64(s + F64(kk * F64(g)))
            out[i, j] = F32(s)
    return out


def smooth(img, step):
    """the same, vectorised: float32 array adds in the source's order, float64 products and sums"""
    img = np.asarray(img, dtype=F32)
    nl, nc = img.shape
    ii, jj = np.arange(nl), np.arange(nc)
    r = {0: ii, 1: np.clip(ii - step, 0, nl - 1), 2: np.clip(ii + step, 0, nl - 1),
         3: np.clip(ii - 2 * step, 0, nl - 1), 4: np.clip(ii + 2 * step, 0, nl - 1)}
    c = {0: jj, 1: np.clip(jj - step, 0, nc - 1), 2: np.clip(jj + step, 0, nc - 1),
         3: np.clip(jj - 2 * step, 0, nc - 1), 4: np.clip(jj + 2 * step, 0, nc - 1)}

    def group(pairs):
        acc = None
        for a, b in pairs:
            t = img[np.ix_(r[a], c[b])]
            acc = t if acc is None else acc + t         # float32 + float32
        assert acc.dtype == F32
        return acc.astype(F64)

    s = K1 * group([(3, 3), (3, 4), (4, 3), (4, 4)])
    s = s + K2 * group([(4, 2), (3, 2), (4, 1), (3, 1), (2, 3), (2, 4), (1, 3), (1, 4)])
    s = s + K3 * group([(3, 0), (4, 0), (0, 3), (0, 4)])
    s = s + K4 * group([(1, 1), (1, 2), (2, 1), (2, 2)])
    s = s + K5 * group([(1, 0), (2, 0), (0, 1), (0, 2)])
    s = s + K6 * img.astype(F64)
    return s.astype(F32)


def smooth_separable(img, step):
    """WRONG on purpose: the B3 kernel (1 4 6 4 1) / 16 as a column pass after a row pass in float32"""
    img = np.asarray(img, dtype=F32)
    w = [F32(1 / 16), F32(4 / 16), F32(6 / 16), F32(4 / 16), F32(1 / 16)]

    def pass1d(a, axis):
        n = a.shape[axis]
        idx = np.arange(n)
        acc = np.zeros_like(a)
        for kk, off in zip(w, (-2 * step, -step, 0, step, 2 * step)):
            acc = acc + kk * np.take(a, np.clip(idx + off, 0, n - 1), axis=axis)
        return acc.astype(F32)

    return pass1d(pass1d(img, 1), 0)


def smooth_exact(img, step):
    """the tensor-product sum in float64 (exact for integer input below 2^16 at step 1)"""
    img = np.asarray(img, dtype=F64)
    w = [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16]
    nl, nc = img.shape
    out = np.zeros_like(img)
    for a, oi in zip(w, (-2 * step, -step, 0, step, 2 * step)):
        ri = np.clip(np.arange(nl) + oi, 0, nl - 1)
        for b, oj in zip(w, (-2 * step, -step, 0, step, 2 * step)):
            cj = np.clip(np.arange(nc) + oj, 0, nc - 1)
            out += (a * b) * img[np.ix_(ri, cj)]
    return out


def float_plane(plane, smoother=smooth):
    """plane 2 of get_wavelet_layers(.., 3, 2, TO_PAVE_BSPLINE, ..) before reget_rawdata"""
    return smoother(smoother(np.asarray(plane).astype(F32), 1), 2)


def detection_plane(plane, smoother=smooth):
    """(wave uint16, wavelet_applied, ratio_applied): the smoothed plane quantised by reget_rawdata
    (reconstr.c:120-140), or the image itself when the transform refuses it"""
    plane = np.asarray(plane, dtype=np.uint16)
    if min(plane.shape) < MIN_SIDE:
        return plane.copy(), 0, 0
    s = float_plane(plane, smoother)
    maximum = max(F32(0), s.max())
    ratio = F64(65535.0) / F64(maximum) if maximum > F32(65535) else F64(1.0)
    return rtw_v(s.astype(F64) * ratio), 1, int(maximum > F32(65535))


# ---------------------------------------------------------------------------- peak test

def scan_rect(shape, r, area=None):
    """(x0, x1, y0, y1) of the loops at :176-178; area = (x, y, w, h) in display coordinates"""
    H, W = shape
    ax, ay, aw, ah = (0, 0, W, H) if area is None else area
    return ax + r, ax + aw - r, ay + r, ay + ah - r


def peaks_literal(wave, thr, r, area=None):
    """:176-199 as written (the `break` leaves the inner loop only; bingo stays FALSE)"""
    top = np.asarray(wave)[::-1].astype(np.int64)
    x0, x1, y0, y1 = scan_rect(top.shape, r, area)
    out = []
    for y in range(y0, y1):
        for x in range(x0, x1):
            pixel = top[y, x]
            if pixel > thr and pixel < NORM:
                bingo = True
                for yy in range(y - 1, y + 2):
                    for xx in range(x - 1, x + 2):
                        if xx == x and yy == y:
                            continue
                        nb = top[yy, xx]
                        if nb > pixel:
                            bingo = False
                            break
                        elif nb == pixel:
                            if (xx <= x and yy <= y) or (xx > x and yy < y):
                                bingo = False
                                break
                if bingo:
                    out.append((x, y))
    return out


def peaks(wave, thr, r, area=None, rule="ref"):
    """the same, vectorised.  rule "ref": an equal neighbour rejects in the row above and to the
    left; "gt_only" (WRONG): equal neighbours never reject; "ge_all" (WRONG): they always do."""
    top = np.asarray(wave)[::-1].astype(np.int64)
    x0, x1, y0, y1 = scan_rect(top.shape, r, area)
    if x1 <= x0 or y1 <= y0:
        return []
    c = top[y0:y1, x0:x1]
    ok = (c > thr) & (c < NORM)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            nb = top[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            strict = {"ref": dy < 0 or (dy == 0 and dx < 0), "gt_only": False, "ge_all": True}[rule]
            ok &= (nb < c) if strict else (nb <= c)
    return [(int(x) + x0, int(y) + y0) for y, x in np.argwhere(ok)]


def candidates(plane, k, r, area=None, rule="ref", smoother=smooth):
    """the ordered candidate list of peaker for one plane: (list of (x, y), threshold record, wave)"""
    rec = threshold(plane, k)
    wave, _, _ = detection_plane(plane, smoother)
    if rec["no_data"]:
        return [], rec, wave
    return peaks(wave, rec["threshold"], r, area, rule), rec, wave


def boxes(plane, cands, r):
    """:203-211: z[ii][jj] = real_top[y - r + jj][x - r + ii], [n][2r][2r] uint16"""
    top = np.asarray(plane, dtype=np.uint16)[::-1]
    out = np.zeros((len(cands), 2 * r, 2 * r), dtype=np.uint16)
    for n, (x, y) in enumerate(cands):
        out[n] = top[y - r:y + r, x - r:x + r].T
    return out


# ---------------------------------------------------------------------------- test images
# (shared by tests/test_findstar_cpu.py, which holds the conditions the GPU tests rely on, and
# tests/test_gpu_findstar.py)

# [H][W] of the detection-plane cases: the transform's smallest sides, one 64 x 32 tile of the kernel,
# a tile edge - 1 / + 1, exact multiples, 2 x 2 and 3 x 3 tiles with a partial last tile
PLANE_SHAPES = [(32, 32), (32, 33), (33, 32), (32, 64), (32, 63), (33, 65), (64, 128), (37, 70), (70, 130)]


def plane_case(H, W):
    """full-range noise; the seeds are ones at which the separable variant changes a WORD at every shape"""
    return noise_frame(H * 1000 + W + 1, H, W)


def noise_frame(seed, H, W):
    """full-range random uint16"""
    return np.random.default_rng(seed).integers(0, 65536, size=(H, W)).astype(np.uint16)


def star_field(seed, H, W, nstars, fwhm=2.5, bg=800, noise=12.0, peak=(3000, 40000), margin=0):
    """Gaussian stars on a noisy background, their centres `margin` pixels or more from the border"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = rng.normal(bg, noise, size=(H, W))
    s = fwhm / 2.3548
    for _ in range(nstars):
        cx, cy, a = rng.uniform(margin, W - margin), rng.uniform(margin, H - margin), rng.uniform(*peak)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16)


TIE_VALUES = (5000, 6000, 7000)


def tie_image(seed=5, H=31, W=200, density=0.35):
    """a no-wavelet image (H < 32) of three values above the threshold on a low background, dense
    enough that equal neighbours occur at all eight positions"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 10, dtype=np.uint16)
    m = rng.random((H, W)) < density
    img[m] = rng.choice(np.array(TIE_VALUES, dtype=np.uint16), size=int(m.sum()))
    return img


# (seed, H, W, radius, stars, margin) of the star-field cases
STAR_CASES = [(40, 40, 48, 5, 5, 8), (96, 96, 130, 10, 14, 12)]


def star_case(i):
    seed, H, W, r, n, margin = STAR_CASES[i]
    return star_field(seed, H, W, n, margin=margin), r


BATCH_SHAPE = (40, 48)          # [H][W] of the many-frame cases
BATCH_FRAMES = (257, 258)       # one and two frames past the first chunk of sg_findstar_device
BATCH_EMPTY_AREA = (7, 11, 6, 20)       # with r = 3: 2r >= the area's width, nothing to scan
COPY_SWEEP_SHAPE = (31, 8500)   # no wavelet (H < 32), more pixels than k_findstar_copy's capped grid has threads


def batch_sequence(nframes, tail):
    """frames [nframes][1][40][48] for a call of more than one chunk: three star fields in rotation, then
    `tail`, a list of plane numbers (3 = a fourth star field, -1 = an all-zero frame), as the last frames.
    Returns (frames, plane number per frame, the four star fields)."""
    H, W = BATCH_SHAPE
    planes = [star_field(300 + i, H, W, 5, margin=8) for i in range(4)]
    which = [i % 3 for i in range(nframes - len(tail))] + list(tail)
    frames = np.zeros((nframes, 1, H, W), dtype=np.uint16)
    for f, n in enumerate(which):
        if n >= 0:
            frames[f, 0] = planes[n]
    return frames, which, planes


def bright_frame(seed=3, S=1536):
    """S x S pixels bright enough that the sum of squares passes 2^53"""
    return np.random.default_rng(seed).integers(62000, 65535, size=(S, S)).astype(np.uint16)
