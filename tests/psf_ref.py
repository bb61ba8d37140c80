"""numpy fp64 restatement of the second half of Siril 0.9's peaker (src/algos/star_finder.c:200-247,
src/algos/PSF.c:46-157, 160-220, 314-428, 620-662), the oracle of sg_findstar_fit* (include/sirilgpu.h)
and of siril-0.9_amd/csrc/sg_psf.h.

  piece                 here
  psf_init_data         init_literal (getMedian3x3 with its zero padding and pointer offset, as written)
  psf_Gaussian_f / _df  model (the reference's formulas, vectorised over the box)
  lmsder                lm (MINPACK lmder / lmpar in the scaled variables y = D p; see sg_psf.h), for any
                        parameter count and model: seqpsf_ref runs it with p = 6 and p = 7
  finish, is_star       finish, is_star
  peaker :200-247       peaker_tail

A box is the gsl_matrix z of peaker, z[ii][jj] = top[y - r + jj][x - r + ii] (findstar_ref.boxes):
matrix rows run along image x and the model's x0 belongs to the column index (image y).

Many fits end at the cap of 10 iterations, so the answer is "x after these iterations", and no
converged optimiser can be the reference.  What another implementation of the same algorithm may
differ by is measured instead: VARIANTS change one thing each in the arithmetic the device does
differently (summation order, linear algebra, exp by one ulp, contraction of the sums).
  - A box is branch-stable when all variants agree on status, iters and the whole accept / reject
    trace, and no is_star comparison (nor the sx / sy swap) lies within 100 * TOL of flipping.
  - SPREAD_MEASURED is the largest relative spread (denominator max(|v|, 1)) of any reported field
    across the variants over the stable boxes of all GPU test cases (starfit_cases), TOL = 16 x it:
    the device differs in summation order, contraction and exp at once, each variant in one.
    tests/test_psf_cpu.py recomputes the spread and holds it within TOL / 16.
"""
import math

import numpy as np

import findstar_ref as fsr

F64 = np.float64
LN2 = 0.6931471805599453            # log(2.0)
FWHM_K = 2.0 * math.sqrt(math.log(2.0) * 2.0)
NP = 6
MAX_ITER, MAX_INNER, MAX_LMPAR = 10, 10, 10
DBL_MIN = 2.2250738585072014e-308

FIT_STAR, FIT_NOT_ENOUGH_PIXELS, FIT_NONFINITE, FIT_BAD_FWHM, FIT_NOT_STAR, FIT_OVER_CAP = range(6)

# measured by tests/test_psf_cpu.py::test_spread_within_tol over starfit_cases (see the docstring)
SPREAD_MEASURED = 1.10e-13      # measured 1.0902e-13 (the case of radius 5), rounded up
TOL = 16 * SPREAD_MEASURED
# restatement against scipy.optimize.least_squares run to 1e-12 from the same start, on boxes where
# the delta test was met before the cap: the largest relative parameter difference observed
# (tests/test_psf_cpu.py::test_restatement_is_a_working_lm), and 4 x it as the bound
LSQ_DIFF_MEASURED = 1.17e-5     # measured 1.1620e-05 over 83 converged boxes, rounded up
LSQ_BOUND = 4 * LSQ_DIFF_MEASURED

FIELDS = ("B", "A", "x0", "y0", "sx", "sy", "fwhmx", "fwhmy", "mag", "rmse", "xpos", "ypos")

# (sums, linalg, exp, contraction): the base is the sequential form of sg_psf_fit_box
BASE = dict(sums="seq", linalg="chol", exp="libm", fma="off")
VARIANTS = {
    "base": BASE,
    "pairwise": dict(BASE, sums="lanes"),     # 64 strided partial sums, then a butterfly: the device's order
    "qr": dict(BASE, linalg="qr"),            # Householder QR of [J D^-1; sqrt(par) I] instead of Cholesky
    "exp_ulp": dict(BASE, exp="ulp"),         # every exp result moved one ulp up or down, fixed seed
    "fused": dict(BASE, fma="fused"),         # products and running sums unrounded (80-bit) until the end
}
ULP_SEED = 20261


# ---------------------------------------------------------------------------- start values

def median3x3_literal(z, xx, yy):
    """getMedian3x3 (PSF.c:46-73) as written: 8 zeroed doubles, the neighbours inside the box, all 8
    sorted, the median of n values read from the offset 8 - n - 1; truncated to WORD"""
    h, w = z.shape
    value = [0.0] * 8
    n = 0
    for y in range(yy - 1, yy + 2):
        for x in range(xx - 1, xx + 2):
            if 0 <= y < h and 0 <= x < w and (x != xx or y != yy):
                value[n] = float(z[y, x])
                n += 1
    start = 8 - n - 1
    value.sort()
    lhs, rhs = (n - 1) // 2, n // 2        # gsl_stats_median_from_sorted_data
    median = value[start + lhs] if lhs == rhs else (value[start + lhs] + value[start + rhs]) / 2.0
    return int(median) & 0xFFFF


def remove_hot_pixels(z):
    out = np.zeros(z.shape, dtype=F64)
    for y in range(z.shape[0]):
        for x in range(z.shape[1]):
            out[y, x] = median3x3_literal(z, x, y)
    return out


def init_literal(box, bg):
    """psf_init_data (PSF.c:92-139) and x_init of psf_minimiz_no_angle (:334-336):
    [bg, max, x0, y0, SX, SY] as float64"""
    z = np.asarray(box).astype(F64)
    nrows, ncols = z.shape
    m = remove_hot_pixels(z)
    i, j = np.unravel_index(int(np.argmax(m)), m.shape)     # the first maximum in row-major order
    i, j = int(i), int(j)
    mx = m[i, j]
    ii1 = ii2 = perm1 = i
    jj1 = jj2 = perm2 = j
    bg = float(bg)
    while 2.0 * (z[ii1, perm2] - bg) > (z[perm1, perm2] - bg) and ii1 < nrows - 1.0:
        ii1 += 1
    while 2.0 * (z[ii2, perm2] - bg) > (z[perm1, perm2] - bg) and ii2 > 0:
        ii2 -= 1
    while 2.0 * (z[perm1, jj1] - bg) > (z[perm1, perm2] - bg) and jj1 < ncols - 1:
        jj1 += 1
    while 2.0 * (z[perm1, jj2] - bg) > (z[perm1, perm2] - bg) and jj2 > 0:
        jj2 -= 1
    v0 = (jj1 + jj2 + 2) / 2.0
    v1 = (ii1 + ii2 + 2) / 2.0
    v3 = float(int(((ii1 - ii2) ** 2) / 4.0 / LN2))
    v4 = float(int(((jj1 - jj2) ** 2) / 4.0 / LN2))
    return np.array([bg, mx, v0, v1, v4, v3], dtype=F64)


# ---------------------------------------------------------------------------- model

def model(x, z, rng=None):
    """psf_Gaussian_f / psf_Gaussian_df (sigma = 1) over the box: (f [n], J [n][6]) in matrix order"""
    n2r, n2c = z.shape
    tx = np.arange(1, n2c + 1, dtype=F64)[None, :]
    ty = np.arange(1, n2r + 1, dtype=F64)[:, None]
    B, A, x0, y0, SX, SY = [F64(v) for v in x]
    with np.errstate(all="ignore"):
        dx = tx - x0 + 0 * ty
        dy = ty - y0 + 0 * tx
        c = np.exp(-(dx * dx / SX + dy * dy / SY))
        if rng is not None:
            c = np.nextafter(c, np.where(rng.integers(0, 2, size=c.shape) == 1, np.inf, -np.inf))
        f = B + A * c - z
        J = np.stack([np.ones_like(c), c, A * c * 2 * dx / SX, A * c * 2 * dy / SY,
                      A * c * (dx * dx) / (SX * SX), A * c * (dy * dy) / (SY * SY)], axis=-1)
    return f.reshape(-1), J.reshape(-1, NP)


def _total(cols, v):
    """the sum over pixels of each column of cols [n][k] as the variant sums it"""
    with np.errstate(all="ignore"):
        if v["fma"] == "fused":
            return np.cumsum(cols, axis=0, dtype=np.longdouble)[-1].astype(F64)
        if v["sums"] == "seq":
            return np.cumsum(cols, axis=0)[-1]
        n, k = cols.shape
        pad = (-n) % 64
        lanes = np.concatenate([cols, np.zeros((pad, k), dtype=cols.dtype)]).reshape(-1, 64, k)
        part = np.cumsum(lanes, axis=0)[-1]                 # [64][k]: lane l holds pixels l, l + 64, ..
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            part = part + part[idx ^ o]
        return part[0]


def _products(a, b, v):
    if v["fma"] == "fused":
        return a.astype(np.longdouble) * b.astype(np.longdouble)
    return a * b


def sums(x, z, v, rng=None):
    """(a [6][6] = J^T J, g [6] = J^T f, ff = |f|^2, J)"""
    f, J = model(x, z, rng)
    with np.errstate(all="ignore"):
        cols = [_products(J[:, i], J[:, j], v) for i in range(NP) for j in range(i, NP)]
        cols += [_products(J[:, i], f, v) for i in range(NP)]
        cols.append(_products(f, f, v))
        t = _total(np.stack(cols, axis=1), v)
    a = np.zeros((NP, NP), dtype=F64)
    k = 0
    for i in range(NP):
        for j in range(i, NP):
            a[i, j] = a[j, i] = t[k]
            k += 1
    return a, t[21:27].copy(), F64(t[27]), J


def resid(x, z, v, rng=None):
    f, _ = model(x, z, rng)
    with np.errstate(all="ignore"):
        return F64(_total(_products(f, f, v)[:, None], v)[0])


def flux(z, B, v):
    """psf_get_mag's intensity, the sum of z - B"""
    with np.errstate(all="ignore"):
        return F64(_total((z.reshape(-1) - F64(B))[:, None], dict(v, fma="off"))[0])


# ---------------------------------------------------------------------------- p x p linear algebra
# (p is read from the arguments: 6 here, 6 and 7 in seqpsf_ref)

def _chol(At, par):
    """L L^T = At + par I as sg_psf.h does it; (L, ri = 1 / diag L, ok)"""
    p = At.shape[0]
    L = np.zeros((p, p), dtype=F64)
    ri = np.zeros(p, dtype=F64)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(p):
            d = At[j, j] + par
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not d > 0.0:
                ok = False
            l = np.sqrt(d)
            rl = 1.0 / l
            L[j, j] = l
            ri[j] = rl
            for i in range(j + 1, p):
                val = At[i, j]
                for k in range(j):
                    val = val - L[i, k] * L[j, k]
                L[i, j] = val * rl
    return L, ri, ok


def _fwd(L, ri, w):
    w = w.copy()
    with np.errstate(all="ignore"):
        for i in range(len(w)):
            val = w[i]
            for k in range(i):
                val = val - L[i, k] * w[k]
            w[i] = val * ri[i]
    return w


def _bwd(L, ri, w):
    w = w.copy()
    n = len(w)
    with np.errstate(all="ignore"):
        for i in range(n - 1, -1, -1):
            val = w[i]
            for k in range(i + 1, n):
                val = val - L[k, i] * w[k]
            w[i] = val * ri[i]
    return w


def _norm(v):
    t = F64(0.0)
    with np.errstate(all="ignore"):
        for k in range(len(v)):
            t = t + v[k] * v[k]
        return np.sqrt(t)


def _solve(L, ri, gt):
    """(y = (L L^T)^-1 gt, |y|, |L^-1 (y / |y|)|^2)"""
    y = _bwd(L, ri, _fwd(L, ri, gt))
    n = _norm(y)
    with np.errstate(all="ignore"):
        wn = _norm(_fwd(L, ri, y / n))
    return y, n, wn * wn


class _Chol:
    """the factorisation of At + par I through the normal equations"""

    def __init__(self, At, gt, Js):
        self.At, self.gt = At, gt

    def factor(self, par):
        self.L, self.ri, ok = _chol(self.At, par)
        return ok

    def solve(self):
        return _solve(self.L, self.ri, self.gt)


class _QR:
    """the same through Householder QR of [J D^-1; sqrt(par) I]: R^T R = At + par I without forming At"""

    def __init__(self, At, gt, Js):
        self.Js, self.gt = Js, gt

    def factor(self, par):
        with np.errstate(all="ignore"):
            M = np.concatenate([self.Js, math.sqrt(par) * np.eye(self.Js.shape[1])]) if par > 0 else self.Js
            if not np.isfinite(M).all():
                return False
            self.R = np.linalg.qr(M, mode="r")
        d = np.abs(np.diag(self.R))
        return bool((d > 0).all() and np.isfinite(self.R).all())

    def solve(self):
        L = self.R.T.copy()
        with np.errstate(all="ignore"):
            ri = 1.0 / np.diag(L)
        return _solve(L, ri, self.gt)


def lmpar(fac, gt, delta, par):
    """MINPACK lmpar in the scaled variables: (y = D p, par)"""
    par_lower = F64(0.0)
    with np.errstate(all="ignore"):
        if fac.factor(0.0):
            y, dxnorm, phider = fac.solve()
            fp = dxnorm - delta
            if fp <= 0.1 * delta:
                return y, F64(0.0)
            par_lower = fp / (delta * phider) if phider > 0.0 else F64(0.0)
        else:
            dxnorm = fp = F64(np.inf)
        gnorm = _norm(gt)
        par_upper = gnorm / delta
        if par_upper == 0.0:
            par_upper = DBL_MIN / min(delta, 0.1)
        if par > par_upper:
            par = par_upper
        elif par < par_lower:
            par = par_lower
        if par == 0.0:
            par = gnorm / dxnorm
        it = 0
        while True:
            it += 1
            if par == 0.0:
                par = max(0.001 * par_upper, DBL_MIN)
            if not fac.factor(par):
                return np.full(len(gt), np.nan), F64(par)
            y, dxnorm, phider = fac.solve()
            fp_old = fp
            fp = dxnorm - delta
            if abs(fp) <= 0.1 * delta or (par_lower == 0.0 and fp <= fp_old and fp_old < 0.0) or it == MAX_LMPAR:
                break
            par_c = fp / (delta * phider)
            if fp > 0.0:
                if par > par_lower:
                    par_lower = par
            elif fp < 0.0:
                if par < par_upper:
                    par_upper = par
            par = par + par_c if par + par_c > par_lower else par_lower
    return y, F64(par)


# ---------------------------------------------------------------------------- the fit

def _finite(*vals):
    return all(bool(np.isfinite(v).all()) for v in vals)


def lm(z, init, v, sums=sums, resid=resid, seed=ULP_SEED):
    """lmsder as sg_psf.h restates it, for p = len(init) parameters of the model whose sums(x, z, v, rng)
    and resid(x, z, v, rng) are given (seqpsf_ref passes its own, and its seed of the exp variant).
    Returns dict(x, ff, iters, bad, trace); trace lists every trial step as (outer, inner, accepted)."""
    rng = np.random.default_rng(seed) if v["exp"] == "ulp" else None
    Fac = _QR if v["linalg"] == "qr" else _Chol
    x = np.array(init, dtype=F64)
    n = len(x)
    trace = []
    with np.errstate(all="ignore"):
        a, g, ff, J = sums(x, z, v, rng)
        if not _finite(a, g, ff):
            return dict(x=x, ff=F64(np.nan), iters=0, bad=True, trace=trace)
        diag = np.sqrt(np.diag(a)).copy()
        diag[diag == 0.0] = 1.0
        xn = _norm(diag * x)
        delta = F64(100.0) if xn == 0.0 else 100.0 * xn
        par = F64(0.0)
        first = True
        iters = 0
        for outer in range(1, MAX_ITER + 1):
            iters = outer
            fnorm = np.sqrt(ff)
            if fnorm == 0.0:
                break
            gt = g / diag
            At = a / np.outer(diag, diag)
            fac = Fac(At, gt, J / diag[None, :])
            accepted = False
            for inner in range(MAX_INNER):
                y, par = lmpar(fac, gt, delta, par)
                pnorm = _norm(y)
                if not np.isfinite(pnorm):
                    break
                p = -(y / diag)
                xt = x + p
                if first and pnorm < delta:
                    delta = pnorm
                ff1 = resid(xt, z, v, rng)
                fnorm1 = np.sqrt(ff1)
                actred = F64(-1.0)
                if 0.1 * fnorm1 < fnorm:
                    u = fnorm1 / fnorm
                    actred = 1.0 - u * u
                q = F64(0.0)
                for i in range(n):
                    r = F64(0.0)
                    for j in range(n):
                        r = r + At[i, j] * y[j]
                    q = q + y[i] * r
                t1 = np.sqrt(q if q > 0.0 else F64(0.0)) / fnorm
                t2 = np.sqrt(par) * pnorm / fnorm
                prered = t1 * t1 + t2 * t2 / 0.5
                dirder = -(t1 * t1 + t2 * t2)
                ratio = actred / prered if prered > 0.0 else F64(0.0)
                if ratio > 0.25:
                    if par == 0.0 or ratio >= 0.75:
                        delta = pnorm / 0.5
                        par = par * 0.5
                else:
                    temp = F64(0.5) if actred >= 0.0 else 0.5 * dirder / (dirder + 0.5 * actred)
                    if 0.1 * fnorm1 >= fnorm or temp < 0.1:
                        temp = F64(0.1)
                    delta = temp * min(delta, pnorm / 0.1)
                    par = par / temp
                ok = bool(ratio >= 1e-4)
                trace.append((outer, inner, ok))
                if ok:
                    x = xt
                    a, g, ff, J = sums(x, z, v, rng)
                    if not _finite(a, g, ff):
                        return dict(x=x, ff=ff, iters=iters, bad=True, trace=trace)
                    first = False
                    diag = np.maximum(diag, np.sqrt(np.diag(a)))
                    accepted = True
                    break
            if not accepted:
                trace.append((outer, "no progress"))
                break
            if bool((np.abs(p) < 1e-4 + 1e-4 * np.abs(x)).all()):
                trace.append((outer, "delta test"))
                break
    return dict(x=x, ff=ff, iters=iters, bad=False, trace=trace)


def is_star(r, roundness):
    """is_star (star_finder.c:59-78): 0 for a star, else the number of the failed test"""
    if math.isnan(r["fwhmx"]) or math.isnan(r["fwhmy"]):
        return 1
    if math.isnan(r["x0"]) or math.isnan(r["y0"]):
        return 2
    if math.isnan(r["mag"]):
        return 3
    if r["x0"] <= 0.0 or r["y0"] <= 0.0:
        return 4
    if r["A"] < 0.01:
        return 5
    if r["sx"] > 200 or r["sy"] > 200:
        return 6
    if r["fwhmx"] <= 0.0 or r["fwhmy"] <= 0.0:
        return 7
    if r["fwhmy"] / r["fwhmx"] < roundness:
        return 8
    return 0


def finish(x, ff, intensity, n, r, cx, cy, norm, scales, roundness):
    """psf_minimiz_no_angle :393-409, psf_global_minimisation :636-657, psf_update_units as the two
    factors, is_star, peaker :221-222"""
    with np.errstate(all="ignore"):
        o = dict(B=F64(x[0]), A=F64(x[1]), x0=F64(x[2]), y0=F64(x[3]), sx=F64(x[4]), sy=F64(x[5]))
        o["fwhmx"] = np.sqrt(o["sx"] / 2.0) * FWHM_K
        o["fwhmy"] = np.sqrt(o["sy"] / 2.0) * FWHM_K
        o["mag"] = F64(-2.5) * np.log10(F64(intensity))
        o["rmse"] = np.sqrt(F64(ff) / F64(n))
        o["swap_margin"] = abs(o["sx"] - o["sy"])
        if o["sy"] > o["sx"]:
            o["sx"], o["sy"] = o["sy"], o["sx"]
            o["fwhmx"], o["fwhmy"] = o["fwhmy"], o["fwhmx"]
        o["B"] = o["B"] / F64(norm)
        o["A"] = o["A"] / F64(norm)
        o["rmse"] = o["rmse"] / F64(norm)
        o["xpos"] = F64(cx) + o["x0"] - F64(r) - 1.0
        o["ypos"] = F64(cy) + o["y0"] - F64(r) - 1.0
        o["failed_test"] = 0
        if (not np.isfinite(o["fwhmx"]) or not np.isfinite(o["fwhmy"]) or o["fwhmx"] <= 0.0 or o["fwhmy"] <= 0.0):
            o["status"] = FIT_BAD_FWHM
            return o
        o["fwhmx"] = o["fwhmx"] * F64(scales[0])
        o["fwhmy"] = o["fwhmy"] * F64(scales[1])
        o["failed_test"] = is_star(o, roundness)
        o["status"] = FIT_NOT_STAR if o["failed_test"] else FIT_STAR
    return o


def fit(box, bg, variant="base", cx=0, cy=0, norm=65535.0, scales=(1.0, 1.0), roundness=0.5, init=None):
    """psf_global_minimisation(z, bg, layer, FALSE, FALSE), psf_update_units, is_star and xpos / ypos for
    the box of the candidate (cx, cy): dict(init, status, failed_test, iters, trace, FIELDS...)"""
    v = VARIANTS[variant] if isinstance(variant, str) else variant
    z = np.asarray(box).astype(F64)
    n2 = z.shape[0]
    init = init_literal(box, bg) if init is None else init
    o = dict({k: F64(0.0) for k in FIELDS}, init=init, status=FIT_NOT_ENOUGH_PIXELS, failed_test=0, iters=0,
             trace=[], swap_margin=F64(np.inf))
    if z.size <= NP:
        return o
    res = lm(z, init, v)
    o["iters"], o["trace"] = res["iters"], res["trace"]
    if res["bad"] or not _finite(res["x"], res["ff"]):
        o["status"] = FIT_NONFINITE
        return o
    o.update(finish(res["x"], res["ff"], flux(z, res["x"][0], v), z.size, n2 // 2, cx, cy, norm, scales, roundness))
    return o


# ---------------------------------------------------------------------------- stability and the tail

def _margin_ok(o, roundness, tol):
    """no is_star comparison, nor the swap, within 100 * tol of flipping (relative, denominator max(|v|, 1))"""
    if o["status"] not in (FIT_STAR, FIT_NOT_STAR):
        return True
    m = 100.0 * tol

    def far(vv, thr):
        return abs(float(vv) - thr) > m * max(abs(float(vv)), abs(thr), 1.0)

    checks = [far(o["x0"], 0.0), far(o["y0"], 0.0), far(o["A"], 0.01), far(o["sx"], 200.0), far(o["sy"], 200.0),
              far(o["fwhmx"], 0.0), far(o["fwhmy"], 0.0), float(o["swap_margin"]) > m * max(abs(float(o["sx"])), 1.0)]
    if float(o["fwhmx"]) != 0.0:
        checks.append(far(o["fwhmy"] / o["fwhmx"], roundness))
    return all(checks)


def classify(outs, roundness, tol):
    """outs: {variant: fit result} of one box.  (stable, spread): stable when every variant agrees on
    status, failed_test, iters and the trace and the base has its margins; spread is the largest
    relative difference of a reported field between two variants"""
    base = outs["base"]
    same = all(o["status"] == base["status"] and o["failed_test"] == base["failed_test"] and
               o["iters"] == base["iters"] and o["trace"] == base["trace"] for o in outs.values())
    if not same or not _margin_ok(base, roundness, tol):
        return False, 0.0
    spread = 0.0
    if base["status"] in (FIT_STAR, FIT_NOT_STAR, FIT_BAD_FWHM):
        for k in FIELDS:
            vals = np.array([float(o[k]) for o in outs.values()])
            if not np.isfinite(vals).all():
                if not (np.isnan(vals).all() or (vals == vals[0]).all()):
                    return False, 0.0
                continue
            spread = max(spread, float((vals.max() - vals.min()) / max(np.abs(vals).max(), 1.0)))
    return True, spread


def peaker_tail(plane, cands, r, bg, roundness=0.5, norm=65535.0, scales=(1.0, 1.0), max_stars=50000,
                variants=("base",), tol=None):
    """peaker :200-247 on the stored candidates of one plane, serially.  Returns dict(records = one
    fit result per candidate (base variant, status FIT_OVER_CAP past the cap), stable [n] bool,
    spread, stars = the indices of the accepted candidates sorted by (mag, cand), fits = the records and
    the stable mask before the cap, for cap_stars).  With one variant every box counts as stable."""
    tol = TOL if tol is None else tol
    bx = fsr.boxes(plane, cands, r)
    records, stable, spread = [], [], 0.0
    for n, (x, y) in enumerate(cands):
        init = init_literal(bx[n], bg)
        outs = {name: fit(bx[n], bg, name, x, y, norm, scales, roundness, init=init) for name in variants}
        if "base" not in outs:
            outs["base"] = fit(bx[n], bg, "base", x, y, norm, scales, roundness, init=init)
        st, sp = classify(outs, roundness, tol) if len(outs) > 1 else (True, 0.0)
        records.append(outs["base"])
        stable.append(st)
        if st:
            spread = max(spread, sp)
    fits = (records, np.array(stable, dtype=bool))      # before the cap: what cap_stars takes
    records, stable, stars = cap_stars(records, stable, max_stars, tol)
    return dict(records=records, stable=stable, spread=spread, stars=stars, fits=fits)


def cap_stars(records, stable, max_stars, tol=None):
    """the end of peaker_tail on uncapped fit results (no status FIT_OVER_CAP among them): the cap, the
    sorted star list and the mag pairs too close to order.  Returns (records, stable, stars); the arguments
    are left as they are, so one set of fits serves every max_stars."""
    tol = TOL if tol is None else tol
    records = list(records)
    accepted = [n for n, o in enumerate(records) if o["status"] == FIT_STAR]
    for n in accepted[max_stars:]:
        records[n] = dict(records[n], status=FIT_OVER_CAP)
    kept = accepted[:max_stars]
    stars = sorted(kept, key=lambda n: (float(records[n]["mag"]), n))
    # a neighbouring mag pair within 100 * tol of flipping makes both boxes unstable
    stable = np.array(stable, dtype=bool)
    for a, b in zip(stars, stars[1:]):
        ma, mb = float(records[a]["mag"]), float(records[b]["mag"])
        if abs(ma - mb) <= 100.0 * tol * max(abs(ma), abs(mb), 1.0):
            stable[a] = stable[b] = False
    return records, stable, stars


# ---------------------------------------------------------------------------- GPU test cases
# (shared by tests/test_psf_cpu.py, which holds the conditions the GPU tests rely on, and
# tests/test_gpu_starfit.py)

ALL_VARIANTS = tuple(VARIANTS)
K_SIGMA = 0.5           # sf->sigma of the cases: the narrow stars are low in the smoothed plane

# radius -> (seed, H, W, grid columns, grid rows, fwhm): frames of at most 160 x 160 whose stars sit on
# a jittered grid inside the scan rectangle, so that 30 or more stay separate candidates
STARFIT_CASES = {
    2: (22, 96, 112, 7, 6, 1.6),
    3: (23, 96, 112, 7, 6, 1.8),
    4: (24, 112, 112, 7, 6, 2.0),
    5: (25, 112, 128, 7, 6, 2.2),
    10: (30, 128, 144, 7, 6, 2.5),
    16: (36, 144, 160, 7, 6, 2.8),
    32: (52, 160, 160, 7, 6, 3.0),
}


def starfit_frame(r):
    """a star field like findstar_ref.star_field, plus one star whose centre sits exactly r from the
    image border, one hot pixel beside a star and one star clipped at 65535 with a flat top"""
    seed, H, W, gx, gy, fwhm = STARFIT_CASES[r]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    img = rng.normal(800.0, 12.0, size=(H, W))
    s = fwhm / 2.3548
    cw, ch = (W - 2 * r - 1) / gx, (H - 2 * r - 1) / gy
    cx = np.array([r + (i + 0.5) * cw for j in range(gy) for i in range(gx)]) + rng.uniform(-1.0, 1.0, size=gx * gy)
    cy = np.array([r + (j + 0.5) * ch for j in range(gy) for i in range(gx)]) + rng.uniform(-1.0, 1.0, size=gx * gy)
    amp = rng.uniform(6000, 40000, size=gx * gy)
    first = gx * (gy // 2)                              # the first star of a middle row:
    cx[first], cy[first] = float(r), float(round(cy[first]))   # its centre exactly r from the left border
    amp[first] = 30000.0
    amp[1] = 400000.0                                  # clipped: a flat top at 65535
    for k in range(gx * gy):
        img += amp[k] * np.exp(-((xx - cx[k]) ** 2 + (yy - cy[k]) ** 2) / (2 * s * s))
    img = np.clip(np.rint(img), 0, 65535).astype(np.uint16)
    hx, hy = int(round(cx[2])) + 2, int(round(cy[2]))  # a hot pixel beside star 2
    img[hy, hx] = 60000
    return img


DENSE_CASE = (78, 192, 192, 14, 14, 1.8, 3)     # seed, H, W, grid columns, grid rows, fwhm, radius


def starfit_dense_frame():
    """the construction of starfit_frame without its three special stars, dense enough that one frame
    stores more than two 64-candidate steps of k_starfit_select (tests/test_batches_cpu.py holds the
    counts): for r = 3, k = K_SIGMA"""
    seed, H, W, gx, gy, fwhm, r = DENSE_CASE
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    img = rng.normal(800.0, 12.0, size=(H, W))
    s = fwhm / 2.3548
    cw, ch = (W - 2 * r - 1) / gx, (H - 2 * r - 1) / gy
    cx = np.array([r + (i + 0.5) * cw for j in range(gy) for i in range(gx)]) + rng.uniform(-1.0, 1.0, size=gx * gy)
    cy = np.array([r + (j + 0.5) * ch for j in range(gy) for i in range(gx)]) + rng.uniform(-1.0, 1.0, size=gx * gy)
    amp = rng.uniform(6000, 40000, size=gx * gy)
    for k in range(gx * gy):
        img += amp[k] * np.exp(-((xx - cx[k]) ** 2 + (yy - cy[k]) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16)


def starfit_batch_sequence(nframes):
    """frames [nframes][1][112][128] for a call of more than one chunk of 256: starfit_frame(5), its 180
    degree rotation and an all-zero frame in rotation; frame 256 is the zero frame, frame 257 the
    rotation.  Returns (frames, plane number per frame, the three planes)."""
    a = starfit_frame(5)
    planes = [a, np.ascontiguousarray(a[::-1, ::-1]), np.zeros_like(a)]
    which = [i % 3 for i in range(nframes)]
    which[256:] = [2, 1][:max(nframes - 256, 0)]
    return np.stack([planes[w] for w in which])[:, None], which, planes


def starfit_extra_frames():
    """the further planes tests/test_gpu_starfit.py fits: (plane, radius)"""
    a = starfit_frame(5)
    return [(np.ascontiguousarray(a[::-1, ::-1]), 5), (np.ascontiguousarray(a[::-1]), 5), (starfit_frame(2), 1)]


_cache = {}


def starfit_case(r, roundness=0.5, norm=65535.0, scales=(1.0, 1.0), variants=ALL_VARIANTS):
    """(frame, candidates, threshold record, peaker_tail result) of the case of radius r, computed once"""
    key = (r, roundness, norm, scales, variants)
    if key not in _cache:
        img = starfit_frame(r)
        cands, rec, _ = fsr.candidates(img, K_SIGMA, r)
        tail = peaker_tail(img, cands, r, rec["median"], roundness, norm, scales, variants=variants)
        _cache[key] = (img, cands, rec, tail)
    return _cache[key]
