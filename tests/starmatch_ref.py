"""numpy fp64 restatement of Siril 0.9's new_star_match and of the frame loop of register_star_alignment
around it (src/registration/matching/match.c:125-389, atpmatch.c, misc.c:333; src/opencv/opencv.cpp:207-240,
findHomography/fundam.cpp:63-291, modelest.cpp:73-188, 277-361, calibration.cpp:95-300;
src/registration/registration.c:55, 589-755; src/algos/star_finder.c:353-367), the oracle of sg_starmatch
(include/sirilgpu.h) and of siril-0.9_amd/csrc/sg_starmatch.h.

  piece                                           here
  stars_to_triangles, set_triangle, prune         bright, triangles
  make_vote_matrix, find_ba_triangle              votes (the literal search: it can step over one A triangle)
  top_vote_getters                                winners_literal, winners (the closed form, asserted equal)
  calc_trans_linear, gauss_matrix, gauss_pivot    calc_trans, gauss
  iter_trans, find_percentile                     iter_trans
  atFindTrans and match.c's second try            find_trans
  atApplyTrans, atMatchLists                      match_lists_literal, match_lists (closed form, asserted equal)
  atCalcRMS, atRecalcTrans                        calc_rms, match_frame
  cvCalculH .. runRANSAC, getSubset, checkSubset  homography, ransac, get_subset, check_subset, Rng
  runKernel, refine (CvLevMarq)                   kernel, refine
  cvEigenVV, cvSVD + cvSVBkSb                     jacobi (one cyclic Jacobi solver for both; see below)
  the frame loop, FWHM_average                    starmatch
  the loop's failed / skipped bookkeeping         warp_plan

Contracts where the reference leaves the result open or reads past its data:
  - sort_star_by_mag, sort_triangle_array, sort_star_by_x are qsorts: ties go to the smaller original index.
  - match lists: stage 1 is per A star the argmin of dist^2 over its candidates, ties to the smaller (x, id) of B;
    stage 2 per B star the argmin over the A stars that chose it, ties to the smaller A id; the pairs come out in
    ascending B id.  match_lists_literal materialises the lists with stable sorts and is asserted equal.
  - iter_trans(RECALC_NO) with fewer than 6 winners left after the cut at 2 votes makes calc_trans read winner
    slots that hold 1-vote cells or -1 (an out-of-bounds read): that is a failure here.
  - prune_triangle_array with no triangle at ba <= 0.8 trips an assert in the reference: no triangles here.
  - OpenCV's cvEigenVV and cvSVD are not in the tree: both are one cyclic Jacobi eigen-solver for symmetric
    matrices (JtJ is symmetric, so its SVD is its eigen-decomposition).  CvLevMarq's lambda = exp(l * log(10)) is
    taken from a table of powers of ten and pow(1 - ep, 4) is two squarings, so that no libm function but log
    and sqrt decides a bit.  Parity with an OpenCV build is unpinned, as for the warp and ECC.

Tolerance, by the method of seqpsf_ref: VARIANTS differ only in the order of the sums over pairs (the 3 x 3 normal
equations, atCalcRMS, runKernel's centroids, scales and LtL on the inliers, refine's JtJ, JtErr, errNorm):
sequential as the reference, pairwise, and `tree`, what the kernel and the host program do: item i belongs to
virtual lane i % 256, a lane adds its items in ascending order, and the 256 partial sums are folded by halving
(p[v] += p[v + s], s = 128 .. 1).  The 4-point sample kernels of RANSAC are sequential in every variant.
  - A frame is branch-stable when all variants agree on every integer field but lm_iters and on the pairs, and
    cvRound's argument in cvRANSACUpdateNumIters is not within 1e-6 of a half.  lm_iters is left out: refine stops
    at a relative step below DBL_EPSILON, so its count hangs on the last bit of the sums and differs between the
    variants on most frames, while the homographies they reach lie within the spread.  Against the `tree` variant,
    whose order is the product's, the host program and the kernel are held to every integer field, lm_iters too.
  - SPREAD_MEASURED is the largest relative difference (denominator max(|v|, 1)) of hom, trans0, trans, sig, sx,
    sy over the stable frames of every case; TOL = 16 x it.  tests/test_starmatch_cpu.py recomputes and holds it.
"""
import math

import numpy as np

F64 = np.float64
DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
FLT_EPSILON = 1.1920928955078125e-07

MAX_STARS_FITTED = 2000
AT_MATCH_MINPAIRS = 10
AT_MATCH_NBRIGHT = 20
AT_TRIANGLE_RADIUS = 0.002
AT_MATCH_RADIUS = 5.0
AT_MATCH_MAXDIST = 50.0
AT_MATCH_RATIO = 0.8
AT_MATCH_REQUIRE_LINEAR = 3
AT_MATCH_STARTN_LINEAR = 6
AT_MATCH_PERCENTILE = 0.70
AT_MATCH_NSIGMA = 3.0
AT_MATCH_MAXITER = 3
AT_MATCH_HALTSIGMA = 1.0e-12
AT_MATCH_MINVOTES = 2
ONE_STDEV_PERCENTILE = 0.683
MATRIX_TOL = 1.0e-12
RANSAC_THRESHOLD = 3.0
RANSAC_CONFIDENCE = 0.995
RANSAC_MAX_ITERS = 2000
RANSAC_ATTEMPTS = 300
LM_MAX_ITERS = 10
JACOBI_SWEEPS = 50
LANES = 256                         # SGM_LANES of sg_starmatch.h

OK, REFERENCE, EXCLUDED, FEW_STARS, NO_TRANS, NO_RECALC, NO_HOMOGRAPHY = range(7)
WARP_SKIP, WARP_APPLY, WARP_COPY = 0, 1, 2

# measured by tests/test_starmatch_cpu.py::test_spread_within_tol over CASES (see the docstring)
SPREAD_MEASURED = 1.3e-6       # measured 1.2905e-06 (n2000: hom, refine ends at its 10 iterations), rounded up
TOL = 16 * SPREAD_MEASURED

INT_FIELDS = ("status", "nbpoints", "nbright", "scale_retry", "nwinners", "npairs", "nr_recalc", "inliers",
              "ransac_iters", "lm_iters")
FP_FIELDS = ("trans0", "trans", "sig", "sx", "sy", "hom")
VARIANTS = ("seq", "pairwise", "tree")


# ---------------------------------------------------------------------------- sums

def total(terms, variant):
    """the sums over the rows of terms [n][K] as the variant adds them; every order starts from +0.0"""
    t = np.asarray(terms, dtype=F64)
    if t.ndim == 1:
        t = t[:, None]
    n, k = t.shape
    zero = np.zeros((1, k))
    with np.errstate(all="ignore"):
        if variant == "seq":
            return np.cumsum(np.concatenate([zero, t]), axis=0)[-1]
        if variant == "pairwise":
            def rec(a):
                if len(a) <= 1:
                    return np.cumsum(np.concatenate([zero, a]), axis=0)[-1]
                return rec(a[:len(a) // 2]) + rec(a[len(a) // 2:])
            return rec(t)
        pad = (-n) % LANES
        th = np.concatenate([t, np.zeros((pad, k))]).reshape(-1, LANES, k)
        part = np.cumsum(np.concatenate([np.zeros((1, LANES, k)), th]), axis=0)[-1]
        s = LANES // 2
        while s >= 1:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
        return part[0].copy()


# ---------------------------------------------------------------------------- triangles and votes

def stable_order(keys):
    return np.argsort(np.asarray(keys), kind="stable")


def bright(stars, nbright):
    """the original indices of the nbright smallest mags, ascending (ties by index)"""
    return stable_order(stars[:, 2])[:nbright]


def triangles(x, y):
    """all C(n, 3) triangles of the bright stars in creation order, then sorted by ba and pruned:
    (ba, ca, a_length, a_index, b_index, c_index) arrays of the kept ones, ascending ba"""
    n = len(x)
    d = [[0.0] * n for _ in range(n)]
    for i in range(n - 1):
        for j in range(i + 1, n):
            dx, dy = x[i] - x[j], y[i] - y[j]
            d[i][j] = d[j][i] = math.sqrt(dx * dx + dy * dy)
    out = []
    for s1 in range(n - 2):
        for s2 in range(s1 + 1, n - 1):
            for s3 in range(s2 + 1, n):
                d12, d23, d13 = d[s1][s2], d[s2][s3], d[s1][s3]
                if d12 >= d23 and d12 >= d13:
                    ai, a = s3, d12
                    if d23 >= d13:
                        bi, b, ci, c = s1, d23, s2, d13
                    else:
                        bi, b, ci, c = s2, d13, s1, d23
                elif d23 > d12 and d23 >= d13:
                    ai, a = s1, d23
                    if d12 > d13:
                        bi, b, ci, c = s3, d12, s2, d13
                    else:
                        bi, b, ci, c = s2, d13, s3, d12
                else:
                    ai, a = s2, d13
                    if d12 > d23:
                        bi, b, ci, c = s3, d12, s1, d23
                    else:
                        bi, b, ci, c = s1, d23, s3, d12
                ba, ca = (b / a, c / a) if a > 0.0 else (1.0, 1.0)
                out.append((ba, ca, a, ai, bi, ci))
    order = stable_order([t[0] for t in out])
    srt = [out[i] for i in order]
    keep = -1
    for i in range(len(srt) - 1, -1, -1):
        if srt[i][0] <= AT_MATCH_RATIO:
            keep = i
            break
    return srt[:max(keep, 0)]       # numtriangles = i: the last triangle at or below the ratio goes too


def find_ba(tri, ba0):
    """find_ba_triangle as written"""
    num = len(tri)
    top, bottom = 0, max(num - 1, 0)
    while bottom - top > 2:
        mid = (top + bottom) // 2
        if tri[mid][0] < ba0:
            top = mid
        else:
            bottom = mid
    return bottom if tri[top][0] < ba0 else top


def votes(tri_a, tri_b, nbright, min_scale, max_scale):
    vm = np.zeros((nbright, nbright), dtype=np.int64)
    rad2 = AT_TRIANGLE_RADIUS * AT_TRIANGLE_RADIUS
    if not tri_a:
        return vm
    for tb in tri_b:
        ba_b, ca_b = tb[0], tb[1]
        ba_min, ba_max = ba_b - AT_TRIANGLE_RADIUS, ba_b + AT_TRIANGLE_RADIUS
        for i in range(find_ba(tri_a, ba_min), len(tri_a)):
            ta = tri_a[i]
            if ta[0] > ba_max:
                break
            if (ta[0] - ba_b) * (ta[0] - ba_b) + (ta[1] - ca_b) * (ta[1] - ca_b) < rad2:
                if min_scale != -1:
                    ratio = ta[2] / tb[2]
                    if ratio < min_scale or ratio > max_scale:
                        continue
                vm[ta[3], tb[3]] += 1
                vm[ta[4], tb[4]] += 1
                vm[ta[5], tb[5]] += 1
    return vm


def winners_literal(vm):
    """top_vote_getters as written: (votes, index A, index B) lists of len(vm)"""
    num = len(vm)
    wv, wa, wb = [0] * num, [-1] * num, [-1] * num
    for i in range(num):
        for j in range(num):
            if vm[i][j] > wv[num - 1]:
                for k in range(num):
                    if vm[i][j] > wv[k]:
                        for l in range(num - 2, k - 1, -1):
                            wv[l + 1], wa[l + 1], wb[l + 1] = wv[l], wa[l], wb[l]
                        wv[k], wa[k], wb[k] = int(vm[i][j]), i, j
                        break
    return wv, wa, wb


def winners(vm):
    """the closed form: the cells by descending votes, ties in row-major order, cut at num; cells without a
    vote never enter"""
    num = len(vm)
    flat = np.asarray(vm).reshape(-1)
    order = stable_order(-flat)[:num]
    wv, wa, wb = [0] * num, [-1] * num, [-1] * num
    for k, c in enumerate(order):
        if flat[c] > 0:
            wv[k], wa[k], wb[k] = int(flat[c]), int(c) // num, int(c) % num
    return wv, wa, wb


# ---------------------------------------------------------------------------- TRANS

def gauss(m, v):
    """gauss_matrix with gauss_pivot on copies: the solution or None"""
    num = len(v)
    m = [list(map(float, r)) for r in m]
    v = list(map(float, v))
    big = []
    for i in range(num):
        b = max(abs(e) for e in m[i])
        if b == 0.0:
            return None
        big.append(b)
    for i in range(num - 1):
        pr, bg = i, abs(m[i][i] / big[i])
        for r in range(i + 1, num):
            o = abs(m[r][i] / big[r])
            if o > bg:
                bg, pr = o, r
        if pr != i:
            for c in range(i, num):
                m[pr][c], m[i][c] = m[i][c], m[pr][c]
            v[pr], v[i] = v[i], v[pr]
            big[pr], big[i] = big[i], big[pr]
        if abs(m[i][i] / big[i]) < MATRIX_TOL:
            return None
        for j in range(i + 1, num):
            f = m[j][i] / m[i][i]
            for k in range(i + 1, num):
                m[j][k] -= f * m[i][k]
            v[j] -= f * v[i]
    if abs(m[num - 1][num - 1] / big[num - 1]) < MATRIX_TOL:
        return None
    sol = [0.0] * num
    sol[num - 1] = v[num - 1] / m[num - 1][num - 1]
    for i in range(num - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, num):
            s += m[i][j] * sol[j]
        sol[i] = (v[i] - s) / m[i][i]
    return sol


def calc_trans(ax, ay, bx, by, variant):
    """calc_trans_linear over the given pairs: TRANS (a .. f) or None"""
    one = np.ones_like(ax)
    t = total(np.stack([one, ax, bx, ay, by, ax * ax, ay * ay, ax * bx, ax * ay, ax * by, ay * bx, ay * by], axis=1), variant)
    s, sx1, sx2, sy1, sy2, sx1sq, sy1sq, sx1x2, sx1y1, sx1y2, sy1x2, sy1y2 = [float(e) for e in t]
    m = [[sx1sq, sx1y1, sx1], [sx1y1, sy1sq, sy1], [sx1, sy1, s]]
    abc = gauss(m, [sx1x2, sy1x2, sx2])
    if abc is None:
        return None
    d_e_f = gauss(m, [sx1y2, sy1y2, sy2])
    if d_e_f is None:
        return None
    return [abc[2], abc[0], abc[1], d_e_f[2], d_e_f[0], d_e_f[1]]


def apply_trans(tr, x, y):
    return tr[0] + tr[1] * x + tr[2] * y, tr[3] + tr[4] * x + tr[5] * y


def find_percentile(srt, num, perc):
    index = int(math.floor(num * perc + 0.5))
    if index >= num:
        index = num - 1
    return float(srt[index])


def iter_trans(A, B, pa, pb, recalc, variant):
    """iter_trans over the pairs (pa[i], pb[i]) of original indices: (ok, trans or None, nr, sig)"""
    pa, pb = np.array(pa, dtype=np.int64), np.array(pb, dtype=np.int64)
    nbright = len(pa)
    if nbright < AT_MATCH_REQUIRE_LINEAR:
        return False, None, 0, 0.0
    initial = nbright if recalc else AT_MATCH_STARTN_LINEAR
    if initial > nbright:
        return False, None, 0, 0.0        # the reference reads past the winners here (see the docstring)
    tr = calc_trans(A[pa[:initial], 0], A[pa[:initial], 1], B[pb[:initial], 0], B[pb[:initial], 1], variant)
    if tr is None:
        return False, None, 0, 0.0
    nr, ok, it = nbright, True, 0
    max_dist2 = AT_MATCH_MAXDIST * AT_MATCH_MAXDIST
    srt = np.zeros(0)
    while it < AT_MATCH_MAXITER:
        nx, ny = apply_trans(tr, A[pa, 0], A[pa, 1])
        xd, yd = nx - B[pb, 0], ny - B[pb, 1]
        d2 = xd * xd + yd * yd
        srt = np.sort(d2)
        keep = ~(d2 > max_dist2)
        nb = int((~keep).sum())
        pa, pb, d2 = pa[keep], pb[keep], d2[keep]
        nr = len(pa)
        if nr < 2:
            if nr == 0:
                return False, None, 0, 0.0
            sigma = 0.0
        else:
            sigma = find_percentile(srt, nr, AT_MATCH_PERCENTILE)
        if sigma <= AT_MATCH_HALTSIGMA:
            break
        keep = ~(d2 > AT_MATCH_NSIGMA * sigma)
        nb += int((~keep).sum())
        pa, pb = pa[keep], pb[keep]
        nr = len(pa)
        if nb == 0:
            break
        if nr < AT_MATCH_REQUIRE_LINEAR:
            ok = False
            break
        tr = calc_trans(A[pa, 0], A[pa, 1], B[pb, 0], B[pb, 1], variant)
        if tr is None:
            return False, None, 0, 0.0
        it += 1
    sig = find_percentile(srt, nr, ONE_STDEV_PERCENTILE)
    return ok, tr, nr, sig


def find_trans(A, B, variant, stages=None):
    """atFindTrans, and once more without the scale test if it fails: (ok, trans, nr, nbright, scale_retry)"""
    n = min(len(A), len(B))
    nbright = min(AT_MATCH_NBRIGHT, n)
    if n < AT_MATCH_STARTN_LINEAR:
        return False, None, 0, nbright, 0
    ia, ib = bright(A, nbright), bright(B, nbright)
    ta = triangles([float(v) for v in A[ia, 0]], [float(v) for v in A[ia, 1]])
    tb = triangles([float(v) for v in B[ib, 0]], [float(v) for v in B[ib, 1]])
    for retry, (lo, hi) in enumerate(((0.9, 1.1), (-1.0, -1.0))):
        vm = votes(ta, tb, nbright, lo, hi)
        wv, wa, wb = winners(vm)
        assert (wv, wa, wb) == winners_literal(vm), "top_vote_getters: the closed form differs from the literal form"
        nw = nbright
        for i in range(nbright):
            if wv[i] < AT_MATCH_MINVOTES:
                nw = i
                break
        if stages is not None:
            stages.append(dict(votes=vm, winners=(wv[:nw], wa[:nw], wb[:nw]), ntri=(len(ta), len(tb))))
        ok, tr, nr, _ = iter_trans(A, B, [ia[k] for k in wa[:nw]], [ib[k] for k in wb[:nw]], False, variant)
        if ok:
            return True, tr, nr, nbright, retry
    return False, None, 0, nbright, 1


# ---------------------------------------------------------------------------- match lists

def _candidates(ax, ay, B):
    bx, by = B[:, 0][None, :], B[:, 1][None, :]
    Ax, Ay = ax[:, None], ay[:, None]
    r = AT_MATCH_RADIUS
    box = ~((bx < Ax - r) | (bx > Ax + r) | (by < Ay - r) | (by > Ay + r))
    dx, dy = Ax - bx, Ay - by
    d = dx * dx + dy * dy
    return box & (d < r * r), d


def match_lists(ax, ay, B):
    """the closed form: (A ids, B ids) of the matched pairs, ascending B id"""
    cand, d = _candidates(ax, ay, B)
    na, nb = cand.shape
    xpos = np.empty(nb, dtype=np.int64)
    xpos[np.lexsort((np.arange(nb), B[:, 0]))] = np.arange(nb)      # position in the x-sorted B, ties by id
    choice = np.full(na, -1, dtype=np.int64)
    cd = np.zeros(na)
    for a in range(na):
        js = np.nonzero(cand[a])[0]
        if len(js):
            j = js[np.lexsort((xpos[js], d[a, js]))[0]]
            choice[a], cd[a] = j, d[a, j]
    pa, pb = [], []
    for b in range(nb):
        who = np.nonzero(choice == b)[0]
        if len(who):
            pa.append(int(who[np.lexsort((who, cd[who]))[0]]))
            pb.append(b)
    return pa, pb


def _remove_repeated(l1, l2, dist):
    """remove_repeated_elements over parallel lists; l1 holds the ids that repeat"""
    o1, o2, od = [], [], []
    for a, b, dd in zip(l1, l2, dist):
        if o1 and o1[-1] == a:
            if dd < od[-1]:
                o1[-1], o2[-1], od[-1] = a, b, dd
        else:
            o1.append(a)
            o2.append(b)
            od.append(dd)
    return o1, o2, od


def match_lists_literal(ax, ay, B):
    """match_arrays_slow as written, its qsorts stable: both arrays sorted by x, every candidate listed, sorted
    by A id, the repeats removed, sorted by B id, the repeats removed"""
    cand, d = _candidates(ax, ay, B)
    oa = np.lexsort((np.arange(len(ax)), ax))
    ob = np.lexsort((np.arange(len(B)), B[:, 0]))
    J, K, D = [], [], []
    for a in oa:
        for b in ob:
            if cand[a, b]:
                J.append(int(a))
                K.append(int(b))
                D.append(float(d[a, b]))
    o = stable_order(J)
    J, K, D = _remove_repeated([J[i] for i in o], [K[i] for i in o], [D[i] for i in o])
    o = stable_order(K)
    K, J, D = _remove_repeated([K[i] for i in o], [J[i] for i in o], [D[i] for i in o])
    return J, K


def calc_rms(ax, ay, bx, by, variant):
    """atCalcRMS: (sx, sy); a* are the transformed matched A"""
    n = len(ax)
    if n == 0:
        return 0.0, 0.0
    dx, dy = bx - ax, by - ay
    t = total(np.stack([dx * dx, dy * dy], axis=1), variant)
    xms, yms = float(t[0]) / n, float(t[1]) / n
    dx2, dy2 = dx * dx, dy * dy
    keep = (dx2 < 9 * xms) & (dy2 < 9 * yms)
    t = total(np.stack([np.where(keep, dx2, 0.0), np.where(keep, dy2, 0.0)], axis=1), variant)
    ntoss = int((~keep).sum())
    sx = 0.0 if t[0] <= 0.0 else math.sqrt(float(t[0]) / (n - ntoss))
    sy = 0.0 if t[1] <= 0.0 else math.sqrt(float(t[1]) / (n - ntoss))
    return sx, sy


# ---------------------------------------------------------------------------- the eigen-solver

def jacobi(a):
    """cyclic Jacobi on a symmetric n x n matrix (lists): (eigenvalues [n], V [n][n], column k the k-th vector).
    Rows p < q in order; a rotation is skipped where 100 |a_pq| vanishes beside both diagonal entries; at most
    JACOBI_SWEEPS sweeps, ended by a sweep that finds every off-diagonal entry zero."""
    n = len(a)
    a = [list(map(float, r)) for r in a]
    v = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _ in range(JACOBI_SWEEPS):
        off = 0.0
        for p in range(n - 1):
            for q in range(p + 1, n):
                off += abs(a[p][q])
        if off == 0.0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                g = 100.0 * abs(apq)
                if abs(a[p][p]) + g == abs(a[p][p]) and abs(a[q][q]) + g == abs(a[q][q]):
                    a[p][q] = a[q][p] = 0.0
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                tau = s / (1.0 + c)
                a[p][p] -= t * apq
                a[q][q] += t * apq
                a[p][q] = a[q][p] = 0.0
                for r in range(n):
                    if r != p and r != q:
                        arp, arq = a[r][p], a[r][q]
                        a[r][p] = a[p][r] = arp - s * (arq + tau * arp)
                        a[r][q] = a[q][r] = arq + s * (arp - tau * arq)
                for r in range(n):
                    vrp, vrq = v[r][p], v[r][q]
                    v[r][p] = vrp - s * (vrq + tau * vrp)
                    v[r][q] = vrq + s * (vrp - tau * vrq)
    return [a[i][i] for i in range(n)], v


# ---------------------------------------------------------------------------- the homography

class Rng:
    """OpenCV's cvRandInt (core/types_c.h, CV_RNG_COEFF): multiply-with-carry, 64-bit state, the low 32 bits"""
    def __init__(self):
        self.state = 0xFFFFFFFFFFFFFFFF          # cvRNG(-1)

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF


def check_subset(px, py):
    count = len(px)
    if count <= 2:
        return True
    for i in range(count):
        for j in range(i):
            dx1, dy1 = px[j] - px[i], py[j] - py[i]
            for k in range(j):
                dx2, dy2 = px[k] - px[i], py[k] - py[i]
                if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                    return False
    return True


def get_subset(rng, Mx, My, mx, my, rejects=None):
    """getSubset(.., 300) with checkPartialSubsets off: the 4 indices or None; rejects[0] counts the samples
    checkSubset refused"""
    count = len(Mx)
    iters = 0
    while iters < RANSAC_ATTEMPTS:
        idx = []
        while len(idx) < 4:
            k = rng.next() % count
            if k not in idx:
                idx.append(k)
        if check_subset([Mx[k] for k in idx], [My[k] for k in idx]) and check_subset([mx[k] for k in idx], [my[k] for k in idx]):
            return idx
        iters += 1
        if rejects is not None:
            rejects[0] += 1
    return None


def kernel(Mx, My, mx, my, variant):
    """runKernel: H [9] or None; M = A (object), m = B (image)"""
    Mx, My, mx, my = [np.asarray(e, dtype=F64) for e in (Mx, My, mx, my)]
    count = len(Mx)
    t = total(np.stack([mx, my, Mx, My], axis=1), variant)
    cmx, cmy, cMx, cMy = [float(e) / count for e in t]
    t = total(np.stack([np.abs(mx - cmx), np.abs(my - cmy), np.abs(Mx - cMx), np.abs(My - cMy)], axis=1), variant)
    smx, smy, sMx, sMy = [float(e) for e in t]
    if abs(smx) < DBL_EPSILON or abs(smy) < DBL_EPSILON or abs(sMx) < DBL_EPSILON or abs(sMy) < DBL_EPSILON:
        return None
    smx, smy, sMx, sMy = count / smx, count / smy, count / sMx, count / sMy
    x, y = (mx - cmx) * smx, (my - cmy) * smy
    X, Y = (Mx - cMx) * sMx, (My - cMy) * sMy
    one, zero = np.ones(count), np.zeros(count)
    Lx = [X, Y, one, zero, zero, zero, -x * X, -x * Y, -x]
    Ly = [zero, zero, zero, X, Y, one, -y * X, -y * Y, -y]
    cols = [Lx[j] * Lx[k] + Ly[j] * Ly[k] for j in range(9) for k in range(j, 9)]
    t = total(np.stack(cols, axis=1), variant)
    LtL = [[0.0] * 9 for _ in range(9)]
    n = 0
    for j in range(9):
        for k in range(j, 9):
            LtL[j][k] = LtL[k][j] = float(t[n])
            n += 1
    w, V = jacobi(LtL)
    small = 0
    for k in range(1, 9):
        if w[k] < w[small]:
            small = k
    h0 = [V[r][small] for r in range(9)]
    inv = [1.0 / smx, 0.0, cmx, 0.0, 1.0 / smy, cmy, 0.0, 0.0, 1.0]
    n2 = [sMx, 0.0, -cMx * sMx, 0.0, sMy, -cMy * sMy, 0.0, 0.0, 1.0]

    def mul(a, b):
        return [a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]
    h = mul(mul(inv, h0), n2)
    s = float(F64(1.0) / F64(h[8]))
    return [e * s for e in h]


def reproj_errors(H, Mx, My, mx, my):
    ww = 1.0 / (H[6] * Mx + H[7] * My + 1.0)
    dx = (H[0] * Mx + H[1] * My + H[2]) * ww - mx
    dy = (H[3] * Mx + H[4] * My + H[5]) * ww - my
    return (dx * dx + dy * dy).astype(np.float32)


def update_num_iters(p, ep, max_iters, margins):
    """cvRANSACUpdateNumIters with 4 model points"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    w = 1.0 - ep
    denom = 1.0 - (w * w) * (w * w)
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    margins.append(num / denom)
    return int(np.rint(num / denom))        # cvRound: to nearest, ties to even


def ransac(Mx, My, mx, my, variant, margins, rejects=None):
    """runRANSAC: (found, H, mask, iterations run)"""
    count = len(Mx)
    rng = Rng()
    niters, best, H, mask = RANSAC_MAX_ITERS, 0, None, np.ones(count, dtype=bool)
    it = 0
    while it < niters:
        idx = get_subset(rng, Mx, My, mx, my, rejects)
        if idx is None:
            if it == 0:
                return False, None, mask, 0
            break
        it += 1
        h = kernel(Mx[idx], My[idx], mx[idx], my[idx], "seq")
        if h is None:
            continue
        tm = reproj_errors(h, Mx, My, mx, my) <= RANSAC_THRESHOLD * RANSAC_THRESHOLD
        good = int(tm.sum())
        if good > max(best, 3):
            mask, H, best = tm, h, good
            niters = update_num_iters(RANSAC_CONFIDENCE, (count - good) / count, niters, margins)
    return best > 0, H, mask, it


LAMBDA = {k: float("1e%d" % k) for k in range(-16, 18)}


def refine(H, Mx, My, mx, my, variant):
    """CvHomographyEstimator::refine through CvLevMarq::updateAlt / step: (H [9], iterations)"""
    param = [float(e) for e in H[:8]]

    def evaluate(h, want_j):
        ww = h[6] * Mx + h[7] * My + 1.0
        with np.errstate(all="ignore"):
            ww = np.where(np.abs(ww) > DBL_EPSILON, 1.0 / ww, 0.0)
        xi = (h[0] * Mx + h[1] * My + h[2]) * ww
        yi = (h[3] * Mx + h[4] * My + h[5]) * ww
        e0, e1 = xi - mx, yi - my
        cols = []
        if want_j:
            z = np.zeros(len(Mx))
            J0 = [Mx * ww, My * ww, ww, z, z, z, -Mx * ww * xi, -My * ww * xi]
            J1 = [z, z, z, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi]
            cols = [J0[j] * J0[k] + J1[j] * J1[k] for j in range(8) for k in range(j, 8)]
            cols += [J0[j] * e0 + J1[j] * e1 for j in range(8)]
        cols.append(e0 * e0 + e1 * e1)
        t = [float(e) for e in total(np.stack(cols, axis=1), variant)]
        if not want_j:
            return None, None, t[0]
        JtJ = [[0.0] * 8 for _ in range(8)]
        n = 0
        for j in range(8):
            for k in range(j, 8):
                JtJ[j][k] = JtJ[k][j] = t[n]
                n += 1
        return JtJ, t[36:44], t[44]

    def step(JtJ, JtErr, prev, lg):
        lam = LAMBDA[lg]
        N = [r[:] for r in JtJ]
        for i in range(8):
            N[i][i] *= 1.0 + lam
        w, V = jacobi(N)
        thr = 0.0
        for i in range(8):
            thr += abs(w[i])
        thr *= 2 * DBL_EPSILON
        delta = [0.0] * 8
        for k in range(8):
            if abs(w[k]) > thr:
                dot = 0.0
                for r in range(8):
                    dot += V[r][k] * JtErr[r]
                dot /= w[k]
                for r in range(8):
                    delta[r] += V[r][k] * dot
        return [prev[i] - delta[i] for i in range(8)]

    lg, iters = -3, 0
    JtJ, JtErr, err = evaluate(param, True)
    while True:
        prev = param
        param = step(JtJ, JtErr, prev, lg)
        prev_err = err
        _, _, err = evaluate(param, False)
        while err > prev_err:
            lg += 1
            if lg > 16:
                break
            param = step(JtJ, JtErr, prev, lg)
            _, _, err = evaluate(param, False)
        lg = max(lg - 1, -16)
        iters += 1
        if iters >= LM_MAX_ITERS:
            break
        num = den = 0.0
        for i in range(8):
            num += (param[i] - prev[i]) * (param[i] - prev[i])
            den += prev[i] * prev[i]
        if F64(math.sqrt(num)) / F64(math.sqrt(den)) < DBL_EPSILON:
            break
        JtJ, JtErr, _ = evaluate(param, True)
    return param + [float(H[8])], iters


def homography(ax, ay, bx, by, variant, margins, rejects=None):
    """cvCalculH on matched pairs: (ok, H [9], inliers, ransac iterations, lm iterations)"""
    Mx, My, mx, my = [np.asarray(e, dtype=np.float32).astype(F64) for e in (ax, ay, bx, by)]
    count = len(Mx)
    with np.errstate(all="ignore"):
        if count == 4:
            H = kernel(Mx, My, mx, my, variant)
            if H is None or not any(e != 0.0 for e in H):
                return False, [0.0] * 9, 0, 0, 0
            return True, H, 4, 0, 0
        found, H, mask, its = ransac(Mx, My, mx, my, variant, margins, rejects)
        if not found:
            return False, [0.0] * 9, 0, its, 0
        Mx, My, mx, my = Mx[mask], My[mask], mx[mask], my[mask]
        h2 = kernel(Mx, My, mx, my, variant)
        if h2 is not None:
            H = h2
        H, lm = refine(H, Mx, My, mx, my, variant)
        if not any(e != 0.0 for e in H):
            return False, [0.0] * 9, 0, its, lm
    return True, H, int(mask.sum()), its, lm


# ---------------------------------------------------------------------------- a frame, a sequence

def clear_result(status):
    return dict(status=status, nbpoints=0, nbright=0, scale_retry=0, nwinners=0, npairs=0, nr_recalc=0, inliers=0,
                ransac_iters=0, lm_iters=0, trans0=[0.0] * 6, trans=[0.0] * 6, sig=0.0, sx=0.0, sy=0.0, hom=[0.0] * 9,
                fwhmx=np.float32(0), fwhmy=np.float32(0), shiftx=0.0, shifty=0.0, pairs=([], []), margins=[],
                subset_rejects=[0])


def match_frame(A, B, variant="seq", check=True):
    """new_star_match(A, B, n = len(A) = len(B)): A, B [n][3] = (xpos, ypos, mag)"""
    A, B = np.asarray(A, dtype=F64), np.asarray(B, dtype=F64)
    o = clear_result(NO_TRANS)
    o["nbpoints"] = len(A)
    ok, tr, nr, o["nbright"], o["scale_retry"] = find_trans(A, B, variant)
    if not ok:
        return o
    o["trans0"], o["nwinners"] = list(tr), nr
    tx, ty = apply_trans(tr, A[:, 0], A[:, 1])
    pa, pb = match_lists(tx, ty, B)
    if check:
        assert (pa, pb) == match_lists_literal(tx, ty, B), "atMatchLists: the closed form differs from the literal form"
    o["pairs"], o["npairs"] = (pa, pb), len(pa)
    o["sx"], o["sy"] = calc_rms(tx[pa], ty[pa], B[pb, 0], B[pb, 1], variant)
    o["status"] = NO_RECALC
    if len(pa) < AT_MATCH_STARTN_LINEAR:
        return o
    ok, tr2, nr2, sig = iter_trans(A, B, pa, pb, True, variant)
    if not ok:
        return o
    o["trans"], o["nr_recalc"], o["sig"] = list(tr2), nr2, sig
    o["status"] = NO_HOMOGRAPHY
    ok, H, o["inliers"], o["ransac_iters"], o["lm_iters"] = homography(A[pa, 0], A[pa, 1], B[pb, 0], B[pb, 1], variant, o["margins"],
                                                                            o["subset_rejects"])
    if not ok:
        return o
    o["hom"], o["status"] = list(H), OK
    o["shiftx"], o["shifty"] = H[2], -H[5]
    return o


def fwhm_average(fw, n):
    """FWHM_average: float sums in order"""
    sx = sy = np.float32(0.0)
    for i in range(n):
        sx = np.float32(sx + np.float32(fw[i][0]))
        sy = np.float32(sy + np.float32(fw[i][1]))
    return np.float32(sx / np.float32(n)), np.float32(sy / np.float32(n))


def starmatch(lists, ref_image=0, included=None, variant="seq", fwhm=None, cache=None):
    """the frame loop: lists[f] = [n_f][3]; fwhm[f] = [n_f][2] or None.  None when the reference has fewer
    than 10 stars (the whole call fails)."""
    ref = np.asarray(lists[ref_image], dtype=F64)
    if len(ref) < AT_MATCH_MINPAIRS:
        return None
    fitted = min(len(ref), MAX_STARS_FITTED)
    out = []
    for f, L in enumerate(lists):
        L = np.asarray(L, dtype=F64).reshape(-1, 3)
        if included is not None and not included[f]:
            out.append(clear_result(EXCLUDED))
            continue
        if f == ref_image:
            o = clear_result(REFERENCE)
            o["nbpoints"] = fitted
            o["hom"] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        elif len(L) < AT_MATCH_MINPAIRS:
            out.append(clear_result(FEW_STARS))
            continue
        else:
            n = min(len(L), fitted)
            key = (L[:n].tobytes(), ref[:n].tobytes(), variant)
            if cache is not None and key in cache:
                o = dict(cache[key])
            else:
                o = match_frame(L[:n], ref[:n], variant)
                if cache is not None:
                    cache[key] = dict(o)
        if fwhm is not None and o["status"] in (OK, REFERENCE):
            o["fwhmx"], o["fwhmy"] = fwhm_average(fwhm[f], o["nbpoints"])
        out.append(o)
    return out


def warp_plan(results):
    """the loop's bookkeeping (:653-755): (hom [n][9], action [n], out_slot [n], new_total)"""
    n = len(results)
    hom, action, slot = np.zeros((n, 9)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    failed = skipped = 0
    for f, r in enumerate(results):
        if r["status"] == EXCLUDED:
            skipped += 1
        elif r["status"] in (OK, REFERENCE):
            action[f] = WARP_COPY if r["status"] == REFERENCE else WARP_APPLY
            hom[f] = r["hom"]
            slot[f] = f - failed - skipped
        else:
            failed += 1
    return hom, action, slot, n - failed - skipped


# ---------------------------------------------------------------------------- stability

def classify(outs):
    """outs: {variant: result} of one frame -> (stable, spread)"""
    base = outs["seq"]
    for o in outs.values():
        if any(o[k] != base[k] for k in INT_FIELDS if k != "lm_iters") or o["pairs"] != base["pairs"]:
            return False, 0.0
        if any(abs(abs(m - math.floor(m)) - 0.5) < 1e-6 for m in o["margins"]):
            return False, 0.0
    spread = 0.0
    for k in FP_FIELDS:
        vals = np.array([np.atleast_1d(np.asarray(o[k], dtype=F64)) for o in outs.values()])
        den = np.maximum(np.abs(vals).max(axis=0), 1.0)
        spread = max(spread, float(((vals.max(axis=0) - vals.min(axis=0)) / den).max()))
    return True, spread


# ---------------------------------------------------------------------------- cases
# Star lists are (xpos, ypos, mag) rows in ascending mag, as sg_findstar_fit returns them.  A scene is n stars on a
# jittered grid (no two closer than 0.3 cells, so a clean case has no second candidate inside the match radius)
# with distinct mags; the frame's list A is the scene, the reference's list B = T(A) + Gaussian noise of `sigma`.

def scene(n, seed, size=1000.0):
    rng = np.random.default_rng(seed)
    g = int(math.ceil(math.sqrt(n * 1.3)))
    cell = size / g
    cells = rng.permutation(g * g)[:n]
    x = (cells % g + rng.uniform(0.15, 0.85, n)) * cell
    y = (cells // g + rng.uniform(0.15, 0.85, n)) * cell
    mag = np.sort(rng.uniform(-12.0, -2.0, n)) + np.arange(n) * 1e-9
    return np.stack([x, y, mag], axis=1)


def project(T, P):
    T = np.asarray(T, dtype=F64).reshape(3, 3)
    w = T[2, 0] * P[:, 0] + T[2, 1] * P[:, 1] + T[2, 2]
    return np.stack([(T[0, 0] * P[:, 0] + T[0, 1] * P[:, 1] + T[0, 2]) / w, (T[1, 0] * P[:, 0] + T[1, 1] * P[:, 1] + T[1, 2]) / w], axis=1)


def similarity(deg, scale, tx, ty, mirror=False, c=500.0):
    a = math.radians(deg)
    m = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]) * scale
    if mirror:
        m = m @ np.array([[-1.0, 0.0], [0.0, 1.0]])
    t = np.array([tx + c, ty + c]) - m @ np.array([c, c])
    return np.array([[m[0, 0], m[0, 1], t[0]], [m[1, 0], m[1, 1], t[1]], [0.0, 0.0, 1.0]])


def pair_lists(n, seed, T, sigma=0.05, size=1000.0, outliers=0.0, nref=None):
    """(A [n][3], B [nref or n][3], truth): truth[i] = the index in B of A's star i, or -1"""
    total_n = max(n, nref or n)
    S = scene(total_n, seed, size)
    rng = np.random.default_rng(seed + 7)
    Bp = project(T, S[:, :2]) + rng.normal(0.0, sigma, (total_n, 2))
    A, B = S[:n].copy(), np.concatenate([Bp, S[:, 2:3]], axis=1)[:nref or n]
    truth = np.where(np.arange(n) < len(B), np.arange(n), -1)
    if outliers > 0.0:
        k = int(round(n * outliers))
        pick = rng.permutation(n)[:k]
        A[pick, :2] = rng.uniform(0.0, size, (k, 2))
        truth[pick] = -1
        pickb = rng.permutation(len(B))[:int(round(len(B) * outliers))]
        B[pickb, :2] = rng.uniform(0.0, size, (len(pickb), 2))
        truth[np.isin(truth, pickb)] = -1
    return A, B, truth


SHIFT = similarity(0.0, 1.0, 12.3, -7.6)
SIGMA = 0.05


def _build(name):
    """(A, B, truth homography or None, sigma, clean)"""
    if name in ("n10", "n19", "n20", "n21", "n40"):
        n = int(name[1:])
        A, B, _ = pair_lists(n, 100 + n, SHIFT)
        return A, B, SHIFT, SIGMA, True
    if name == "rot180":
        T = similarity(180.0, 1.0, 3.0, 4.0)
    elif name == "rot30_scale105":
        T = similarity(30.0, 1.05, -20.0, 11.0)
    elif name == "scale130":
        T = similarity(5.0, 1.30, 6.0, -9.0)
    elif name == "mirror":
        T = similarity(10.0, 1.0, 5.0, 5.0, mirror=True)
    elif name == "persp":
        T = similarity(3.0, 1.0, 8.0, -4.0)
        T[2, 0], T[2, 1] = 2.0e-5, -1.5e-5
    else:
        T = None
    if T is not None:
        A, B, _ = pair_lists(60, sum(map(ord, name)), T)
        return A, B, T, SIGMA, True
    if name == "outliers30":
        A, B, _ = pair_lists(90, 301, SHIFT, outliers=1.0 / 3.0)
        return A, B, SHIFT, SIGMA, False
    if name == "unrelated":
        return scene(60, 401), scene(60, 402), None, 0.0, False
    if name == "nine":
        A, B, _ = pair_lists(40, 501, SHIFT)
        return A[:9], B, None, 0.0, False
    if name == "nine_ref":
        A, B, _ = pair_lists(40, 502, SHIFT)
        return A, B[:9], None, 0.0, False
    if name == "crowded":
        # stars 3 px apart in A near one B star, and two B stars 3 px apart near one A star
        A, B, _ = pair_lists(60, 601, SHIFT, sigma=0.0)
        A, B = A.copy(), B.copy()
        for i, j in ((30, 31), (40, 41), (50, 51)):
            A[j, :2] = A[i, :2] + (3.0, 0.25 * (i - 40))       # both transform to within 5 px of B[i]
            B[j, :2] = B[i, :2] + (100.0, 100.0)               # B[j] moves away: A[j] has only B[i]
        for i, j in ((33, 34), (43, 44)):
            B[j, :2] = B[i, :2] + (0.5, 3.0)
            A[j, :2] = A[i, :2] + (-90.0, 70.0)
        return A, B, SHIFT, SIGMA, False
    if name == "collinear4":
        # most stars on one grid line: samples of 4 keep failing checkSubset
        A, B, _ = pair_lists(30, 701, SHIFT, sigma=0.0)
        A, B = A.copy(), B.copy()
        line = [4] + list(range(10, 30))       # with 30 pairs the generator's first two samples draw three of these
        A[line, 1] = 400.0
        A[line, 0] = 30.0 + 44.0 * np.arange(21) + np.random.default_rng(702).uniform(0.0, 25.0, 21)
        B[:, :2] = project(SHIFT, A[:, :2])
        return A, B, SHIFT, 0.01, False
    if name == "ransac_out":
        A, B, _ = pair_lists(100, 801, SHIFT)
        B = B.copy()
        B[20::4, 0] += 4.0                                     # a fifth of the stars, none of the 20 brightest, sits 4 px off
        return A, B, SHIFT, SIGMA, False
    if name in ("n2000", "n2001"):
        n = int(name[1:])
        A, B, _ = pair_lists(n, 901, SHIFT, size=4096.0, nref=2500)
        return A, B, SHIFT, SIGMA, True
    if name == "ref_fewer":
        A, B, _ = pair_lists(300, 951, SHIFT, nref=50)
        return A, B, SHIFT, SIGMA, True
    raise KeyError(name)


PAIR_CASES = ("n10", "n19", "n20", "n21", "n40", "rot180", "rot30_scale105", "scale130", "mirror", "persp", "outliers30",
              "unrelated", "nine", "nine_ref", "crowded", "collinear4", "ransac_out", "n2000", "n2001", "ref_fewer")
MIXED = ("n40", "rot180", "rot30_scale105", "scale130", "mirror", "persp", "outliers30", "unrelated", "nine", "crowded",
         "ransac_out", "n21", "n19")
MIXED_REF = 5
CASES = {name: dict(kind="pair") for name in PAIR_CASES}
CASES["mixed70"] = dict(kind="sequence")

_built, _results, _cache = {}, {}, {}


def build(name):
    if name not in _built:
        b = _build(name)
        for a in b[:2]:
            a.setflags(write=False)
        _built[name] = b
    return _built[name]


def case_lists(name):
    """(lists, ref_image, included, fwhm): a pair case is the sequence [A, B] with the reference last"""
    if CASES[name]["kind"] == "pair":
        A, B = build(name)[:2]
        lists, ref, inc = [A, B], 1, None
    else:
        # 70 frames of 60-star lists against one reference: every frame is the reference scene under another map
        ref_scene = scene(60, 1234)
        rng = np.random.default_rng(4321)
        lists, inc = [], []
        for f in range(70):
            if f == MIXED_REF:
                lists.append(ref_scene)
                inc.append(1)
                continue
            kind = f % 7
            T = similarity([0.0, 180.0, 30.0, 5.0, 10.0, -3.0, 0.0][kind], [1.0, 1.0, 1.05, 1.30, 1.0, 1.0, 1.0][kind],
                           float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20)), mirror=kind == 4)
            P = project(np.linalg.inv(T), ref_scene[:, :2]) + rng.normal(0.0, SIGMA, (60, 2))
            L = np.concatenate([P, ref_scene[:, 2:3]], axis=1)
            if kind == 6:
                L = scene(60, 5000 + f) if f % 2 else L[:9]       # unrelated stars, or too few
            if f % 10 == 3:
                L = L[rng.permutation(60)[:45]]
                L = L[np.argsort(L[:, 2], kind="stable")]         # some stars missing
            lists.append(L)
            inc.append(0 if f in (0, 17, 18, 44, 69) else 1)
        ref = MIXED_REF
    frng = np.random.default_rng(99)
    fwhm = [frng.uniform(2.0, 5.0, (len(L), 2)) for L in lists]
    return lists, ref, inc, fwhm


def case(name):
    """the case's lists, arguments and results, computed once: dict(lists, ref_image, included, fwhm, results (the
    `tree` variant, None when the call fails), stable [N], spread)"""
    if name in _results:
        return _results[name]
    lists, ref, inc, fwhm = case_lists(name)
    runs = {v: starmatch(lists, ref, inc, v, fwhm, _cache) for v in VARIANTS}
    res = dict(lists=lists, ref_image=ref, included=inc, fwhm=fwhm, results=runs["tree"], stable=None, spread=0.0)
    if runs["tree"] is not None:
        stable = []
        for f in range(len(lists)):
            st, sp = classify({v: runs[v][f] for v in VARIANTS})
            stable.append(st)
            if st:
                res["spread"] = max(res["spread"], sp)
        res["stable"] = np.array(stable)
    _results[name] = res
    return res
