"""Star matching without a GPU: tests/starmatch_ref.py (the numpy restatement of new_star_match) against its own
literal forms, ground truth and the measured spread behind TOL, and siril-0.9_amd/csrc/sg_starmatch.h with
sg_starmatch_plan.hpp (what k_starmatch runs) built into a stand-alone host program, plainly and under
AddressSanitizer + UBSan, fed every case.  It also holds the conditions tests/test_gpu_starmatch.py relies on."""
import subprocess

import numpy as np
import pytest

import starmatch_host as sh
import starmatch_ref as sr

CLEAN = ("n10", "n19", "n20", "n21", "n40", "rot180", "rot30_scale105", "scale130", "mirror", "persp", "n2000", "n2001",
         "ref_fewer")
WITH_TRUTH = CLEAN + ("outliers30", "crowded", "collinear4", "ransac_out")


# ------------------------------------------------------------------ the oracle's own checks

def test_winners_closed_form_equals_literal():
    rng = np.random.default_rng(5)
    for num in (6, 10, 19, 20):
        for hi in (2, 4, 40):            # few distinct values: ties everywhere
            for _ in range(20):
                vm = rng.integers(0, hi, (num, num))
                assert sr.winners(vm) == sr.winners_literal(vm)
    vm = np.zeros((20, 20), dtype=np.int64)
    assert sr.winners(vm) == sr.winners_literal(vm) == ([0] * 20, [-1] * 20, [-1] * 20)


def test_match_lists_tie_rules():
    """constructed exact ties: dist^2 values that are equal bit for bit"""
    B = np.array([[10.0, 10.0, 0.0], [16.0, 10.0, 1.0], [13.0, 13.0, 2.0], [13.0, 7.0, 3.0], [50.0, 50.0, 4.0], [56.0, 50.0, 5.0]])
    # A0 is 3 px from B0 and B1 (tie: the smaller x, B0) and sqrt(9) from B2, B3 (x = 13 lies between)
    ax, ay = np.array([13.0, 7.0, 53.0, 53.0]), np.array([10.0, 10.0, 50.0, 50.0])
    # A1 is 3 px from B0 as well: stage 2's tie between A0 and A1 goes to A0; A2 and A3 coincide, 3 px from B4 and B5
    want = ([0, 2], [0, 4])
    assert sr.match_lists(ax, ay, B) == want
    assert sr.match_lists_literal(ax, ay, B) == want
    # equal x in B: the tie in x goes to the smaller id
    B2 = np.array([[20.0, 13.0, 0.0], [20.0, 7.0, 1.0]])
    assert sr.match_lists(np.array([20.0]), np.array([10.0]), B2) == sr.match_lists_literal(np.array([20.0]), np.array([10.0]), B2) == ([0], [0])
    # the radius is open: a star exactly 5 px away is no candidate, one on the box's edge inside the circle is
    B3 = np.array([[5.0, 0.0, 0.0], [0.0, 4.999, 1.0]])
    assert sr.match_lists(np.array([0.0]), np.array([0.0]), B3) == sr.match_lists_literal(np.array([0.0]), np.array([0.0]), B3) == ([0], [1])
    rng = np.random.default_rng(11)
    for _ in range(30):                  # integer grids: many exact ties
        P = rng.integers(0, 12, (25, 2)).astype(float)
        Bq = np.concatenate([rng.integers(0, 12, (25, 2)).astype(float), np.arange(25.0)[:, None]], axis=1)
        assert sr.match_lists(P[:, 0], P[:, 1], Bq) == sr.match_lists_literal(P[:, 0], P[:, 1], Bq)


def test_generator_and_jacobi():
    r = sr.Rng()
    first = [r.next() for _ in range(3)]
    s = 0xFFFFFFFFFFFFFFFF
    for v in first:
        s = (s & 0xFFFFFFFF) * 4164903690 + (s >> 32)
        assert v == s & 0xFFFFFFFF and s < 2 ** 64
    rng = np.random.default_rng(3)
    for n in (8, 9):
        m = rng.normal(size=(n, n))
        m = m @ m.T
        w, V = sr.jacobi(m.tolist())
        V = np.array(V)
        assert np.allclose(V @ np.diag(w) @ V.T, m, atol=1e-12 * np.abs(m).max())
        assert np.allclose(np.sort(w), np.linalg.eigvalsh(m), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_case_results(name):
    """statuses and counts the cases were built for (match_frame asserts the literal forms on every frame)"""
    c = sr.case(name)
    r = c["results"]
    if name == "nine_ref":
        assert r is None
        return
    if name == "mixed70":
        st = [o["status"] for o in r]
        assert len(r) == 70 and st[sr.MIXED_REF] == sr.REFERENCE and all(st[f] == sr.EXCLUDED for f in (0, 17, 18, 44, 69))
        assert {sr.OK, sr.FEW_STARS, sr.NO_TRANS, sr.NO_RECALC} <= set(st) or {sr.OK, sr.FEW_STARS, sr.NO_TRANS} <= set(st)
        assert sum(s == sr.OK for s in st) >= 40 and any(o["scale_retry"] for o in r if o["status"] == sr.OK)
        return
    o = r[0]
    assert r[1]["status"] == sr.REFERENCE
    want_status = {"unrelated": (sr.NO_TRANS, sr.NO_RECALC, sr.NO_HOMOGRAPHY), "nine": (sr.FEW_STARS,)}.get(name, (sr.OK,))
    assert o["status"] in want_status, o["status"]
    if name == "n10":
        assert o["nbright"] == 10
    if name in ("n19", "n20", "n21", "n40"):
        assert o["nbright"] == min(int(name[1:]), 20)
    if name == "rot30_scale105":
        assert o["scale_retry"] == 0
    if name == "scale130":
        assert o["scale_retry"] == 1
    if name == "persp":
        assert o["hom"][6] != 0.0 and o["hom"][7] != 0.0
    if name == "outliers30":
        assert 10 <= o["npairs"] < o["nbpoints"]
    if name == "crowded":
        assert o["npairs"] == 55         # 60 stars, 3 dropped by stage 2, 2 by stage 1
    if name == "collinear4":
        assert o["subset_rejects"][0] > 0
    if name == "ransac_out":
        assert o["ransac_iters"] > 1 and o["inliers"] < o["npairs"]
    if name in ("n2000", "n2001"):
        assert o["nbpoints"] == 2000 and r[1]["nbpoints"] == 2000
    if name == "ref_fewer":
        assert o["nbpoints"] == 50


@pytest.mark.parametrize("name", WITH_TRUTH)
def test_ground_truth(name):
    A, B, T, sigma, clean = sr.build(name)
    o = sr.case(name)["results"][0]
    n = o["nbpoints"]
    pa, pb = o["pairs"]
    if name in CLEAN:
        assert clean and pa == pb and len(pa) >= 0.75 * n, "a pair that is no true correspondence, or too few pairs"
    got = sr.project(o["hom"], A[:n, :2])
    want = sr.project(T, A[:n, :2])
    err = np.sqrt(((got - want) ** 2).sum(axis=1))
    inside = (want[:, 0] > 0) & (want[:, 0] < 4096) & (want[:, 1] > -100) & (want[:, 1] < 4096)
    print(name, "max error", err[inside].max(), "bound", 3 * sigma)
    assert err[inside].max() <= 3 * sigma


def test_spread_within_tol():
    worst, where = 0.0, None
    stable = total = 0
    for name in sr.CASES:
        c = sr.case(name)
        if c["results"] is None:
            continue
        stable += int(c["stable"].sum())
        total += len(c["stable"])
        if c["spread"] > worst:
            worst, where = c["spread"], name
    print("spread", worst, "in", where, "stable", stable, "of", total)
    assert worst <= sr.SPREAD_MEASURED == sr.TOL / 16
    assert stable >= 0.9 * total


# ------------------------------------------------------------------ the host program

def _check_program(exe, tmp_path, names):
    for name in names:
        c = sr.case(name)
        nstars, stars = sh.star_arrays(c["lists"], c["fwhm"])
        out = sh.run(exe, tmp_path, nstars, stars, c["ref_image"], c["included"])
        if c["results"] is None:
            assert out["plan"][0] == -1 and "not enough stars in the reference" in out["plan"][4] and not out["frames"]
            continue
        assert out["plan"][0] == 0 and len(out["frames"]) == len(c["results"])
        worst = 0.0
        for f, (g, w) in enumerate(zip(out["frames"], c["results"])):
            worst = max(worst, sh.compare(g, w, bool(c["stable"][f]), (name, f)))
        print(name, "worst relative difference", worst, "ms", out["ms"])
        hom, action, slot, total = sr.warp_plan(c["results"])
        assert out["warp"] == (0, total, action.tolist(), slot.tolist()), name


def test_host_program(tmp_path):
    _check_program(sh.build(tmp_path), tmp_path, sorted(sr.CASES))


def test_host_program_sanitized(tmp_path):
    """the same program under AddressSanitizer + UBSan (host code only, run stand-alone)"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", *sh.SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not installed")
    _check_program(sh.build(tmp_path, sh.SAN, "-O0"), tmp_path, sorted(sr.CASES))


def test_warp_plan_bookkeeping():
    """sr.warp_plan against the loop's counters written out, on mixed70"""
    res = sr.case("mixed70")["results"]
    hom, action, slot, total = sr.warp_plan(res)
    failed = skipped = written = 0
    for frame, r in enumerate(res):
        if r["status"] == sr.EXCLUDED:
            skipped += 1
            assert action[frame] == sr.WARP_SKIP
            continue
        if frame != sr.MIXED_REF and r["status"] != sr.OK:
            failed += 1
            assert action[frame] == sr.WARP_SKIP
            continue
        assert slot[frame] == frame - failed - skipped == written
        assert action[frame] == (sr.WARP_COPY if frame == sr.MIXED_REF else sr.WARP_APPLY) and hom[frame].tolist() == list(r["hom"])
        written += 1
    assert total == written == 70 - failed - skipped and failed > 0 and skipped == 5


# ------------------------------------------------------------------ the plan header

def _plan(tmp_path, exe, lists, ref, included=None, **kw):
    nstars, stars = sh.star_arrays(lists, max_stars=kw.pop("alloc", None))
    return sh.run(exe, tmp_path, kw.pop("nstars", nstars), stars, ref, included, **kw)["plan"]


def test_plan_refusals_and_lds(tmp_path):
    exe = sh.build(tmp_path)
    A, B = sr.build("n40")[:2]
    ok = _plan(tmp_path, exe, [A, B], 1)
    assert ok[0] == 0 and ok[2] == 1 and ok[3] == 40
    big = sr.case("n2000")
    nstars, stars = sh.star_arrays(big["lists"])
    full = sh.run(exe, tmp_path, nstars, stars, 1)["plan"]
    print("LDS bytes at 2000 stars", full[1])
    assert full[0] == 0 and full[3] == 2000 and full[1] <= 163840
    SIZE, GENERIC = -2, -1
    assert _plan(tmp_path, exe, [A, B], 1, nframes=0)[0] == SIZE
    assert _plan(tmp_path, exe, [A, B], 1, max_stars=0)[0] == SIZE
    assert _plan(tmp_path, exe, [A, B], 1, alloc=50001)[0] == SIZE
    assert _plan(tmp_path, exe, [A, B], 2)[0] == GENERIC and _plan(tmp_path, exe, [A, B], -1)[0] == GENERIC
    assert _plan(tmp_path, exe, [A, B], 1, included=[1, 0])[0] == GENERIC
    assert _plan(tmp_path, exe, [A, B], 1, nstars=np.array([41, 40], dtype=np.int32))[0] == GENERIC
    assert _plan(tmp_path, exe, [A, B], 1, nstars=np.array([-1, 40], dtype=np.int32))[0] == GENERIC
    for col in range(3):
        bad = A.copy()
        bad[7, col] = [np.nan, np.inf, -np.inf][col]
        assert _plan(tmp_path, exe, [bad, B], 1)[0] == GENERIC
        assert _plan(tmp_path, exe, [A, bad], 1)[0] == GENERIC
        assert _plan(tmp_path, exe, [bad, B], 1, included=[0, 1])[0] == 0          # not among the stars used
    late = np.concatenate([A, A[:5]])
    late[42, 0] = np.nan                                                           # beyond nbpoints = 40
    assert _plan(tmp_path, exe, [late, B], 1)[0] == 0
