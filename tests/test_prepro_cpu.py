"""Sequence preprocessing without a GPU: tests/prepro_ref.py's literal forms against its rule forms
(random inputs and every edge), hand-worked answers, and the host-only plan
(siril-0.9_amd/csrc/sg_prepro_plan.hpp) built as a stand-alone host program and compared with
prepro_ref: level, dark statistics, thresholds, deviant list, derived masters, the schedule's
equivalence to the sequential loop, the noise rows and the golden-section state machine."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import prepro_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include <string>
#include "sg_prepro_plan.hpp"

static FILE *in;
template <typename T> static std::vector<T> rd(size_t n) {
	std::vector<T> v(n);
	if (n && fread(v.data(), sizeof(T), n, in) != n) { printf("short input\n"); exit(3); }
	return v;
}
template <typename T> static void wr(const std::string &path, const std::vector<T> &v) {
	FILE *f = fopen(path.c_str(), "wb");
	if (!f) exit(4);
	if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
	fclose(f);
}

int main(int argc, char **argv) {
	if (argc < 3) return 2;
	in = fopen(argv[1], "rb");
	if (!in) return 2;
	const std::string out = argv[2];
	const std::vector<int32_t> h = rd<int32_t>(5);
	const int W = h[0], H = h[1], C = h[2], flags = h[3], nfr = h[4];
	const float norm = rd<float>(1)[0];
	const std::vector<double> sig = rd<double>(2);
	const size_t npix = W > 0 && H > 0 ? (size_t)W * H : 0, total = C > 0 ? npix * C : 0;
	std::vector<uint16_t> off, dark, flat;
	if (flags & 1) off = rd<uint16_t>(total);
	if (flags & 2) dark = rd<uint16_t>(total);
	if (flags & 4) flat = rd<uint16_t>(total);
	sg_prepro_desc d;
	memset(&d, 0, sizeof d);
	d.width = W; d.height = H; d.nb_layers = C;
	d.offset = (flags & 1) ? off.data() : nullptr;
	d.dark = (flags & 2) ? dark.data() : nullptr;
	d.flat = (flags & 4) ? flat.data() : nullptr;
	d.dark_optimization = !!(flags & 8);
	d.cosmetic = !!(flags & 16);
	d.is_cfa = !!(flags & 32);
	d.autolevel = !!(flags & 64);
	d.normalisation = norm;
	d.cosme_sigma[0] = sig[0]; d.cosme_sigma[1] = sig[1];
	SgPreproPlan p;
	const int rc = sg_prepro_plan(&d, p);
	printf("rc %d\nerr %s\n", rc, p.err);
	if (rc == SG_OK) {
		printf("level %a\nflat_mean %a\nsigma %a\nmedian %a\ntcold %a\nthot %a\n", (double)p.level, p.flat_mean,
				p.dark_sigma, p.dark_median, p.thres_cold, p.thres_hot);
		printf("icold %ld\nihot %ld\napplies %d\nncomp %ld\nlongest %u\n", (long)p.icold, (long)p.ihot, p.cosme_applies,
				(long)p.comp_start.size() - 1, p.longest);
		wr(out + ".list", p.list);
		wr(out + ".items", p.items);
		wr(out + ".flat1", p.flat1);
		wr(out + ".darkfit", p.darkfit);
		/* the correction through the schedule (components in REVERSE order, list order inside: any
		 * component order must do) and through the sequential loop */
		std::vector<uint16_t> sched, seq;
		for (int f = 0; f < nfr; f++) {
			std::vector<uint16_t> a = rd<uint16_t>(npix), b = a;
			for (size_t c = p.comp_start.size() - 1; c-- > 0;)
				for (uint32_t it = p.comp_start[c]; it < p.comp_start[c + 1]; it++) {
					const uint32_t pix = p.items[it] & ~SGP_COLD;
					a[pix] = sgp_correct_one(a.data(), W, H, (int)(pix % W), (int)(pix / W), !!(p.items[it] & SGP_COLD), p.is_cfa);
				}
			for (uint32_t e : p.list) {
				const uint32_t pix = e & ~SGP_COLD;
				b[pix] = sgp_correct_one(b.data(), W, H, (int)(pix % W), (int)(pix / W), !!(e & SGP_COLD), p.is_cfa);
			}
			sched.insert(sched.end(), a.begin(), a.end());
			seq.insert(seq.end(), b.begin(), b.end());
		}
		wr(out + ".sched", sched);
		wr(out + ".seq", seq);
	} else
		for (int f = 0; f < nfr; f++)
			rd<uint16_t>(npix);
	/* noise of max(raw - rtw(dark * k), 0) */
	const int nk = rd<int32_t>(1)[0];
	const std::vector<double> ks = rd<double>(nk);
	if (nk > 0) {
		const std::vector<uint16_t> raw = rd<uint16_t>(npix);
		std::vector<double> rows;
		for (double k : ks) {
			std::vector<double> sd(H, 0.0);
			std::vector<int> fl(H, 0);
			for (int y = 0; y < H; y++)
				fl[y] = W < 3 ? 0 : sgp_noise_row(raw.data() + (size_t)y * W, dark.data() + (size_t)y * W, W, k, &sd[y]);
			printf("noise %a\n", sgp_noise_finish(sd.data(), fl.data(), H, W));
			for (int y = 0; y < H; y++) { rows.push_back(sd[y]); rows.push_back(fl[y]); }
		}
		wr(out + ".rows", rows);
	}
	/* the search fed with recorded objective values */
	const int nseq = rd<int32_t>(1)[0];
	for (int s = 0; s < nseq; s++) {
		const int n = rd<int32_t>(1)[0];
		const std::vector<double> vals = rd<double>(n);
		SgGolden g;
		g.init(0.0, 2.0, 1E-3);
		size_t at = 0;
		while (!g.done) {
			double kk[2];
			const int w = g.want(kk);
			if (at + w > vals.size()) { printf("gshort\n"); break; }
			for (int j = 0; j < w; j++) printf("gk %a\n", kk[j]);
			g.feed(vals.data() + at);
			at += w;
		}
		printf("gres %a %d %zu\n", g.result(), g.iters, at);
	}
	return 0;
}
'''


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    """the plan header as a stand-alone host program, under AddressSanitizer + UBSan when their
    runtimes are installed (host code only, never loaded into Python)"""
    tmp = tmp_path_factory.mktemp("prepro_plan")
    src = tmp / "prepro_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp / "prepro_plan_check"
    base = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC, str(src), "-o", str(exe), "-lm"]
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(exe)], capture_output=True).returncode != 2:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    return exe, tmp


_case_no = [0]


def run_plan(plan_exe, W, H, C, offset=None, dark=None, flat=None, optd=False, cosme=False, cfa=False, autolevel=False,
             norm=1.0, sig=(-1.0, -1.0), frames=(), ks=(), raw=None, seqs=()):
    exe, tmp = plan_exe
    _case_no[0] += 1
    base = tmp / f"case{_case_no[0]}"
    flags = (offset is not None) | (dark is not None) << 1 | (flat is not None) << 2 | optd << 3 | cosme << 4 | cfa << 5 | autolevel << 6
    blob = struct.pack("<5i", W, H, C, int(flags), len(frames)) + struct.pack("<f", norm) + struct.pack("<2d", *sig)
    for m in (offset, dark, flat):
        if m is not None:
            blob += np.ascontiguousarray(m, dtype=np.uint16).tobytes()
    for f in frames:
        blob += np.ascontiguousarray(f, dtype=np.uint16).tobytes()
    blob += struct.pack("<i", len(ks)) + np.asarray(ks, dtype=np.float64).tobytes()
    if len(ks):
        blob += np.ascontiguousarray(raw, dtype=np.uint16).tobytes()
    blob += struct.pack("<i", len(seqs))
    for s in seqs:
        blob += struct.pack("<i", len(s)) + np.asarray(s, dtype=np.float64).tobytes()
    (tmp / "in.bin").write_bytes(blob)
    r = subprocess.run([str(exe), str(tmp / "in.bin"), str(base)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {"noise": [], "gk": [], "gres": []}
    for line in r.stdout.splitlines():
        key, _, val = line.partition(" ")
        if key in ("noise", "gk"):
            out[key].append(float.fromhex(val))
        elif key == "gres":
            a, b, c = val.split()
            out[key].append((float.fromhex(a), int(b), int(c)))
        elif key in ("rc", "icold", "ihot", "applies", "ncomp", "longest"):
            out[key] = int(val)
        elif key == "err":
            out[key] = val
        else:
            out[key] = float.fromhex(val)
    for ext, dt in (("list", np.uint32), ("items", np.uint32), ("flat1", np.uint16), ("darkfit", np.uint16),
                    ("sched", np.uint16), ("seq", np.uint16), ("rows", np.float64)):
        path = str(base) + "." + ext
        if os.path.exists(path):
            out[ext] = np.fromfile(path, dtype=dt)
    return out


def same(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


# ------------------------------------------------------------------ literal == rule

def test_median24_literal_equals_rule():
    rng = np.random.default_rng(1)
    for n in range(0, 25):
        for _ in range(40):
            kind = rng.integers(4)
            vals = [int(v) for v in (rng.integers(0, 65536, n) if kind == 0 else rng.integers(0, 3, n) if kind == 1
                                     else rng.integers(65530, 65536, n) if kind == 2 else np.full(n, rng.integers(65536)))]
            assert pr.median24_literal(vals) == pr.median24_rule(vals), (n, vals)


def test_median24_hand_worked():
    # 5x5, cold centre, neighbours 1..24: the largest (24) is dropped and a zero comes in:
    # {0, 1, ..., 23}, even count, median (11 + 12) / 2 = 11.5 -> 12
    vals = [v for v in range(1, 25)]
    f = np.zeros((5, 5), dtype=np.uint16)
    f.reshape(-1)[[i for i in range(25) if i != 12]] = vals
    assert pr._neighbours(f, 2, 2, True, False) == vals
    assert pr.median24_literal(vals) == 12 and pr.median24_rule(vals) == 12
    assert pr.cosmetic_literal(f, [(2, 2, True)], False)[2, 2] == 12
    # cold corner: n = 8 neighbours {10, 20, ..., 80} -> {0, 10, ..., 70}, median (30 + 40) / 2 = 35
    c = np.zeros((5, 5), dtype=np.uint16)
    c[0:3, 0:3] = np.array([[0, 10, 20], [30, 40, 50], [60, 70, 80]])
    assert len(pr._neighbours(c, 0, 0, True, False)) == 8
    assert pr.cosmetic_literal(c, [(0, 0, True)], False)[0, 0] == 35
    assert pr.cosmetic_rule(c, [(0, 0, True)], False)[0, 0] == 35
    # hot corner: n = 3 neighbours {10, 30, 40}: 80 / 3 = 26.67 -> 27
    assert pr.cosmetic_literal(c, [(0, 0, False)], False)[0, 0] == 27
    # CFA hot pixel on the left edge (x = 0, y = 2) of a 5x5: same-colour neighbours at step 2:
    # (0,0) (2,0) (2,2) (0,4) (2,4) -> 5 values
    e = np.arange(25, dtype=np.uint16).reshape(5, 5) * 100
    vals = pr._neighbours(e, 0, 2, False, True)
    assert vals == [0, 200, 1200, 2000, 2200]
    assert pr.cosmetic_literal(e, [(0, 2, False)], True)[2, 0] == 1120      # 5600 / 5


def test_cosmetic_literal_equals_rule():
    for seed, (H, W) in enumerate([(9, 7), (16, 12), (24, 31), (1, 9), (9, 1), (2, 2), (1, 1)]):
        rng = np.random.default_rng(seed)
        for cfa in (False, True):
            for density in (0.02, 0.2, 1.0):
                mask = rng.random((H, W)) < density
                dev = [(int(x), int(y), bool(rng.random() < 0.4)) for y, x in zip(*np.nonzero(mask))]
                frame = rng.integers(0, 65536, size=(H, W)).astype(np.uint16)
                want = pr.cosmetic_literal(frame, dev, cfa)
                assert np.array_equal(pr.cosmetic_rule(frame, dev, cfa), want), (H, W, cfa, density)
                n = len(pr.components(dev, W, H, cfa))
                assert np.array_equal(pr.cosmetic_rule(frame, dev, cfa, order=list(range(n))[::-1]), want)


def test_noise_row_literal_equals_rule():
    seen = set()
    for name, row, passes in pr.edge_rows():
        ran = []
        a, b = pr.noise_row_literal(row), pr.noise_row_rule(row, ran)
        assert (a is None) == (b is None), name
        if a is not None:
            assert same(a, b), (name, a, b)
            seen.add(ran[0])
            if passes is not None:
                assert ran[0] == passes, (name, ran)
    assert seen >= {0, 1, 2, 3}, seen      # every pass count occurs
    rng = np.random.default_rng(6)
    for i in range(300):
        W = int(rng.integers(1, 200))
        row = rng.normal(500, 1 + 30 * rng.random(), W).clip(0, 65535).astype(np.int64)
        row[rng.random(W) < rng.random() * 0.5] = 0
        if rng.random() < 0.5:
            row[rng.integers(0, W, 3)] = rng.integers(0, 65536, 3)
        a, b = pr.noise_row_literal(row), pr.noise_row_rule(row)
        assert (a is None) == (b is None) and (a is None or same(a, b) or (math.isnan(a) and math.isnan(b))), (i, a, b)


def test_noise_row_hand_worked():
    # non-zero pixels 10 11 10 11 ... (40 of them) with one 1000 in the middle and zeros between.
    # differences: 37 of +-1 and the pair (11 - 1000, 1000 - 11) = (-989, 989): n = 39
    row = []
    for i in range(40):
        row += [10 + (i & 1), 0]
    row[40] = 1000          # replaces the 10 at pixel index 20
    ran = []
    got = pr.noise_row_rule(row, ran)
    d = [row[i] - row[i + 2] for i in range(0, 78, 2)]
    assert sorted(d)[0] == -989 and sorted(d)[-1] == 989 and len(d) == 39
    # stdev = sqrt(2 * 989^2 / 39) ~ 224, so 5 sigma ~ 1120 > 989: pass 1 drops nothing and the row ends
    m = sum(d) / 39
    s = math.sqrt(sum(v * v for v in d) / 39 - m * m)
    assert 5 * s > 989 and ran == [1] and same(got, s)
    # a longer row of the same kind: 400 pairs, stdev ~ 70, 5 sigma ~ 350 < 989: pass 1 drops the two
    # outlier differences, pass 2 sees only +-1 (stdev ~ 1) and drops nothing
    row = []
    for i in range(400):
        row += [10 + (i & 1), 0]
    row[400] = 1000
    ran = []
    got = pr.noise_row_rule(row, ran)
    d = [row[i] - row[i + 2] for i in range(0, 798, 2)]
    kept = [v for v in d if abs(v) <= 1]
    assert len(kept) == len(d) - 2
    m = float(sum(kept)) / len(kept)
    s = math.sqrt(float(sum(v * v for v in kept)) / len(kept) - m * m)
    assert ran == [2] and same(got, s) and same(pr.noise_row_literal(row), s)


def test_flat_rounding_hand_worked():
    # level 1.5 (a float), v / f = 3 / 2 = 1.5: 1.5 * 1.5 = 2.25 -> 2;  v = 1, f = 1, level 2.5 -> exactly 2.5 -> 3
    raw = np.array([[[3, 1, 60000, 0]]], dtype=np.uint16)
    flat = np.array([[[2, 1, 1, 0]]], dtype=np.uint16)
    assert pr.calibrate(raw, flat=flat, level=1.5)[0, 0].tolist() == [2, 2, 65535, 0]
    assert pr.calibrate(raw, flat=flat, level=2.5)[0, 0].tolist() == [4, 3, 65535, 0]   # 3.75 -> 4, 2.5 -> 3 (x.5 up)
    # the level is a float: 0.1f = 0.100000001490116..., so 10 * level exceeds 1 ... and 5 * that = 0.5000000074 -> 1
    raw = np.array([[[5]]], dtype=np.uint16)
    assert pr.calibrate(raw, flat=np.array([[[1]]], dtype=np.uint16), level=0.1)[0, 0, 0] == 1
    assert pr.rtw(5 * 0.1) == 1 and pr.rtw(0.49999999) == 0
    # offset and dark saturate at 0
    raw = np.array([[[10, 10, 10]]], dtype=np.uint16)
    off = np.array([[[3, 10, 11]]], dtype=np.uint16)
    dk = np.array([[[8, 0, 0]]], dtype=np.uint16)
    assert pr.calibrate(raw, offset=off, dark=dk)[0, 0].tolist() == [0, 0, 0]
    assert pr.calibrate(raw, offset=off)[0, 0].tolist() == [7, 0, 0]


def test_search_literal_equals_rule():
    for f in (lambda k: (k - 0.7) ** 2, lambda k: 1.0, lambda k: -k, lambda k: k, lambda k: abs(k - 1.0)):
        a, b = pr.search_literal(f), pr.search_rule(f)
        assert same(a[0], b[0]) and a[1] == b[1] == 13, (a, b)
    frames, dark = pr.fit_case(33, 130, [1.0], seed=3)
    f = lambda k: pr.objective(frames[0, 0], dark, k)
    a, b = pr.search_literal(f), pr.search_rule(f)
    assert same(a[0], b[0]) and a[1] == b[1] == 13
    assert abs(a[0] - 1.0) < 0.05


# ------------------------------------------------------------------ the plan header

def _record(f):
    """objective values in the order the state machine asks for them, its points and its result"""
    g = pr.Golden()
    vals, ks = [], []
    while not g.done:
        w = g.want()
        v = [f(k) for k in w]
        ks += w
        vals += v
        g.feed(v)
    return vals, ks, g.result(), g.iters


def test_plan_search_state_machine(plan_exe):
    frames, dark = pr.fit_case(17, 70, [1.3], seed=4)
    fs = [lambda k: pr.objective(frames[0, 0], dark, k), lambda k: 1.0, lambda k: (k - 0.7) ** 2, lambda k: -k]
    rec = [_record(f) for f in fs]
    out = run_plan(plan_exe, 4, 4, 1, seqs=[r[0] for r in rec])
    at = 0
    for (vals, ks, res, iters), (gres, giters, used), f in zip(rec, out["gres"], fs):
        assert giters == iters == 13 and used == len(vals) == 14
        assert all(same(a, b) for a, b in zip(out["gk"][at:at + used], ks))
        at += used
        assert same(gres, res) and same(gres, pr.search_literal(f)[0])
    # the constant objective ties every time and takes the else branch: a grows, b stays 2
    assert rec[1][2] > 1.99


def _check_stats(out, dark, sig):
    t = pr.thresholds(dark, sig)
    assert all(same(out[k], v) for k, v in zip(("sigma", "median", "tcold", "thot"), t)), (out, t)
    dev = pr.find_deviant(dark, sig)
    W = dark.shape[1]
    want = np.array([(y * W + x) | (0x80000000 if cold else 0) for x, y, cold in dev], dtype=np.uint32)
    assert np.array_equal(out["list"], want)
    assert out["icold"] == sum(1 for d in dev if d[2]) and out["ihot"] == len(dev) - out["icold"]
    return dev


@pytest.mark.parametrize("cfa", [False, True])
@pytest.mark.parametrize("H,W", [(9, 7), (64, 64), (70, 130)])
def test_plan_clusters(plan_exe, H, W, cfa):
    """hot column, row and block, cold next to hot, corners and edges: statistics, list and the
    schedule against the sequential loop"""
    dark = pr.cluster_dark(H, W, seed=H)
    sig = pr.CLUSTER_SIG
    rng = np.random.default_rng(W)
    frames = [rng.integers(0, 65536, size=(H, W)).astype(np.uint16), rng.normal(900, 30, size=(H, W)).astype(np.uint16)]
    out = run_plan(plan_exe, W, H, 1, dark=dark, cosme=True, cfa=cfa, sig=sig, frames=frames)
    assert out["rc"] == 0 and out["applies"] == 1
    dev = _check_stats(out, dark, sig)
    assert out["ihot"] >= H + W - 1 and out["icold"] > 0, (out["ihot"], out["icold"])
    comps = pr.components(dev, W, H, cfa)
    assert out["ncomp"] == len(comps) and out["longest"] == max(len(c) for c in comps) >= max(H, W) // (2 if cfa else 1)
    assert sorted(out["items"].tolist()) == sorted(out["list"].tolist())
    want = np.stack([pr.cosmetic_literal(f, dev, cfa) for f in frames]).reshape(-1)
    assert np.array_equal(out["seq"], want)
    assert np.array_equal(out["sched"], want)


def test_plan_every_pixel_deviant(plan_exe):
    dark = pr.cluster_dark(12, 16, seed=2, every=True)
    sig = (0.5, 0.5)
    frame = np.random.default_rng(8).integers(0, 65536, size=(12, 16)).astype(np.uint16)
    for cfa in (False, True):
        out = run_plan(plan_exe, 16, 12, 1, dark=dark, cosme=True, cfa=cfa, sig=sig, frames=[frame])
        dev = _check_stats(out, dark, sig)
        assert len(dev) == 12 * 16 and out["ncomp"] == (4 if cfa else 1)
        want = pr.cosmetic_literal(frame, dev, cfa).reshape(-1)
        assert np.array_equal(out["seq"], want) and np.array_equal(out["sched"], want)


def test_plan_dark_statistics_edges(plan_exe):
    rng = np.random.default_rng(9)
    # 65535 pixels: counted in ngood, not in the histogram: more than half saturated -> median 0
    d = rng.normal(300, 5, size=(20, 30)).astype(np.uint16)
    d[:12] = 65535
    for sig in ((1.0, 1.0), (-1.0, 2.0), (2.0, -1.0), (-1.0, -1.0), (1000.0, 1000.0)):
        out = run_plan(plan_exe, 30, 20, 1, dark=d, cosme=True, sig=sig)
        _check_stats(out, d, sig)
        assert out["median"] == 0.0
    assert run_plan(plan_exe, 30, 20, 1, dark=d, cosme=True, sig=(-1.0, 2.0))["tcold"] == -1.0
    assert run_plan(plan_exe, 30, 20, 1, dark=d, cosme=True, sig=(2.0, -1.0))["thot"] == 65536.0
    out = run_plan(plan_exe, 30, 20, 1, dark=d, cosme=True, sig=(1000.0, 1000.0))
    assert out["tcold"] == 0.0 and out["thot"] == 65535.0 and out["ihot"] == 12 * 30
    # half saturated exactly: the running count never exceeds ngood / 2 ... 10 of 20 rows
    d2 = d.copy()
    d2[:10] = 65535
    d2[10:] = 300
    out = run_plan(plan_exe, 30, 20, 1, dark=d2, cosme=True, sig=(1.0, 1.0))
    _check_stats(out, d2, (1.0, 1.0))
    assert out["median"] == 0.0
    # all zero except one pixel: sigma 0, median that pixel's value, the pixel is hot and cold ... hot wins
    one = np.zeros((6, 5), dtype=np.uint16)
    one[3, 2] = 1234
    out = run_plan(plan_exe, 5, 6, 1, dark=one, cosme=True, sig=(3.0, 3.0))
    dev = _check_stats(out, one, (3.0, 3.0))
    assert out["sigma"] == 0.0 and out["median"] == 1234.0 and out["ihot"] == 1 and out["icold"] == 29 and len(dev) == 30
    # all zero: no statistics, no list
    out = run_plan(plan_exe, 5, 6, 1, dark=np.zeros((6, 5), dtype=np.uint16), cosme=True, sig=(3.0, 3.0))
    assert out["rc"] == 0 and out["applies"] == 1 and out["list"].size == 0 and out["ncomp"] == 0
    # three layers: skipped
    out = run_plan(plan_exe, 5, 6, 3, dark=np.ones((3, 6, 5), dtype=np.uint16), cosme=True, sig=(3.0, 3.0))
    assert out["rc"] == 0 and out["applies"] == 0 and out["list"].size == 0


def test_plan_level_and_masters(plan_exe):
    rng = np.random.default_rng(10)
    flat = rng.normal(30000, 2000, size=(3, 11, 13)).astype(np.uint16)
    flat[0, 2, :5] = 0
    flat[1, 3, 3] = 0
    off = rng.integers(90, 110, size=(3, 11, 13)).astype(np.uint16)
    out = run_plan(plan_exe, 13, 11, 3, offset=off, flat=flat, autolevel=True, norm=7.0)
    n, mean, _ = pr.mean_sigma_u16(flat[0])
    assert n == 11 * 13 - 5 and same(out["flat_mean"], mean)
    assert same(out["level"], float(np.float32(mean))) and out["level"] != mean     # the float rounding shows
    assert same(out["level"], pr.auto_level(flat))
    assert np.array_equal(out["flat1"], np.where(flat == 0, 1, flat).reshape(-1))
    out = run_plan(plan_exe, 13, 11, 3, flat=flat, norm=0.1)
    assert same(out["level"], float(np.float32(0.1)))
    # sum2 past 2^53 needs 2^21 saturated pixels; the sequential order is pinned at a size that shows it
    big = np.full((1, 1500, 1500), 65535, dtype=np.uint16)
    big[0, ::7] = 60001
    out = run_plan(plan_exe, 1500, 1500, 1, dark=big[0], cosme=True, sig=(1.0, 1.0))
    assert same(out["sigma"], pr.mean_sigma_u16(big)[2])
    # one non-zero pixel: mean = that value; none: refused
    one = np.zeros((1, 4, 4), dtype=np.uint16)
    one[0, 1, 1] = 4242
    assert run_plan(plan_exe, 4, 4, 1, flat=one, autolevel=True)["level"] == 4242.0
    out = run_plan(plan_exe, 4, 4, 1, flat=np.zeros((1, 4, 4), dtype=np.uint16), autolevel=True)
    assert out["rc"] == -1 and "no non-zero pixel" in out["err"]
    # the fit's dark: round_to_WORD(dark - offset)
    dark = rng.integers(0, 300, size=(1, 11, 13)).astype(np.uint16)
    out = run_plan(plan_exe, 13, 11, 1, offset=off[:1], dark=dark, optd=True)
    assert np.array_equal(out["darkfit"], np.maximum(dark.astype(int) - off[:1], 0).reshape(-1))
    assert run_plan(plan_exe, 13, 11, 1, dark=dark, optd=True)["darkfit"].size == 0


def test_plan_refusals(plan_exe):
    m = np.ones((3, 4, 4), dtype=np.uint16)
    out = run_plan(plan_exe, 4, 4, 3, dark=m, optd=True)
    assert out["rc"] == -1 and "nb_layers != 1" in out["err"]
    out = run_plan(plan_exe, 4, 4, 1, optd=True)
    assert out["rc"] == -1 and "needs a master dark" in out["err"]
    out = run_plan(plan_exe, 4, 4, 1, cosme=True)
    assert out["rc"] == -1 and "cosmetic correction needs a master dark" in out["err"]
    for W, H, C in ((0, 4, 1), (4, -1, 1), (4, 4, 0)):
        assert run_plan(plan_exe, W, H, C)["rc"] == -2


def test_plan_noise_rows(plan_exe):
    """the host form of the noise (sgp_noise_row, sgp_noise_finish) on the edge rows and a fit case"""
    rows = [r for _, r, _ in pr.edge_rows()]
    W = max(len(r) for r in rows)
    raw = np.zeros((len(rows), W), dtype=np.uint16)
    for i, r in enumerate(rows):
        raw[i, :len(r)] = r
    dark = np.random.default_rng(12).integers(0, 40, size=raw.shape).astype(np.uint16)
    ks = [0.0, 0.37, 1.0, 2.0]
    out = run_plan(plan_exe, W, len(rows), 1, dark=dark, ks=ks, raw=raw)
    got = out["rows"].reshape(len(ks), len(rows), 2)
    for i, k in enumerate(ks):
        p = pr.dark_subtracted(raw, dark, k)
        assert not pr.has_nan_row(raw, dark, k)
        for y in range(len(rows)):
            want = pr.noise_row_literal(p[y])
            assert (want is not None) == bool(got[i, y, 1]), (k, y)
            if want is not None:
                assert same(got[i, y, 0], want), (k, y)
        assert same(out["noise"][i], pr.objective(raw, dark, k, row=pr.noise_row_literal))
    frames, dark = pr.fit_case(9, 67, [0.6], seed=13)
    out = run_plan(plan_exe, 67, 9, 1, dark=dark, ks=ks, raw=frames[0, 0])
    for i, k in enumerate(ks):
        assert same(out["noise"][i], pr.objective(frames[0, 0], dark, k))
    # too narrow: 0
    out = run_plan(plan_exe, 2, 3, 1, dark=np.ones((3, 2), dtype=np.uint16), ks=[0.5], raw=np.full((3, 2), 9, dtype=np.uint16))
    assert out["noise"] == [0.0]
