"""The host-only plan of the automatic cosmetic correction (siril-0.9_amd/csrc/sg_cosme_plan.hpp)
without a GPU, at pinned answers: the tile grid and halos, the scratch of a chunk, the frames per
chunk from the byte budget and from the SG_COSME_CHUNK / SG_COSME_LIST knobs, the 32-bit pixel id,
every refusal with its code, and the layer thresholds of sgc_rule_make against the double
comparisons they replace."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sg_cosme_plan.hpp"

int main(int argc, char **argv) {
	if (argc >= 2 && !strcmp(argv[1], "rule")) {	/* rule ngood median sumabs sig0 sig1 amount cfa */
		sgc_rule r;
		sgc_rule_make(&r, atoll(argv[2]), (uint32_t)atoll(argv[3]), (uint64_t)atoll(argv[4]), atof(argv[5]), atof(argv[6]),
				atof(argv[7]), atoi(argv[8]));
		int bad = 0;	/* the thresholds against the reference's double comparisons, every WORD */
		for (int v = 0; v < 65536; v++) {
			const double k1 = r.avg_dev, k2 = k1 / 2, k = r.avg_dev * atof(argv[5]);
			const bool hot = atof(argv[6]) != -1.0 && (v > r.bkg + k1), amax = atof(argv[6]) != -1.0 && (v < r.bkg + k2);
			const bool cold = atof(argv[5]) != -1.0 && ((v + k) < r.bkg);
			bad += hot != (v >= r.hot_min) || amax != (v <= r.a_max) || cold != (v <= r.cold_max);
			bad += sgc_own(r, (uint32_t)v) != (hot ? SGC_HOT : (cold ? SGC_COLD : SGC_NONE));
		}
		printf("%d %d %d %d %.17g %.17g %d %zu\n", r.hot_min, r.a_max, r.cold_max, r.step, r.bkg, r.avg_dev, bad,
				sizeof(sgc_rule));
		return 0;
	}
	/* plan W H C cfa sig0 sig1 amount nframes stride budget chunk list */
	sg_cosme_desc d;
	memset(&d, 0, sizeof d);
	d.width = atoi(argv[2]);
	d.height = atoi(argv[3]);
	d.nb_layers = atoi(argv[4]);
	d.is_cfa = atoi(argv[5]);
	d.sig[0] = atof(argv[6]);
	d.sig[1] = atof(argv[7]);
	d.amount = atof(argv[8]);
	SgCosmePlan p;
	const int rc = sg_cosme_plan(&d, atoi(argv[9]), atoll(argv[10]), atoll(argv[11]), atoi(argv[12]), atoi(argv[13]), p);
	printf("%d|%s|%d %d %d %d %d %d %zu %d %d %d %llu %llu %zu %zu %zu %zu %zu %zu %zu %u %lld\n", rc, p.err, p.step, p.halo,
			p.tiles_x, p.tiles_y, p.in_w, p.in_h, p.lds_tile, p.hist_blocks, p.chunk, p.nchunks,
			(unsigned long long)p.chunk_pixels, (unsigned long long)p.plane_words, p.state_bytes, p.plane_bytes,
			p.list_bytes, p.hist_bytes, p.rule_bytes, p.count_bytes, p.total_bytes, p.list_cap, (long long)p.frame_stride);
	return 0;
}
"""

FIELDS = ["step", "halo", "tiles_x", "tiles_y", "in_w", "in_h", "lds_tile", "hist_blocks", "chunk", "nchunks", "chunk_pixels",
          "plane_words", "state_bytes", "plane_bytes", "list_bytes", "hist_bytes", "rule_bytes", "count_bytes", "total_bytes",
          "list_cap", "frame_stride"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cosme_plan")
    src = tmp / "plan.cpp"
    src.write_text(PROGRAM)
    out = tmp / "plan"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", INC, str(src), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def plan(exe, W=64, H=32, C=1, cfa=0, sig=(3.0, 3.0), amount=1.0, nframes=1, stride=0, budget=0, chunk=0, lst=0):
    r = subprocess.run([str(exe), "plan", *[repr(v) for v in (W, H, C, cfa, sig[0], sig[1], amount, nframes, stride, budget,
                                                                  chunk, lst)]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rc, err, rest = r.stdout.strip().split("|")
    return int(rc), err, dict(zip(FIELDS, [int(v) for v in rest.split()]))


def up16(v):
    return (v + 15) & ~15


def scratch(chunk, C, npix, list_cap=None):
    """the documented layout, computed independently of the header"""
    px = chunk * C * npix
    words = (px + 31) // 32
    cap = max(px // 8, 65536) if list_cap is None else list_cap
    d = dict(chunk_pixels=px, plane_words=words, state_bytes=up16(2 * px), plane_bytes=up16(4 * words), list_cap=cap,
             list_bytes=up16(4 * cap), hist_bytes=chunk * C * 65536 * 4, rule_bytes=up16(chunk * C * 72),
             count_bytes=up16(chunk * 16) + 32)
    d["total_bytes"] = (d["state_bytes"] + 4 * d["plane_bytes"] + 2 * d["list_bytes"] + d["hist_bytes"] + d["rule_bytes"]
                        + d["count_bytes"])
    return d


def test_full_size_sequence(exe):
    rc, err, p = plan(exe, W=4096, H=4096, nframes=64)
    assert rc == 0 and err == ""
    assert (p["step"], p["halo"], p["tiles_x"], p["tiles_y"], p["in_w"], p["in_h"], p["lds_tile"]) == (1, 2, 64, 128, 68, 36, 4896)
    assert p["hist_blocks"] == 257 and p["frame_stride"] == 4096 * 4096
    # one frame: 32 MiB state + 4 x 2 MiB planes + 2 x 8 MiB lists + 256 KiB histogram + 80 + 48 bytes
    assert scratch(1, 1, 4096 * 4096)["total_bytes"] == 58982528
    assert (p["chunk"], p["nchunks"]) == ((1 << 30) // 58982528, 4) == (18, 4)
    assert {k: p[k] for k in scratch(18, 1, 4096 * 4096)} == scratch(18, 1, 4096 * 4096)


def test_cfa_and_edges_of_the_grid(exe):
    rc, _, p = plan(exe, W=65, H=33, C=3, cfa=1, nframes=5)
    assert rc == 0
    assert (p["step"], p["halo"], p["tiles_x"], p["tiles_y"], p["in_w"], p["in_h"], p["lds_tile"]) == (2, 4, 2, 2, 72, 40, 5760)
    assert (p["chunk"], p["nchunks"], p["hist_blocks"], p["frame_stride"]) == (5, 1, 1, 3 * 65 * 33)
    assert {k: p[k] for k in scratch(5, 3, 65 * 33)} == scratch(5, 3, 65 * 33)
    assert p["list_cap"] == 65536
    for W, H, tx, ty in [(63, 31, 1, 1), (64, 32, 1, 1), (65, 32, 2, 1), (64, 33, 1, 2), (129, 65, 3, 3), (1, 7, 1, 1)]:
        rc, _, p = plan(exe, W=W, H=H)
        assert rc == 0 and (p["tiles_x"], p["tiles_y"]) == (tx, ty), (W, H)


def test_chunking(exe):
    rc, _, p = plan(exe, W=30, H=20, nframes=3, chunk=2)
    assert rc == 0 and (p["chunk"], p["nchunks"]) == (2, 2)
    rc, _, p = plan(exe, W=30, H=20, nframes=3, chunk=7)
    assert (p["chunk"], p["nchunks"]) == (3, 1)
    rc, _, p = plan(exe, W=30, H=20, nframes=9, budget=1)      # below one frame's scratch: one frame per chunk
    assert (p["chunk"], p["nchunks"]) == (1, 9)
    rc, _, p = plan(exe, W=30, H=20, nframes=9, budget=3 * scratch(1, 1, 600)["total_bytes"] + 5)
    assert (p["chunk"], p["nchunks"]) == (3, 3)
    rc, _, p = plan(exe, W=30, H=20, C=3, nframes=40000, chunk=40000)   # frame * C + layer is the grid's z
    assert (p["chunk"], p["nchunks"]) == (21845, 2)
    rc, _, p = plan(exe, W=30, H=20, nframes=3, lst=8)
    assert p["list_cap"] == 8 and p["list_bytes"] == 32
    rc, _, p = plan(exe, W=30, H=20, nframes=3, stride=700)
    assert rc == 0 and p["frame_stride"] == 700


def test_pixel_id_fits_32_bits(exe):
    # 16384^2 = 2^28 pixels a frame: at most 15 frames hold their ids below 2^32 - 64
    rc, _, p = plan(exe, W=16384, H=16384, nframes=64, chunk=64)
    assert rc == 0 and p["chunk"] <= 15 and p["chunk"] * (1 << 28) <= 0xFFFFFFFF - 64 and p["chunk"] >= 8
    rc, err, _ = plan(exe, W=46340, H=46340, C=3, nframes=1)
    assert rc == -2 and "32-bit" in err


REFUSED = [
    (dict(W=0), -2, "not positive"), (dict(H=-3), -2, "not positive"), (dict(W=65536, H=32768), -2, "2^31"),
    (dict(C=0), -2, "nb_layers"), (dict(C=4), -2, "nb_layers"), (dict(nframes=0), -2, "no frames"),
    (dict(stride=64 * 32 - 1), -2, "frame_stride"), (dict(C=2, stride=64 * 32), -2, "frame_stride"),
    (dict(W=1, H=1), -2, "neighbour"), (dict(W=2, H=2, cfa=1), -2, "neighbour"), (dict(W=2, H=1, cfa=1), -2, "neighbour"),
    (dict(sig=(-0.5, 3.0)), -1, "sigma"), (dict(sig=(3.0, -2.0)), -1, "sigma"), (dict(sig=(float("nan"), 3.0)), -1, "sigma"),
    (dict(sig=(3.0, float("-inf"))), -1, "sigma"), (dict(amount=1.0000001), -1, "amount"), (dict(amount=-1e-9), -1, "amount"),
    (dict(amount=float("nan")), -1, "amount"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_refusals(exe, i):
    change, code, word = REFUSED[i]
    rc, err, p = plan(exe, **change)
    assert rc == code and err.startswith("cosme:") and word in err, (rc, err)
    assert p["chunk"] == 0


def test_accepted_at_the_limits(exe):
    for change in (dict(W=2, H=1), dict(W=1, H=2), dict(W=3, H=1, cfa=1), dict(W=2, H=3, cfa=1), dict(sig=(-1.0, -1.0)),
                   dict(sig=(0.0, 0.0)), dict(amount=0.0), dict(sig=(float("inf"), 3.0)), dict(W=32768, H=65535)):
        rc, err, _ = plan(exe, **change)
        assert rc == 0, (change, err)


@pytest.mark.parametrize("args,want", [
    # ngood median sumabs sig0 sig1 amount cfa -> hot_min a_max cold_max step
    ((1000, 1000, 24500, 3.0, 3.0, 1.0, 0), (1025, 1012, 926, 1)),       # avgDev 24.5: 1024.5, 1012.25, 926.5
    ((1000, 1000, 24000, 3.0, 3.0, 1.0, 1), (1025, 1011, 927, 2)),       # avgDev 24: > 1024, < 1012, + 72 < 1000
    ((1000, 1000, 24000, -1.0, 3.0, 1.0, 0), (1025, 1011, -1, 1)),
    ((1000, 1000, 24000, 3.0, -1.0, 1.0, 0), (65536, -1, 927, 1)),
    ((20, 0, 20 * 65535, 3.0, 3.0, 1.0, 0), (65536, 32767, -1, 1)),      # a layer of 65535s: bkg 0
    ((5, 7, 0, 3.0, 3.0, 1.0, 0), (8, 6, 6, 1)),                         # avgDev 0
    ((0, 0, 0, 3.0, 3.0, 1.0, 0), (65536, -1, -1, 1)),                   # no data
    ((1000, 60000, 8000000, 0.0, 0.0, 0.5, 0), (65536, 63999, 59999, 1)),    # bkg + avgDev above every WORD
])
def test_rule_thresholds(exe, args, want):
    r = subprocess.run([str(exe), "rule", *[repr(v) for v in args]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    f = r.stdout.split()
    assert tuple(int(v) for v in f[:4]) == want, r.stdout
    assert int(f[7]) == 72
    if args[0] > 0:     # a layer without data is never scanned
        assert int(f[6]) == 0, "a threshold disagrees with the double comparison for some WORD"
        assert float(f[4]) == float(args[1]) and float(f[5]) == args[2] / args[0]
