"""The host-only plan of a one-star registration call (siril-0.9_amd/csrc/sg_seqpsf_plan.hpp) without a GPU:
built into a stand-alone program and pinned: every refusal and its code, the per-frame table with the
clamped areas of the parallel framings, the chain's start, the LDS bytes and the grid."""
import os
import subprocess

import pytest

import seqpsf_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "sg_seqpsf_plan.hpp"

/* argv: framing x y w h norm scale_x scale_y W H nframes frame_pitch row_pitch use_shifts use_included use_carry */
int main(int argc, char **argv) {
	if (argc < 17)
		return 2;
	sg_seqpsf_desc d;
	d.framing = atoi(argv[1]);
	d.area.x = atoi(argv[2]);
	d.area.y = atoi(argv[3]);
	d.area.w = atoi(argv[4]);
	d.area.h = atoi(argv[5]);
	d.norm = atof(argv[6]);
	d.fwhm_scale_x = atof(argv[7]);
	d.fwhm_scale_y = atof(argv[8]);
	d.fit_angle = 1;
	const int W = atoi(argv[9]), H = atoi(argv[10]), n = atoi(argv[11]);
	const long long fp = atoll(argv[12]), rp = atoll(argv[13]);
	const int m = n > 0 ? n : 1;
	std::vector<int> sx((size_t)m), sy((size_t)m), inc((size_t)m);
	for (int f = 0; f < m; f++) {
		sx[f] = 7 * f - 10;	/* -10, -3, 4, 11, .. */
		sy[f] = 12 - 9 * f;	/* 12, 3, -6, -15, .. */
		inc[f] = f != 1;
	}
	sg_rect carry = {-9, 70, 1, 1};
	SgSeqpsfPlan p;
	const int rc = sg_seqpsf_plan(&d, W, H, n, fp, rp, atoi(argv[15]) ? inc.data() : nullptr, atoi(argv[14]) ? sx.data() : nullptr,
			atoi(argv[14]) ? sy.data() : nullptr, atoi(argv[16]) ? &carry : nullptr, p);
	printf("rc %d\nerr %s\n", rc, p.err);
	if (rc == SG_OK) {
		printf("plan %d %d %lld %lld %u %u %zu %zu %d %d\n", p.w, p.h, (long long)p.frame_pitch, (long long)p.row_pitch, p.grid,
				p.threads, p.lds_box, p.lds_bytes, p.start_x, p.start_y);
		for (int f = 0; f < n; f++)
			printf("item %d %d %d\n", p.items[f].run, p.items[f].x, p.items[f].y);
	}
	return 0;
}
'''

SG_OK, SG_ERR_GENERIC, SG_ERR_SIZE = 0, -1, -2
THREADS = {0: 256, 1: 256, 2: 256}     # SGQ_THREADS: one size for both kernels (a static chain equals ORIGINAL bit for bit)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("seqpsf_plan")
    src = d / "plan.cpp"
    src.write_text(PROGRAM)
    out = d / "plan"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", INC, str(src), "-o", str(out),
                        "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def plan(exe, framing=0, area=(10, 10, 15, 11), norm=65535.0, scales=(1.0, 1.0), W=64, H=48, n=4, fp=0, rp=0, shifts=0,
         included=0, carry=0):
    args = [framing, *area, norm, scales[0], scales[1], W, H, n, fp, rp, shifts, included, carry]
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    out = dict(rc=int(lines[0].split()[1]), err=lines[1][4:], items=[])
    for ln in lines[2:]:
        t = ln.split()
        if t[0] == "plan":
            out.update(zip(("w", "h", "frame_pitch", "row_pitch", "grid", "threads", "lds_box", "lds_bytes", "start_x", "start_y"),
                           [int(v) for v in t[1:]]))
        else:
            out["items"].append(tuple(int(v) for v in t[1:]))
    return out


def lds(w, h, framing):
    box, waves = (2 * w * h + 15) // 16 * 16, THREADS[framing] // 64
    return box, box + waves * 36 * 8 + 256 * 4 + 16 * 8 + waves * 8


@pytest.mark.parametrize("kw, code, word", [
    (dict(area=(0, 0, 0, 5)), SG_ERR_SIZE, "below 1"),
    (dict(area=(0, 0, 5, -1)), SG_ERR_SIZE, "below 1"),
    (dict(area=(0, 0, 129, 8), W=200, H=200), SG_ERR_SIZE, "above 128"),
    (dict(area=(0, 0, 8, 129), W=200, H=200), SG_ERR_SIZE, "above 128"),
    (dict(area=(0, 0, 65, 8)), SG_ERR_SIZE, "larger than the image"),
    (dict(area=(0, 0, 8, 49)), SG_ERR_SIZE, "larger than the image"),
    (dict(W=7), SG_ERR_SIZE, "below 8"),
    (dict(H=65537), SG_ERR_SIZE, "above 65536"),
    (dict(W=65536, H=32768), SG_ERR_SIZE, "2^31"),
    (dict(rp=63), SG_ERR_SIZE, "row_pitch"),
    (dict(rp=70, fp=47 * 70 + 63), SG_ERR_SIZE, "frame_pitch"),
    (dict(n=0), SG_ERR_SIZE, "no frames"),
    (dict(framing=3), SG_ERR_GENERIC, "framing"),
    (dict(framing=-1), SG_ERR_GENERIC, "framing"),
    (dict(framing=1), SG_ERR_GENERIC, "shifts"),
    (dict(norm=255.0), SG_ERR_GENERIC, "norm"),
    (dict(scales=("nan", 1.0)), SG_ERR_GENERIC, "scale"),
    (dict(scales=(1.0, "inf")), SG_ERR_GENERIC, "scale"),
])
def test_refusals(exe, kw, code, word):
    p = plan(exe, **kw)
    assert p["rc"] == code and word in p["err"], p


def test_accepted_edges(exe):
    assert plan(exe, area=(0, 0, 128, 128), W=128, H=128)["rc"] == SG_OK
    assert plan(exe, area=(0, 0, 64, 48))["rc"] == SG_OK                 # the area is the image
    assert plan(exe, area=(0, 0, 3, 2))["rc"] == SG_OK                   # w h <= 6 is no error
    p = plan(exe, rp=70, fp=47 * 70 + 64)
    assert p["rc"] == SG_OK and (p["frame_pitch"], p["row_pitch"]) == (47 * 70 + 64, 70)
    p = plan(exe)
    assert (p["frame_pitch"], p["row_pitch"]) == (48 * 64, 64)


@pytest.mark.parametrize("framing", [0, 1, 2])
@pytest.mark.parametrize("w, h", [(1, 7), (128, 128), (127, 3)])
def test_lds_bytes(exe, w, h, framing):
    p = plan(exe, framing=framing, area=(0, 0, w, h), W=160, H=144, shifts=1)
    assert p["rc"] == SG_OK and (p["lds_box"], p["lds_bytes"]) == lds(w, h, framing) and p["threads"] == THREADS[framing]
    assert p["lds_bytes"] <= 64 * 1024 and p["lds_box"] % 16 == 0
    assert (w, h) != (128, 128) or p["lds_box"] == 32768


def test_original_table(exe):
    p = plan(exe, area=(-5, 45, 15, 11), n=4, included=1)
    assert p["grid"] == 4 and p["items"] == [(1, 0, 37), (0, 0, 37), (1, 0, 37), (1, 0, 37)]
    assert plan(exe, area=(60, -3, 15, 11), n=2)["items"] == [(1, 49, 0)] * 2
    # shifts given but the framing is ORIGINAL: not applied
    assert plan(exe, n=3, shifts=1)["items"] == [(1, 10, 10)] * 3


def test_registered_table(exe):
    # x -= shiftx, y += shifty with shiftx = -10, -3, 4, 11, 18 and shifty = 12, 3, -6, -15, -24, then the clamp
    p = plan(exe, framing=1, area=(10, 10, 15, 11), n=5, shifts=1, included=1)
    want = [sr.enforce_area(64, 48, (10 - (7 * f - 10), 10 + (12 - 9 * f), 15, 11))[:2] for f in range(5)]
    assert want == [(20, 22), (13, 13), (6, 4), (0, 0), (0, 0)]
    assert p["items"] == [(int(f != 1),) + want[f] for f in range(5)] and p["grid"] == 5


def test_chain_plan(exe):
    p = plan(exe, framing=2, area=(-5, 45, 15, 11), n=6)
    assert p["grid"] == 1 and (p["start_x"], p["start_y"]) == (-5, 45)      # the carry is unclamped
    assert all(it[0] == 1 for it in p["items"])
    p = plan(exe, framing=2, area=(-5, 45, 15, 11), n=3, carry=1, included=1)
    assert (p["start_x"], p["start_y"]) == (-9, 70) and [it[0] for it in p["items"]] == [1, 0, 1]
    # the carry is the chain's business only
    assert plan(exe, framing=0, carry=1)["items"][0] == (1, 10, 10)
