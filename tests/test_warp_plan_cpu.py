"""The host-only plan of the sequence warp (siril-0.9_amd/csrc/sg_warp_plan.hpp) and the host + device
header of its kernel (sg_warp_tile.h) without a GPU, in a stand-alone program:
  - every refusal with its code and message, the grid, the chunking at 65535 frame-layers, the
    per-frame table's bytes and the LDS budget at pinned answers;
  - the header's per-pixel rule: a host loop over sgw_coords / sgw_pixel, tile by tile as the kernel
    goes (box staged from the plane, windows outside it read from the plane), gives warp_ref.warp's
    bytes, with every tile on the gather route as well;
  - the footprint property by brute force: every pixel of every tile the footprint routes to LDS has
    its whole window inside the tile's box (stray == 0), and a tile the horizon crosses is never
    routed to LDS."""
import struct
import subprocess

import numpy as np
import pytest

import warp_cases as wc
import warp_ref

SG_ERR_GENERIC, SG_ERR_SIZE = -1, -2
SKIP, APPLY, COPY = 0, 1, 2

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sg_warp_plan.hpp"

struct PlaneSrc {
	const uint16_t *plane;
	int W, H;
	float operator()(int x, int y) const {
		if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H)
			return 0.f;
		return (float)plane[(int64_t)(H - 1 - y) * W + x];
	}
};

struct StageSrc {
	const uint16_t *stage;
	int x0, y0, pitch;
	float operator()(int x, int y) const {
		return (float)stage[(y - y0) * pitch + (x - x0)];
	}
};

struct Tally {
	long long tiles_lds = 0, tiles_gather = 0, stray = 0, crossed = 0, crossed_lds = 0, staged_max = 0;
};

/* one layer as k_warp_seq<K> goes; out == NULL: the routes and the stray count only */
template <int K> static void run(const double *M, int bw, const uint16_t *plane, int W, int H, uint16_t *out, int oW, int oH,
		const float *tab, int force_gather, Tally &t) {
	std::vector<uint16_t> stage(SGW_LDS_SAMPLES);
	for (int ty0 = 0; ty0 < oH; ty0 += SGW_TILE_Y)
		for (int tx0 = 0; tx0 < oW; tx0 += SGW_TILE_X) {
			const int tx1 = std::min(tx0 + SGW_TILE_X, oW) - 1, ty1 = std::min(ty0 + SGW_TILE_Y, oH) - 1;
			const sgw_box b = sgw_footprint(M, K, tx0, ty0, tx1, ty1, W, H, SGW_LDS_SAMPLES, force_gather);
			const bool lds = b.route == SGW_ROUTE_LDS;
			(lds ? t.tiles_lds : t.tiles_gather)++;
			int pos = 0, neg = 0, zero = 0;
			for (int y = ty0; y <= ty1; y++)
				for (int x = tx0; x <= tx1; x++) {
					const double w = M[6] * x + M[7] * y + M[8];
					pos += w > 0;
					neg += w < 0;
					zero += w == 0;
				}
			const bool crossed = zero || (pos && neg);
			t.crossed += crossed;
			t.crossed_lds += crossed && lds;
			if (lds && b.x1 >= b.x0 && b.y1 >= b.y0) {
				t.staged_max = std::max(t.staged_max, (long long)b.pitch * (b.y1 - b.y0 + 1));
				if ((long long)b.pitch * (b.y1 - b.y0 + 1) > SGW_LDS_SAMPLES || b.pitch < b.x1 - b.x0 + 1)
					abort();
				const PlaneSrc ps = {plane, W, H};
				for (int y = b.y0; y <= b.y1; y++)
					for (int x = b.x0; x <= b.x1; x++)
						stage[(size_t)(y - b.y0) * b.pitch + (x - b.x0)] = plane ? (uint16_t)ps(x, y) : 0;
			}
			for (int yd = ty0; yd <= ty1; yd++)
				for (int x = tx0; x <= tx1; x++) {
					const sgw_coord cd = sgw_coords<K>(M, bw, x, yd);
					uint16_t v = 0;
					if (!sgw_all_outside<K>(cd, W, H)) {
						const float *wt = K > 1 && tab ? tab + (size_t)cd.tab * K * K : nullptr;
						const bool in = lds && sgw_in_box<K>(cd, b);
						t.stray += lds && !in;
						if (out && in) {
							const StageSrc ss = {stage.data(), b.x0, b.y0, b.pitch};
							v = sgw_pixel<K>(ss, cd, wt, W, H);
						} else if (out) {
							const PlaneSrc ps = {plane, W, H};
							v = sgw_pixel<K>(ps, cd, wt, W, H);
						}
					}
					if (out)
						out[(int64_t)(oH - 1 - yd) * oW + x] = v;
				}
		}
}

static void run_k(int K, const double *M, int bw, const uint16_t *plane, int W, int H, uint16_t *out, int oW, int oH,
		const float *tab, int force_gather, Tally &t) {
	switch (K) {
	case 1: run<1>(M, bw, plane, W, H, out, oW, oH, tab, force_gather, t); break;
	case 2: run<2>(M, bw, plane, W, H, out, oW, oH, tab, force_gather, t); break;
	case 4: run<4>(M, bw, plane, W, H, out, oW, oH, tab, force_gather, t); break;
	default: run<8>(M, bw, plane, W, H, out, oW, oH, tab, force_gather, t);
	}
}

template <class T> static std::vector<T> slurp(const char *path, size_t n) {
	std::vector<T> v(n);
	FILE *f = fopen(path, "rb");
	if (!f || fread(v.data(), sizeof(T), n, f) != n)
		exit(3);
	fclose(f);
	return v;
}

int main(int argc, char **argv) {
	if (argc >= 2 && !strcmp(argv[1], "consts")) {
		printf("%d %d %d %d %d %d %d %d %d %d\n", SG_ERR_GENERIC, SG_ERR_SIZE, SG_WARP_SKIP, SG_WARP_APPLY, SG_WARP_COPY,
				SGW_TILE_X, SGW_TILE_Y, SGW_LDS_SAMPLES, SGW_ENTRY_BYTES, SGW_CTR_BYTES);
		return 0;
	}
	if (argc >= 2 && !strcmp(argv[1], "plan")) {
		/* plan W H C oW oH interp fpitch opitch nframes in out nodesc nohom knob mode_a mode_s [actions] [slots] homs
		 * in / out: addresses (0 = NULL); knob: SG_WARP_ROUTE; mode_a / mode_s: 0 = NULL, 1 = listed; homs: "ident" or
		 * 9 * nframes values */
		int a = 2;
		sg_warp_seq_desc d;
		d.width = atoi(argv[a++]);
		d.height = atoi(argv[a++]);
		d.nb_layers = atoi(argv[a++]);
		d.out_width = atoi(argv[a++]);
		d.out_height = atoi(argv[a++]);
		d.interpolation = atoi(argv[a++]);
		d.frame_pitch = atoll(argv[a++]);
		d.out_frame_pitch = atoll(argv[a++]);
		const int n = atoi(argv[a++]);
		const uintptr_t in = (uintptr_t)strtoull(argv[a++], NULL, 10), out = (uintptr_t)strtoull(argv[a++], NULL, 10);
		const int nodesc = atoi(argv[a++]), nohom = atoi(argv[a++]), knob = atoi(argv[a++]), ma = atoi(argv[a++]), ms = atoi(argv[a++]);
		const size_t nn = n > 0 ? (size_t)n : 0;
		std::vector<int> act(nn), slot(nn);
		for (size_t i = 0; ma && i < nn; i++)
			act[i] = atoi(argv[a++]);
		for (size_t i = 0; ms && i < nn; i++)
			slot[i] = atoi(argv[a++]);
		std::vector<double> hom(nn * 9 + 9, 0.0);
		if (!strcmp(argv[a], "ident")) {
			for (size_t i = 0; i < nn; i++)
				hom[i * 9] = hom[i * 9 + 4] = hom[i * 9 + 8] = 1.0;
		} else {
			for (size_t i = 0; i < nn * 9; i++)
				hom[i] = atof(argv[a++]);
		}
		SgWarpPlan p;
		std::vector<SgWarpEntry> table;
		const int rc = sg_warp_plan(nodesc ? NULL : &d, n, nohom ? NULL : hom.data(), ma ? act.data() : NULL, ms ? slot.data() : NULL,
				(const void *)in, (const void *)out, knob, p, table);
		printf("%d|%s|%d %d %d %d %d %d %d %lld %d %zu %d %d %zu %zu %zu %d %d %d %lld %lld %zu|", rc, p.err, p.lds_default, p.force_gather, p.interp, p.K, p.bw, p.tiles_x,
				p.tiles_y, (long long)p.tiles, p.lds_samples, p.lds_bytes, p.frames_per_launch, p.nlaunches, p.table_offset,
				p.table_bytes, p.work_bytes, p.napply, p.ncopy, p.max_slot, (long long)p.frame_pitch, (long long)p.out_frame_pitch,
				table.size());
		const unsigned char *tb = (const unsigned char *)table.data();
		for (size_t i = 0; rc == 0 && i < std::min<size_t>(table.size(), 4) * sizeof(SgWarpEntry); i++)
			printf("%02x", tb[i]);
		printf("\n");
		return 0;
	}
	if (argc >= 2 && (!strcmp(argv[1], "foot") || !strcmp(argv[1], "warp"))) {
		/* foot K W H oW oH force h0..h8;  warp K W H oW oH force h0..h8 C in.bin tab.bin out.bin */
		const int K = atoi(argv[2]), W = atoi(argv[3]), H = atoi(argv[4]), oW = atoi(argv[5]), oH = atoi(argv[6]), force = atoi(argv[7]);
		double hom[9], M[9];
		for (int i = 0; i < 9; i++)
			hom[i] = atof(argv[8 + i]);
		sgw_invert3(hom, M);
		const int bw = sgw_block_width(oW, oH);
		Tally t;
		if (!strcmp(argv[1], "foot")) {
			run_k(K, M, bw, NULL, W, H, NULL, oW, oH, NULL, force, t);
		} else {
			const int C = atoi(argv[17]);
			const std::vector<uint16_t> img = slurp<uint16_t>(argv[18], (size_t)C * W * H);
			const std::vector<float> tab = K > 1 ? slurp<float>(argv[19], (size_t)1024 * K * K) : std::vector<float>();
			std::vector<uint16_t> out((size_t)C * oW * oH);
			for (int c = 0; c < C; c++)
				run_k(K, M, bw, img.data() + (size_t)c * W * H, W, H, out.data() + (size_t)c * oW * oH, oW, oH, tab.data(), force, t);
			FILE *f = fopen(argv[20], "wb");
			if (!f || fwrite(out.data(), 2, out.size(), f) != out.size())
				return 3;
			fclose(f);
		}
		printf("%lld %lld %lld %lld %lld %lld %d\n", t.tiles_lds, t.tiles_gather, t.stray, t.crossed, t.crossed_lds, t.staged_max, bw);
		return 0;
	}
	return 2;
}
"""

FIELDS = ["lds_default", "force_gather", "interp", "K", "bw", "tiles_x", "tiles_y", "tiles", "lds_samples", "lds_bytes", "frames_per_launch", "nlaunches",
          "table_offset", "table_bytes", "work_bytes", "napply", "ncopy", "max_slot", "frame_pitch", "out_frame_pitch", "entries"]
KS = {0: 1, 1: 2, 2: 2, 3: 4, 4: 8}
TILE_X, TILE_Y, LDS_SAMPLES = 64, 16, 8176


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("warp_plan")
    src = tmp / "plan.cpp"
    src.write_text(PROGRAM)
    out = tmp / "plan"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", wc.CSRC, str(src), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _call(exe, *args):
    r = subprocess.run([str(exe), *[a if isinstance(a, str) else repr(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return r.stdout.strip()


def plan(exe, W=96, H=80, C=1, oW=96, oH=80, interp=1, fpitch=0, opitch=0, n=1, inp=1 << 20, out=1 << 30, nodesc=0, nohom=0,
         knob=0, action=None, slot=None, hom=None):
    args = ["plan", W, H, C, oW, oH, interp, fpitch, opitch, n, inp, out, nodesc, nohom, knob, int(action is not None), int(slot is not None)]
    args += list(action or []) + list(slot or [])
    args += ["ident"] if hom is None else [float(v) for v in np.asarray(hom, dtype=np.float64).reshape(-1)]
    rc, err, rest, table = _call(exe, *args).split("|")
    return int(rc), err, dict(zip(FIELDS, [int(v) for v in rest.split()])), bytes.fromhex(table)


def test_constants(exe):
    assert [int(v) for v in _call(exe, "consts").split()] == [SG_ERR_GENERIC, SG_ERR_SIZE, SKIP, APPLY, COPY, TILE_X, TILE_Y,
                                                                LDS_SAMPLES, 80, 16384]


def test_grid_and_lds(exe):
    rc, err, p, _ = plan(exe, W=4096, H=4096, oW=4096, oH=4096, n=64, interp=4, out=1 << 40)
    assert rc == 0 and err == ""
    assert (p["K"], p["bw"], p["tiles_x"], p["tiles_y"], p["tiles"]) == (8, 64, 64, 256, 16384)
    # the staged box and the workgroup's own box stay within 16 KiB: ten workgroups' LDS in a CU's 160 KiB
    assert p["lds_samples"] == LDS_SAMPLES and p["lds_bytes"] == 2 * LDS_SAMPLES and p["lds_bytes"] + 24 <= 16384
    assert (p["frames_per_launch"], p["nlaunches"]) == (64, 1)
    assert (p["table_offset"], p["table_bytes"], p["work_bytes"]) == (16384, 64 * 80, 16384 + 64 * 80)      # 256 counter shards of 64 bytes
    assert (p["frame_pitch"], p["out_frame_pitch"], p["napply"], p["ncopy"], p["max_slot"]) == (4096 * 4096, 4096 * 4096, 64, 0, 63)
    for (oW, oH), want in {(150, 40): (64, 3, 3), (150, 9): (113, 3, 1), (64, 16): (64, 1, 1), (65, 17): (64, 2, 2),
                           (1, 1): (1, 1, 1), (70, 50): (64, 2, 4)}.items():
        rc, err, p, _ = plan(exe, oW=oW, oH=oH)
        assert rc == 0 and (p["bw"], p["tiles_x"], p["tiles_y"]) == want, (oW, oH, p)
    for interp, K in KS.items():
        rc, err, p, _ = plan(exe, interp=interp)
        assert (p["K"], p["interp"]) == (K, 1 if interp == 2 else interp)
        # the measured default: linear (and area) and Lanczos-4 take their taps from LDS, nearest and cubic gather
        assert (p["lds_default"], p["force_gather"]) == ((1, 0) if interp in (1, 2, 4) else (0, 1)), interp
        assert plan(exe, interp=interp, knob=1)[2]["force_gather"] == 1 and plan(exe, interp=interp, knob=2)[2]["force_gather"] == 0


def test_chunks_at_65535_frame_layers(exe):
    rc, err, p, _ = plan(exe, W=8, H=8, oW=8, oH=8, n=70000, C=1, out=1 << 40)
    assert rc == 0 and (p["frames_per_launch"], p["nlaunches"], p["entries"]) == (65535, 2, 70000)
    rc, err, p, _ = plan(exe, W=8, H=8, oW=8, oH=8, n=70000, C=3, out=1 << 40)
    assert (p["frames_per_launch"], p["nlaunches"]) == (21845, 4) and 21845 * 3 == 65535
    rc, err, p, _ = plan(exe, W=8, H=8, oW=8, oH=8, n=21846, C=3, out=1 << 40)
    assert (p["frames_per_launch"], p["nlaunches"]) == (21845, 2)
    rc, err, p, _ = plan(exe, W=8, H=8, oW=8, oH=8, n=5, C=2)
    assert (p["frames_per_launch"], p["nlaunches"]) == (5, 1)


def test_table_layout(exe):
    homs = [wc.HOMS["rot5"], wc.HOMS["singular"], wc.HOMS["perspective"]]
    rc, err, p, tb = plan(exe, n=3, action=[APPLY, SKIP, COPY], slot=[4, -1, 0], hom=homs)
    assert rc == 0 and (p["napply"], p["ncopy"], p["max_slot"], p["entries"]) == (1, 1, 4, 3) and len(tb) == 3 * 80
    for f, (a, s) in enumerate([(APPLY, 4), (SKIP, -1), (COPY, 0)]):
        rec = struct.unpack_from("<9dii", tb, f * 80)
        assert list(rec[:9]) == warp_ref.invert3(homs[f]) and rec[9:] == (a, s), (f, rec)
    assert list(struct.unpack_from("<9d", tb, 80)) == [0.0] * 9          # singular: a zero matrix
    # NULL action / slot: all APPLY, frame f to slot f
    rc, err, p, tb = plan(exe, n=3)
    assert [struct.unpack_from("<ii", tb, f * 80 + 72) for f in range(3)] == [(APPLY, 0), (APPLY, 1), (APPLY, 2)]


def test_pitches(exe):
    rc, err, p, _ = plan(exe, C=3, fpitch=3 * 96 * 80 + 11, opitch=3 * 150 * 40 + 5, oW=150, oH=40, n=2)
    assert rc == 0 and (p["frame_pitch"], p["out_frame_pitch"]) == (3 * 96 * 80 + 11, 3 * 150 * 40 + 5)


FRAME = 96 * 80 * 2


@pytest.mark.parametrize("args, code, text", [
    (dict(nodesc=1), SG_ERR_GENERIC, "descriptor"),
    (dict(W=0), SG_ERR_SIZE, "width or height"), (dict(H=-1), SG_ERR_SIZE, "width or height"),
    (dict(oW=0), SG_ERR_SIZE, "width or height"), (dict(oH=0), SG_ERR_SIZE, "width or height"),
    (dict(W=65536, H=32768), SG_ERR_SIZE, "2^31"), (dict(oW=65536, oH=32768), SG_ERR_SIZE, "2^31"),
    (dict(C=0), SG_ERR_SIZE, "nb_layers"), (dict(C=4), SG_ERR_SIZE, "nb_layers"),
    (dict(interp=-1), SG_ERR_GENERIC, "interpolation"), (dict(interp=5), SG_ERR_GENERIC, "interpolation"),
    (dict(n=0), SG_ERR_SIZE, "no frames"),
    (dict(fpitch=96 * 80 - 1), SG_ERR_SIZE, "frame_pitch"), (dict(opitch=96 * 80 - 1), SG_ERR_SIZE, "out_frame_pitch"),
    (dict(nohom=1), SG_ERR_GENERIC, "missing"), (dict(inp=0), SG_ERR_GENERIC, "missing"), (dict(out=0), SG_ERR_GENERIC, "missing"),
    (dict(n=2, action=[APPLY, 3]), SG_ERR_GENERIC, "action"), (dict(n=2, action=[-1, APPLY]), SG_ERR_GENERIC, "action"),
    (dict(n=2, action=[APPLY, COPY], oW=97), SG_ERR_GENERIC, "COPY"), (dict(n=2, action=[COPY, SKIP], oH=79), SG_ERR_GENERIC, "COPY"),
    (dict(n=3, slot=[0, -1, 1]), SG_ERR_GENERIC, "below 0"),
    (dict(n=3, slot=[0, 1, 0]), SG_ERR_GENERIC, "same slot"), (dict(n=3, action=[APPLY, SKIP, COPY], slot=[2, 0, 2]), SG_ERR_GENERIC, "same slot"),
    # byte ranges: the source spans 3 frames from 1 << 20; the output spans slots 0 .. 2
    (dict(n=3, out=(1 << 20) + 3 * FRAME - 2), SG_ERR_GENERIC, "overlap"),
    (dict(n=3, out=(1 << 20) - 3 * FRAME + 2), SG_ERR_GENERIC, "overlap"),
    (dict(n=3, out=1 << 20), SG_ERR_GENERIC, "overlap"),
    (dict(n=3, out=(1 << 20) - 5 * FRAME + 2, slot=[0, 4, 1]), SG_ERR_GENERIC, "overlap"),
])
def test_refusals(exe, args, code, text):
    rc, err, p, tb = plan(exe, **args)
    assert rc == code and err.startswith("warp:") and text in err, (rc, err)
    assert p["work_bytes"] == 0 and p["nlaunches"] == 0


def test_what_is_not_refused(exe):
    # a skipped frame's slot and a skipped frame's action-dependent checks do not count
    assert plan(exe, n=3, action=[APPLY, SKIP, SKIP], slot=[0, -5, 0])[0] == 0
    assert plan(exe, n=2, action=[SKIP, SKIP], slot=[-1, -1], out=1 << 20)[0] == 0      # nothing written: no overlap
    # the ranges touch
    assert plan(exe, n=3, out=(1 << 20) + 3 * FRAME)[0] == 0 and plan(exe, n=3, out=(1 << 20) - 3 * FRAME)[0] == 0
    assert plan(exe, n=3, out=(1 << 20) - 5 * FRAME, slot=[0, 4, 1])[0] == 0
    assert plan(exe, n=2, action=[APPLY, COPY])[0] == 0


def foot(exe, K, hom, oW, oH, force=0, W=wc.W, H=wc.H):
    v = [int(t) for t in _call(exe, "foot", K, W, H, oW, oH, force, *[float(h) for h in np.asarray(hom).reshape(9)]).split()]
    return dict(zip(["lds", "gather", "stray", "crossed", "crossed_lds", "staged_max", "bw"], v))


def _tiles(oW, oH):
    return ((oW + TILE_X - 1) // TILE_X) * ((oH + TILE_Y - 1) // TILE_Y)


@pytest.mark.parametrize("name", sorted(wc.HOMS))
def test_footprint_holds_every_tap(exe, name):
    for oW, oH in wc.OUT_SIZES + [(96, 80), (70, 50)]:      # and the sizes test_gpu_warp_frames.py adds
        for K in (1, 2, 4, 8):
            t = foot(exe, K, wc.HOMS[name], oW, oH)
            assert t["lds"] + t["gather"] == _tiles(oW, oH)
            assert t["stray"] == 0 and t["crossed_lds"] == 0, (name, oW, oH, K, t)
            assert t["staged_max"] <= LDS_SAMPLES
            if name in wc.REGULAR:
                assert t["gather"] == 0, (name, oW, oH, K, t)      # the property is about something
            if name == "singular":
                assert t["lds"] == 0 and t["crossed"] == _tiles(oW, oH)


def test_horizon_tiles_gather(exe):
    for K in (1, 2, 4, 8):
        t = foot(exe, K, wc.HOMS["horizon"], 150, 40)
        # the denominator changes sign at x = 75: the middle column of tiles, all three rows of it
        assert t["crossed"] == 3 and t["crossed_lds"] == 0 and t["gather"] >= 3 and t["stray"] == 0, t
        t = foot(exe, K, wc.HOMS["horizon"], 64, 16)
        assert t["crossed"] == 0 and t["stray"] == 0


def test_route_knob_and_budget(exe):
    t = foot(exe, 4, wc.HOMS["rot5"], 150, 40, force=1)
    assert (t["lds"], t["gather"], t["stray"]) == (0, 9, 0)
    # a tenfold reduction: a 64 x 16 tile covers 640 x 160 source pixels, far above the budget
    shrink = np.diag([0.1, 0.1, 1.0])
    t = foot(exe, 2, shrink, 128, 32, W=2000, H=500)
    assert (t["lds"], t["gather"]) == (0, 4)
    # but the same tile past the image stages nothing and stays on the LDS route
    t = foot(exe, 2, wc.translation(5000.0, 0.0), 128, 32)
    assert (t["lds"], t["gather"], t["stray"], t["staged_max"]) == (4, 0, 0, 0)


@pytest.fixture(scope="module")
def source():
    return wc.frames(1, 2)[0]


@pytest.mark.parametrize("interp", [0, 1, 3, 4])
@pytest.mark.parametrize("name", ["identity", "shift_frac", "rot5", "rot45", "scale0_8", "perspective", "horizon", "singular"])
def test_header_rule_equals_warp_ref(exe, tmp_path, source, name, interp):
    K = KS[interp]
    C, H, W = source.shape
    (tmp_path / "in.bin").write_bytes(source.tobytes())
    if K > 1:
        (tmp_path / "tab.bin").write_bytes(warp_ref.table(interp)[0].tobytes())
    for oW, oH in [(150, 40), (150, 9), (65, 17)]:
        want = warp_ref.warp(source, wc.HOMS[name], (oW, oH), interp)
        for force in (0, 1):
            _call(exe, "warp", K, W, H, oW, oH, force, *[float(h) for h in wc.HOMS[name].reshape(9)], C,
                  str(tmp_path / "in.bin"), str(tmp_path / "tab.bin"), str(tmp_path / "out.bin"))
            got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint16).reshape(C, oH, oW)
            assert np.array_equal(got, want), (name, interp, oW, oH, force, np.argwhere(got != want)[:5])
