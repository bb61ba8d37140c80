"""CFA SER demosaicing with nearest neighbour and VNG (sg_seq_set_debayer_method,
include/sirilgpu_io.h; csrc/sg_debayer.h, csrc/sg_io.hip): the per-pixel rules against the
reference's loops restated literally (tests/debayer_vng_ref.py), and the library's three read
paths (whole frame, region, device load) against them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "siril-0.9_amd", "python"))
import sirilgpu as sg  # noqa: E402
import oracle_lib as orc  # noqa: E402
import debayer_ref as dr  # noqa: E402
import debayer_vng_ref as vr  # noqa: E402
from seq_files import write_ser  # noqa: E402

NN, VNG = vr.INTER_NEAREST, vr.INTER_VNG
# SER ColorID -> sensor_pattern (ser.h:19-22)
TILE_OF_ID = {8: dr.BAYER_RGGB, 9: dr.BAYER_GRBG, 10: dr.BAYER_GBRG, 11: dr.BAYER_BGGR}
# k_debayer_vng's tile: SG_VNG_TW x SG_VNG_TH (csrc/sg_io.hip)
T_W, T_H = 64, 16


def _cfa(seed, shape, hi=65536):
    return np.random.default_rng(seed).integers(0, hi, size=shape).astype(np.uint16)


# ---- the per-pixel rules == the reference's loops ----

@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 2), (3, 4), (6, 7), (9, 12)])
def test_nearest_rule_matches_literal_loop(tile, shape):
    b = _cfa(tile * 31 + shape[1], shape)
    got = vr.nearest_per_pixel(b, tile)
    assert np.array_equal(got, vr.bayer_nearest_literal(b, tile))
    # the last row and column are 0, the first are not
    assert not got[-1].any() and not got[:, -1].any()
    if shape[0] > 2:
        assert got[0].any() and got[:, 0].any()


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(6, 6), (7, 9), (10, 13)])
def test_vng_rule_matches_literal_loop(tile, shape):
    b = _cfa(tile * 37 + shape[1], shape)
    got = vr.vng_per_pixel(b, tile)
    assert np.array_equal(got, vr.bayer_vng_literal(b, tile))
    # the two-pixel ring keeps the bilinear result, its zero border included
    bil = dr.bayer_bilinear(b, tile)
    ring = np.ones(shape, dtype=bool)
    ring[2:-2, 2:-2] = False
    assert np.array_equal(got[ring], bil[ring])
    for y in range(-2, 3):                              # the colour of a site, both ways
        for x in range(-2, 3):
            assert vr.fc(vr.VNG_FILTERS[tile], y, x) == vr.cfa_color(tile, y, x)


def _open(tmp_path, frames_td, color_id, depth=16, endian_flag=0, name="cfa.ser"):
    """frames_td: [N][H][W] top-down CFA frames -> an opened Seq"""
    mem = np.asarray(frames_td)[:, None, ::-1, :]       # memory order, bottom-up
    path = str(tmp_path / name)
    write_ser(path, mem, depth=depth, color_id=color_id, endian_flag=endian_flag)
    return sg.Seq.open_ser(path)


@pytest.mark.parametrize("tile_id", [8, 9, 10, 11])
def test_vng_flat_frame_is_bilinear(tmp_path, tile_id):
    """every gradient of a flat frame is 0 (gmax == 0): VNG copies the bilinear pixel"""
    b = np.full((8, 9), 1234, dtype=np.uint16)
    tile = TILE_OF_ID[tile_id]
    bil = dr.debayer_frame_memory_order(b, tile)
    assert np.array_equal(vr.frame_memory_order(b, tile, VNG, literal=True), bil)
    with _open(tmp_path, b[None], tile_id) as seq:
        seq.set_debayer(-1, sg.BAYER_INTER_VNG)
        assert np.array_equal(seq.read_frame(0), bil)


def test_vng_hand_worked_6x6(tmp_path):
    """The four VNG pixels of one 6x6 RGGB frame, worked by hand.

    Bilinear image (rows 1..4, columns 1..4; the border ring is 0):
      R: 660 539 642 746 | 722 824 835 846 | 615 827 765 704 | 507 830 696 561
      G: 645 824 717 916 | 102 590 437 529 | 433 996 617 303 | 138 694 731 563
      B: 624 548 472 661 | 766 699 632 660 | 908 850 791 660 | 621 544 467 429
    Directions g = 0..7: (-1,-1) (-1,0) (-1,1) (0,1) (1,1) (1,0) (1,-1) (0,-1).

    (2,2), a red site, own R = 824.  Gradients, each the sum of its terms |a - b| << shift:
      g0 = 1648 + 824 + 102 + 334 + 387 + 894 = 4189    g1 = 102 + 1648 + 437 + 284 + 344 + 319 = 3134
      g2 = 824 + 1648 + 722 + 872 + 479 + 559 = 5104    g3 = 152 + 92 + 670 + 44 + 117 + 693 = 1768
      g4 = 334 + 387 + 894 + 526 + 134 + 265 = 2540     g5 = 284 + 344 + 319 + 36 + 12 + 294 = 1289
      g6 = 722 + 872 + 102 + 1648 + 559 + 858 = 4761    g7 = 824 + 152 + 1648 + 670 + 996 + 117 = 4407
      thold = 1289 + (5104 >> 1) = 3841 takes g1, g3, g4, g5.  All neighbours of a red site are of
      another colour, so R takes (824 + R two steps away) >> 1: (824+0)>>1 = 412, (824+846)>>1 = 835,
      (824+561)>>1 = 692, (824+830)>>1 = 827: sum R = 2766; G = 824 + 437 + 617 + 996 = 2874;
      B = 548 + 632 + 791 + 850 = 2821.  G = 824 + (2874 - 2766) / 4 = 851, B = 824 + 55 / 4 = 837.
    (2,3), a green site, own G = 437: gval = 3942 3967 4264 2966 3386 2302 1662 1768,
      thold = 1662 + 2132 = 3794 takes g3..g7; the cross directions halve G with the green two steps
      away, the diagonal ones (green neighbours) take the neighbour's G:
      G = (437+0)>>1 + 303 + (437+731)>>1 + 996 + (437+102)>>1 = 218 + 303 + 584 + 996 + 269 = 2370,
      R = 846 + 704 + 765 + 827 + 824 = 3966, B = 660 + 660 + 791 + 850 + 699 = 3660:
      R = 437 + 1596 / 5 = 756, B = 437 + 1290 / 5 = 695.
    (3,2), a green site, own G = 996: gval = 5244 1289 1662 2839 5592 4033 5820 4808,
      thold = 1289 + 2910 = 4199 takes g1, g2, g3, g5: G = (996+824)>>1 + 437 + (996+303)>>1 +
      (996+0)>>1 = 910 + 437 + 649 + 498 = 2494, R = 824 + 835 + 765 + 830 = 3254,
      B = 699 + 632 + 791 + 544 = 2666: R = 996 + 760 / 4 = 1186, B = 996 + 172 / 4 = 1039.
    (3,3), a blue site, own B = 791: gval = 2540 2302 3383 4427 3541 3760 4190 2839,
      thold = 2302 + 2213 = 4515 takes all eight: B = (791+624)>>1 + (791+472)>>1 + 6 * ((791+0)>>1)
      + ... in direction order 707 + 631 + 395 + 395 + 395 + 395 + 395 + 849 = 4162,
      R = 824 + 835 + 846 + 704 + 561 + 696 + 830 + 827 = 6123,
      G = 590 + 437 + 529 + 303 + 563 + 731 + 694 + 996 = 4843:
      R = 791 + 1961 / 8 = 1036, G = 791 + 681 / 8 = 876.
    """
    b = np.array([[942, 923, 254, 692, 645, 72], [730, 624, 824, 472, 916, 849], [620, 102, 824, 437, 846, 460],
                  [494, 908, 996, 791, 303, 529], [184, 138, 830, 731, 561, 229], [882, 333, 912, 142, 989, 253]],
                 dtype=np.uint16)
    want = {(2, 2): (824, 851, 837), (2, 3): (756, 437, 695), (3, 2): (1186, 996, 1039), (3, 3): (1036, 876, 791)}
    lit = vr.bayer_vng_literal(b, dr.BAYER_RGGB)
    with _open(tmp_path, b[None], 8) as seq:
        seq.set_debayer(-1, sg.BAYER_INTER_VNG)
        got = seq.read_frame(0)                         # [3][H][W] bottom-up
    for (y, x), rgb in want.items():
        assert tuple(lit[y, x]) == rgb, (y, x)
        assert tuple(got[:, 5 - y, x]) == rgb, (y, x)


HOST_PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include "sg_debayer.h"
/* argv: in out H W pattern method(1 nearest, 2 VNG); in = u16 CFA samples, out = u16 [H][W][3] */
int main(int argc, char **argv) {
	if (argc != 7)
		return 2;
	const int H = atoi(argv[3]), W = atoi(argv[4]), pat = atoi(argv[5]), method = atoi(argv[6]);
	std::vector<uint16_t> cfa((size_t)H * W), rgb((size_t)H * W * 3, 0);
	FILE *f = fopen(argv[1], "rb");
	if (!f || fread(cfa.data(), 2, cfa.size(), f) != cfa.size())
		return 3;
	fclose(f);
	const bool nn = method == 1;
	for (int y = nn ? 0 : 1; y <= H - 2; y++)
		for (int x = nn ? 0 : 1; x <= W - 2; x++) {
			auto at = [&](int dy, int dx) -> int { return cfa[(size_t)(y + dy) * W + x + dx]; };
			int px[3] = {0, 0, 0};
			if (nn)
				sg_nn_px(sg_cfa_color(pat, y, x), sg_cfa_color(pat, y, x + 1), at, px);
			else
				sg_bilinear_px(sg_cfa_color(pat, y, x), sg_cfa_color(pat, y, x + 1), at, px);
			for (int c = 0; c < 3; c++)
				rgb[((size_t)y * W + x) * 3 + c] = (uint16_t)px[c];
		}
	if (!nn) {
		const std::vector<uint16_t> bil(rgb);
		for (int y = 2; y <= H - 3; y++)
			for (int x = 2; x <= W - 3; x++) {
				auto B = [&](int dy, int dx, int c) -> int { return bil[((size_t)(y + dy) * W + x + dx) * 3 + c]; };
				int px[3];
				sg_vng_px_any(pat, y, x, B, px);
				for (int c = 0; c < 3; c++)
					rgb[((size_t)y * W + x) * 3 + c] = (uint16_t)px[c];
			}
	}
	f = fopen(argv[2], "wb");
	if (!f || fwrite(rgb.data(), 2, rgb.size(), f) != rgb.size())
		return 4;
	fclose(f);
	return 0;
}
'''


def test_header_as_plain_host_cxx(tmp_path):
    """csrc/sg_debayer.h built as plain C++17 into a stand-alone program, under AddressSanitizer +
    UBSan where their runtimes are installed (host code only): every pattern, both methods,
    full-range samples and a frame of extremes (all clamps, the largest gradients) == the helper"""
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "siril-0.9_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        san = []
    src = tmp_path / "debayer_host.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "debayer_host"
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", *san, "-I", inc, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    H, W = 13, 18
    extremes = np.random.default_rng(9).choice(np.array([0, 65535], dtype=np.uint16), size=(H, W))
    for k, b in enumerate([_cfa(91, (H, W)), extremes]):
        fin, fout = tmp_path / f"in{k}.bin", tmp_path / f"out{k}.bin"
        b.tofile(fin)
        for tile in range(4):
            for method in (NN, VNG):
                r = subprocess.run([str(exe), str(fin), str(fout), str(H), str(W), str(tile), str(method)],
                                   capture_output=True, text=True)
                assert r.returncode == 0, r.stderr[-4000:]
                got = np.fromfile(fout, dtype=np.uint16).reshape(H, W, 3)
                assert np.array_equal(got, vr.demosaic(b, tile, method, literal=True)), (k, tile, method)


# ---- whole-frame reads: sg_seq_read_frame, sg_seq_read_selection ----

def _frames_with_overshoot(seed, n, shape, tile, hi):
    """n random top-down CFA frames; for 8-bit data the first seed from `seed` on whose frame 0
    has a VNG result (the helper's, before round_to_BYTE) outside the byte range, so the clamp
    has work to do"""
    for s in range(seed, seed + 1000):
        fr = _cfa(s, (n,) + shape, hi)
        if hi > 256 or vr.demosaic(fr[0], tile, VNG).max() > 255:
            return fr
    raise AssertionError("no VNG overshoot found")


@pytest.mark.parametrize("shape", [(6, 6), (21, 30)])
@pytest.mark.parametrize("enc", ["le16", "be16", "u8"])
@pytest.mark.parametrize("color_id,forced", [(8, -1), (9, -1), (10, -1), (11, -1), (8, 3)])
@pytest.mark.parametrize("inter", [NN, VNG])
def test_read_frame_and_selection(tmp_path, inter, color_id, forced, enc, shape):
    """ser_read_frame: debayer() on the whole frame, round_to_BYTE for an 8-bit SER, the flip;
    seq_read_frame_part extracts from that frame"""
    H, W = shape
    depth, flag = (8, 0) if enc == "u8" else (16, 1 if enc == "be16" else 0)
    tile = forced if forced >= 0 else TILE_OF_ID[color_id]
    frames = _frames_with_overshoot(color_id * 100 + H + inter, 2, shape, tile, 256 if depth == 8 else 65536)
    with _open(tmp_path, frames, color_id, depth, flag) as seq:
        seq.set_debayer(forced, inter)
        assert seq.shape == (2, 3, H, W)
        for i in range(2):
            want = vr.frame_memory_order(frames[i], tile, inter, depth)
            if depth == 8 and inter == VNG and i == 0:
                raw = vr.demosaic(frames[i], tile, VNG)
                assert raw.max() > 255 and want.max() == 255        # the clamp changed a sample
            assert np.array_equal(seq.read_frame(i), want), i
            for layer, x, y, w, h in [(0, 0, 0, W, H), (1, 1, 2, W - 2, H - 3), (2, 2, 1, 3, 4)]:
                rc, got = seq.read_selection(layer, i, x, y, w, h)
                assert rc == 0
                assert np.array_equal(got, want[layer, H - y - h:H - y, x:x + w]), (layer, x, y)


# ---- region reads: the widened area demosaiced as an image of its own ----

BANDS_DIFFER = [(0, 4), (2, 4), (4, 5), (5, 7), (6, 1), (7, 1), (18, 2), (16, 3)]
BANDS_AGREE = [(1, 4), (3, 4), (19, 3), (0, 22)]
BANDS_SMALL = [(0, 1), (0, 2), (1, 1), (21, 1), (20, 2)]


@pytest.mark.parametrize("color_id", [9, 11])
def test_region_vng_bands(tmp_path, color_id):
    """ser_read_opened_partial's CFA branch under VNG: every band equals the literal loop on
    its widened area.  The VNG row next to an area edge reads the area's zero bilinear border,
    so some bands differ from the whole frame's rows: a reader that crops the whole-frame
    result fails here, and a stack fed by this reader depends on how its rows were cut."""
    H, W = 22, 16
    tile = TILE_OF_ID[color_id]
    frames = _cfa(color_id, (2, H, W))
    whole = vr.demosaic(frames[1], tile, VNG, literal=True)
    with _open(tmp_path, frames, color_id) as seq:
        seq.set_debayer(-1, sg.BAYER_INTER_VNG)
        for y, h in BANDS_DIFFER + BANDS_AGREE + BANDS_SMALL:
            want = vr.region_band(frames[1], tile, VNG, y, h)
            for layer in range(3):
                rc, got = seq.read_region(layer, 1, 0, y, W, h)
                assert rc == 0, (y, h)
                assert np.array_equal(got, want[:, :, layer]), (y, h, layer)
            same = np.array_equal(want, whole[y:y + h])
            if (y, h) in BANDS_DIFFER:
                assert not same, (y, h)
            if (y, h) in BANDS_AGREE:
                assert same, (y, h)
        # what the small areas give: rows of zeros at columns 2..W-3 from the delay buffer
        rc, got = seq.read_region(1, 1, 0, 0, W, 2)
        assert rc == 0 and not got[1, 2:W - 2].any() and got[1, 1] != 0
        rc, got = seq.read_region(1, 1, 0, 1, W, 1)
        assert rc == 0 and not got[0, 2:W - 2].any()


def test_region_8bit_keeps_overshoot(tmp_path):
    """the region path has no round_to_BYTE: an 8-bit band holds VNG values above 255, where the
    whole-frame read of the same rows is clamped"""
    H, W = 22, 16
    tile = dr.BAYER_RGGB
    frames = _frames_with_overshoot(5, 1, (H, W), tile, 256)
    with _open(tmp_path, frames, 8, depth=8) as seq:
        seq.set_debayer(-1, sg.BAYER_INTER_VNG)
        want = vr.region_band(frames[0], tile, VNG, 0, H)
        assert want.max() > 255
        got = np.stack([seq.read_region(layer, 0, 0, 0, W, H)[1] for layer in range(3)], axis=-1)
        assert np.array_equal(got, want)
        assert seq.read_frame(0).max() == 255


@pytest.mark.parametrize("depth", [8, 16])
def test_region_nearest_equals_whole_frame_rows(tmp_path, depth):
    """the widening (at least 2 rows, or up to the frame's edge) keeps nearest neighbour's zero
    row out of every band: region rows == the literal loop on the area == the whole frame's"""
    H, W = 22, 16
    tile = dr.BAYER_GBRG
    frames = _cfa(77, (1, H, W), 256 if depth == 8 else 65536)
    whole = vr.demosaic(frames[0], tile, NN, literal=True)
    with _open(tmp_path, frames, 10, depth=depth) as seq:
        seq.set_debayer(-1, sg.BAYER_INTER_NEARESTNEIGHBOR)
        for y, h in BANDS_DIFFER + BANDS_AGREE + BANDS_SMALL:
            want = vr.region_band(frames[0], tile, NN, y, h)
            assert np.array_equal(want, whole[y:y + h]), (y, h)
            for layer in range(3):
                rc, got = seq.read_region(layer, 0, 0, y, W, h)
                assert rc == 0 and np.array_equal(got, want[:, :, layer]), (y, h, layer)


def test_region_partial_width_and_bilinear_unchanged(tmp_path):
    """the reference's crop of a partial-width CFA area is garbage (ser.c:907): refused under the
    two new methods; bilinear region reads, partial widths included, are what they were"""
    H, W = 22, 16
    frames = _cfa(12, (1, H, W))
    mem = dr.debayer_frame_memory_order(frames[0], dr.BAYER_BGGR)
    with _open(tmp_path, frames, 11) as seq:
        for inter in (sg.BAYER_INTER_NEARESTNEIGHBOR, sg.BAYER_INTER_VNG):
            seq.set_debayer(-1, inter)
            assert seq.read_region(0, 0, 0, 4, W, 5)[0] == 0
            for x, w in [(1, W - 1), (0, W - 1), (4, 6)]:
                assert seq.read_region(0, 0, x, 4, w, 5)[0] == -1, (inter, x, w)
        for setter in (lambda: seq.set_debayer(-1), lambda: seq.set_debayer(-1, sg.BAYER_INTER_BILINEAR)):
            setter()
            for layer in range(3):
                for x, y, w, h in [(0, 0, W, 4), (0, 5, W, 7), (3, 6, 9, 1), (1, 18, W - 1, 4), (0, 0, W, H)]:
                    rc, got = seq.read_region(layer, 0, x, y, w, h)
                    assert rc == 0
                    assert np.array_equal(got, mem[layer, H - 1 - (y + np.arange(h)), x:x + w]), (layer, x, y)
            assert np.array_equal(seq.read_frame(0), mem)


# ---- refusals ----

def test_refusals(tmp_path):
    lib = sg.load()
    with _open(tmp_path, _cfa(1, (1, 8, 8)), 8, name="a.ser") as seq:
        for inter in (sg.BAYER_INTER_AHD, sg.BAYER_INTER_SUPER_PIXEL, 7, -1):
            assert lib.sg_seq_set_debayer_method(seq.h, -1, inter) == sg.SG_ERR_GENERIC, inter
            with pytest.raises(RuntimeError):
                seq.set_debayer(-1, inter)
        assert lib.sg_seq_set_debayer_method(seq.h, 4, sg.BAYER_INTER_VNG) == sg.SG_ERR_GENERIC   # bad pattern
        info = sg.SeqInfo()
        lib.sg_seq_get_info(seq.h, ctypes.byref(info))
        assert info.nb_layers == 1                      # a refused call leaves the sequence as it was
        assert lib.sg_seq_set_debayer_method(seq.h, -1, sg.BAYER_INTER_VNG) == sg.SG_OK
    for k, shape in enumerate([(5, 8), (8, 5)]):
        with _open(tmp_path, _cfa(2, (1,) + shape), 8, name=f"s{k}.ser") as seq:
            assert lib.sg_seq_set_debayer_method(seq.h, -1, sg.BAYER_INTER_VNG) == sg.SG_ERR_SIZE, shape
            assert lib.sg_seq_set_debayer_method(seq.h, -1, sg.BAYER_INTER_NEARESTNEIGHBOR) == sg.SG_OK
            want = vr.frame_memory_order(_cfa(2, (1,) + shape)[0], dr.BAYER_RGGB, NN, literal=True)
            seq.set_debayer(-1, sg.BAYER_INTER_NEARESTNEIGHBOR)
            assert np.array_equal(seq.read_frame(0), want)
    with _open(tmp_path, _cfa(3, (1, 8, 8)), 0, name="mono.ser") as seq:
        for inter in (sg.BAYER_INTER_BILINEAR, sg.BAYER_INTER_NEARESTNEIGHBOR, sg.BAYER_INTER_VNG):
            assert lib.sg_seq_set_debayer_method(seq.h, -1, inter) == sg.SG_ERR_GENERIC


def test_harness_bayer_inter(tmp_path):
    """the glue's com.debayer.bayer_inter: harness_open_ser_inter and siril_cli --bayer-inter open
    a CFA SER with nearest neighbour or VNG and refuse super-pixel (stacking.c:1321) and AHD"""
    import harness_lib as hl
    lib = hl.load()
    lib.harness_open_ser_inter.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.harness_open_ser_inter.restype = ctypes.c_void_p
    mem = _cfa(4, (2, 8, 10))[:, None]
    path = str(tmp_path / "h.ser")
    write_ser(path, mem, depth=16, color_id=9)
    for inter, ok in [(0, True), (1, True), (2, True), (3, False), (4, False), (9, False)]:
        h = lib.harness_open_ser_inter(os.fsencode(path), -1, inter)
        assert bool(h) == ok, inter
        if h:
            lib.harness_close(h)
        r = subprocess.run([hl.CLI, "--ser", path, "--debayer", "-1", "--bayer-inter", str(inter)],
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (inter, r.stdout, r.stderr)
        if ok:
            assert "2 frames 10 x 8 x 3" in r.stdout


# ---- device load ----

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 6), (21, 30), (T_H - 1, T_W + 1), (2 * T_H + 3, 2 * T_W + 5)])
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("color_id", [8, 9, 10, 11])
@pytest.mark.parametrize("inter", [NN, VNG])
def test_load_device_methods(tmp_path, gpu_ctx, inter, color_id, depth, shape):
    """sg_seq_load_device (k_debayer_nn, k_debayer_vng) == the whole-frame result, at the sizes
    where the halo (6x6), a ragged single tile, a tile seam and a ragged last tile can go wrong,
    into frames 3 H W + 7 apart"""
    import torch
    N, (H, W) = 3, shape
    tile = TILE_OF_ID[color_id]
    frames = _frames_with_overshoot(color_id * 10 + depth + H, N, shape, tile, 256 if depth == 8 else 65536)
    stride = 3 * H * W + 7
    with _open(tmp_path, frames, color_id, depth) as seq:
        seq.set_debayer(-1, inter)
        d = torch.full((N * stride,), 0x5555, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.load_seq_device(seq, d.data_ptr(), frame_stride=stride)
        got = d.cpu().numpy().view(np.uint16).reshape(N, stride)
    for i in range(N):
        want = vr.frame_memory_order(frames[i], tile, inter, depth)
        assert np.array_equal(got[i, :3 * H * W].reshape(3, H, W), want), i
        assert (got[i, 3 * H * W:] == 0x5555).all()     # nothing written between the frames


@pytest.mark.gpu
def test_stack_vng_device(tmp_path, gpu_ctx):
    """a VNG-demosaiced CFA SER loaded on the device and stacked there (SIGMA 3, 3, shifted) ==
    the oracle on the helper's frames; the device load demosaics whole frames, so unlike a stack
    fed by the region reader it does not depend on how rows are cut into bands"""
    import torch
    N, H, W = 12, 26, 40
    mono = orc.synth(N, 1, H, W, seed=23, maxshift=3)
    sx, sy = orc.synth_shifts(N, seed=23, maxshift=3)
    path = str(tmp_path / "cfa_vng.ser")
    write_ser(path, mono, depth=16, color_id=11)        # BGGR
    rgb = np.stack([vr.frame_memory_order(mono[i, 0, ::-1, :], dr.BAYER_BGGR, VNG) for i in range(N)])
    assert not np.array_equal(rgb[0], dr.debayer_frame_memory_order(mono[0, 0, ::-1, :], dr.BAYER_BGGR))
    rc, ref, rej_ref = orc.stack_rejection(rgb, sg.SIGMA, sig=(3.0, 3.0), shiftx=sx, shifty=sy, max_thread=4)
    assert rc == 0
    desc, keep = sg.make_desc(sg.MEAN, N, W, H, 3, rejection=sg.SIGMA, sig=(3.0, 3.0), shiftx=sx, shifty=sy,
                              max_thread=4, max_number_of_rows=H)
    with sg.Seq.open_ser(path) as seq:
        seq.set_debayer(-1, sg.BAYER_INTER_VNG)
        d = torch.zeros(N * 3 * H * W, dtype=torch.int16, device="cuda")
        o = torch.zeros(3 * H * W, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.load_seq_device(seq, d.data_ptr())
        rej, _ = gpu_ctx.stack_device(desc, d.data_ptr(), 3 * H * W, H * W, o.data_ptr(), 0, H)
    assert np.array_equal(o.cpu().numpy().view(np.uint16).reshape(3, H, W), ref)
    assert np.array_equal(rej, rej_ref)
