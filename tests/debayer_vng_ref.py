"""bayer_NearestNeighbor (src/algos/demosaicing.c:177-244), bayer_VNG (:246-420) and
get_debayer_area (:787-842) restated for the tests, on the top-down CFA data.

Each method is here twice: the reference's loop written literally (pointer arithmetic as
indices; VNG in place on the bilinear image behind its three-row delay buffer, any H >= 3 and
W >= 4), and the per-pixel form the library uses (csrc/sg_debayer.h).  The tests check the two
against each other; the literal loops are pure Python and for small frames only, the per-pixel
VNG works on whole arrays, one CFA site of the 2x2 cell at a time.

The VNG term table is the algorithm's data: 64 entries (y1, x1, y2, x2, shift, mask): the
difference of the two positions, shifted, is added to the gradient of every direction whose
bit is set in mask."""
import numpy as np

from debayer_ref import BAYER_BGGR, BAYER_GBRG, BAYER_GRBG, BAYER_RGGB, bayer_bilinear

INTER_BILINEAR, INTER_NEAREST, INTER_VNG, INTER_AHD, INTER_SUPER_PIXEL = range(5)

VNG_TERMS = [
    (-2, -2, 0, -1, 0, 0x01), (-2, -2, 0, 0, 1, 0x01), (-2, -1, -1, 0, 0, 0x01), (-2, -1, 0, -1, 0, 0x02),
    (-2, -1, 0, 0, 0, 0x03), (-2, -1, 0, 1, 1, 0x01), (-2, 0, 0, -1, 0, 0x06), (-2, 0, 0, 0, 1, 0x02),
    (-2, 0, 0, 1, 0, 0x03), (-2, 1, -1, 0, 0, 0x04), (-2, 1, 0, -1, 1, 0x04), (-2, 1, 0, 0, 0, 0x06),
    (-2, 1, 0, 1, 0, 0x02), (-2, 2, 0, 0, 1, 0x04), (-2, 2, 0, 1, 0, 0x04), (-1, -2, -1, 0, 0, 0x80),
    (-1, -2, 0, -1, 0, 0x01), (-1, -2, 1, -1, 0, 0x01), (-1, -2, 1, 0, 1, 0x01), (-1, -1, -1, 1, 0, 0x88),
    (-1, -1, 1, -2, 0, 0x40), (-1, -1, 1, -1, 0, 0x22), (-1, -1, 1, 0, 0, 0x33), (-1, -1, 1, 1, 1, 0x11),
    (-1, 0, -1, 2, 0, 0x08), (-1, 0, 0, -1, 0, 0x44), (-1, 0, 0, 1, 0, 0x11), (-1, 0, 1, -2, 1, 0x40),
    (-1, 0, 1, -1, 0, 0x66), (-1, 0, 1, 0, 1, 0x22), (-1, 0, 1, 1, 0, 0x33), (-1, 0, 1, 2, 1, 0x10),
    (-1, 1, 1, -1, 1, 0x44), (-1, 1, 1, 0, 0, 0x66), (-1, 1, 1, 1, 0, 0x22), (-1, 1, 1, 2, 0, 0x10),
    (-1, 2, 0, 1, 0, 0x04), (-1, 2, 1, 0, 1, 0x04), (-1, 2, 1, 1, 0, 0x04), (0, -2, 0, 0, 1, 0x80),
    (0, -1, 0, 1, 1, 0x88), (0, -1, 1, -2, 0, 0x40), (0, -1, 1, 0, 0, 0x11), (0, -1, 2, -2, 0, 0x40),
    (0, -1, 2, -1, 0, 0x20), (0, -1, 2, 0, 0, 0x30), (0, -1, 2, 1, 1, 0x10), (0, 0, 0, 2, 1, 0x08),
    (0, 0, 2, -2, 1, 0x40), (0, 0, 2, -1, 0, 0x60), (0, 0, 2, 0, 1, 0x20), (0, 0, 2, 1, 0, 0x30),
    (0, 0, 2, 2, 1, 0x10), (0, 1, 1, 0, 0, 0x44), (0, 1, 1, 2, 0, 0x10), (0, 1, 2, -1, 1, 0x40),
    (0, 1, 2, 0, 0, 0x60), (0, 1, 2, 1, 0, 0x20), (0, 1, 2, 2, 0, 0x10), (1, -2, 1, 0, 0, 0x80),
    (1, -1, 1, 1, 0, 0x88), (1, 0, 1, 2, 0, 0x08), (1, 0, 2, -1, 0, 0x40), (1, 0, 2, 1, 0, 0x10),
]
# the eight directions, clockwise from the upper left (bayervng_chood)
VNG_DIRS = [(-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1)]
# the `filters` word of each sensor_pattern (:299-311); FC() reads the colour of a site from it
VNG_FILTERS = {BAYER_BGGR: 0x16161616, BAYER_GRBG: 0x61616161, BAYER_RGGB: 0x94949494, BAYER_GBRG: 0x49494949}


def fc(filters, row, col):
    """FC(row, col) (:276): colour 0 R, 1 G, 2 B of a site; Python's & on a negative int is the
    two's complement one, as in C"""
    return (filters >> (((((row << 1) & 14) + (col & 1))) << 1)) & 3


def cfa_color(tile, y, x):
    """the same from the 2x2 cell of the pattern (the form the library uses)"""
    cell = [[[0, 1], [1, 2]], [[2, 1], [1, 0]], [[1, 2], [0, 1]], [[1, 0], [2, 1]]]
    return cell[tile][y & 1][x & 1]


# ---------------------------------------------------------------------------- nearest neighbour

def bayer_nearest_literal(bayer_img, tile):
    """the reference's row loop; returns interleaved [H][W][3]"""
    sy, sx = bayer_img.shape
    b = bayer_img.astype(np.int64).reshape(-1)
    rgb = np.zeros(3 * sx * sy, dtype=np.int64)
    step, rstep = sx, 3 * sx
    blue = -1 if tile in (BAYER_BGGR, BAYER_GBRG) else 1
    start_with_green = tile in (BAYER_GBRG, BAYER_GRBG)
    imax = sx * sy * 3                                  # "add black border"
    for i in range(sx * (sy - 1) * 3, imax):
        rgb[i] = 0
    iinc = (sx - 1) * 3
    i = (sx - 1) * 3
    while i < imax:
        rgb[i:i + 3] = 0
        i += 3 + iinc
    bi, ri = 0, 1
    height, width = sy - 1, sx - 1
    for _ in range(height):
        bend = bi + width
        if start_with_green:
            rgb[ri - blue] = b[bi + 1]
            rgb[ri] = b[bi + step + 1]
            rgb[ri + blue] = b[bi + step]
            bi += 1
            ri += 3
        while bi <= bend - 2:
            if blue > 0:
                rgb[ri - 1], rgb[ri], rgb[ri + 1] = b[bi], b[bi + 1], b[bi + step + 1]
                rgb[ri + 2], rgb[ri + 3], rgb[ri + 4] = b[bi + 2], b[bi + step + 2], b[bi + step + 1]
            else:
                rgb[ri + 1], rgb[ri], rgb[ri - 1] = b[bi], b[bi + 1], b[bi + step + 1]
                rgb[ri + 4], rgb[ri + 3], rgb[ri + 2] = b[bi + 2], b[bi + step + 2], b[bi + step + 1]
            bi += 2
            ri += 6
        if bi < bend:
            rgb[ri - blue] = b[bi]
            rgb[ri] = b[bi + 1]
            rgb[ri + blue] = b[bi + step + 1]
            bi += 1
            ri += 3
        bi -= width
        ri -= width * 3
        bi += step
        ri += rstep
        blue = -blue
        start_with_green = not start_with_green
    return rgb.astype(np.uint16).reshape(sy, sx, 3)


def nearest_per_pixel(bayer_img, tile):
    """pixel (y, x), y <= H-2 and x <= W-2, from the 2x2 cell whose top-left corner it is"""
    H, W = bayer_img.shape
    b = bayer_img.astype(np.int64)
    out = np.zeros((H, W, 3), dtype=np.int64)
    for y in range(H - 1):
        for x in range(W - 1):
            col = cfa_color(tile, y, x)
            if col != 1:
                out[y, x, col] = b[y, x]
                out[y, x, 1] = b[y, x + 1]
                out[y, x, 2 - col] = b[y + 1, x + 1]
            else:
                rowc = cfa_color(tile, y, x + 1)
                out[y, x, 1] = b[y + 1, x + 1]          # not its own sample
                out[y, x, rowc] = b[y, x + 1]
                out[y, x, 2 - rowc] = b[y + 1, x]
    return out.astype(np.uint16)


# ------------------------------------------------------------------------------------------ VNG

def _round_to_word(t):
    return 0 if t <= 0 else 65535 if t > 65535 else t


def _cdiv(a, n):
    """C's integer division: toward zero"""
    return -((-a) // n) if a < 0 else a // n


def bayer_vng_literal(bayer_img, tile):
    """the reference's loop: bilinear first, then VNG in place, rows written back two rows late
    from the rotating buffer; returns interleaved int64 [H][W][3]"""
    height, width = bayer_img.shape
    assert height >= 3 and width >= 4
    dst = bayer_bilinear(bayer_img, tile).astype(np.int64).reshape(-1)
    filters = VNG_FILTERS[tile]
    code = [[None, None] for _ in range(8)]             # "Precalculate for VNG"
    for row in range(8):
        for col in range(2):
            terms = []
            for y1, x1, y2, x2, weight, grads in VNG_TERMS:
                color = fc(filters, row + y1, col + x1)
                if fc(filters, row + y2, col + x2) != color:
                    continue
                diag = 2 if (fc(filters, row, col + 1) == color and fc(filters, row + 1, col) == color) else 1
                if abs(y1 - y2) == diag and abs(x1 - x2) == diag:
                    continue
                terms.append(((y1 * width + x1) * 3 + color, (y2 * width + x2) * 3 + color, weight,
                              [g for g in range(8) if grads & (1 << g)]))
            hood = []
            for y, x in VNG_DIRS:
                color = fc(filters, row, col)
                if fc(filters, row + y, col + x) != color and fc(filters, row + y * 2, col + x * 2) == color:
                    hood.append(((y * width + x) * 3, (y * width + x) * 6 + color))
                else:
                    hood.append(((y * width + x) * 3, 0))
            code[row][col] = (terms, hood)
    rows3 = [np.zeros((width, 3), dtype=np.int64) for _ in range(3)]    # calloc
    brow = [rows3[0], rows3[1], rows3[2], None]
    row = 2
    while row < height - 2:
        for col in range(2, width - 2):
            pix = (row * width + col) * 3
            terms, hood = code[row & 7][col & 1]
            gval = [0] * 8
            for o1, o2, weight, gs in terms:
                diff = abs(int(dst[pix + o1]) - int(dst[pix + o2])) << weight
                for g in gs:
                    gval[g] += diff
            gmin, gmax = min(gval), max(gval)
            if gmax == 0:
                brow[2][col, :] = dst[pix:pix + 3]
                continue
            thold = gmin + (gmax >> 1)
            sums = [0, 0, 0]
            color = fc(filters, row, col)
            num = 0
            for g in range(8):
                if gval[g] <= thold:
                    for c in range(3):
                        if c == color and hood[g][1]:
                            sums[c] += (int(dst[pix + c]) + int(dst[pix + hood[g][1]])) >> 1
                        else:
                            sums[c] += int(dst[pix + hood[g][0] + c])
                    num += 1
            for c in range(3):
                t = int(dst[pix + color])
                if c != color:
                    t += _cdiv(sums[c] - sums[color], num)
                brow[2][col, c] = _round_to_word(t)
        if row > 3:
            o = 3 * ((row - 2) * width + 2)
            dst[o:o + (width - 4) * 3] = brow[0][2:width - 2].reshape(-1)
        for g in range(4):
            brow[(g - 1) & 3] = brow[g]
        row += 1
    o = 3 * ((row - 2) * width + 2)
    dst[o:o + (width - 4) * 3] = brow[0][2:width - 2].reshape(-1)
    o = 3 * ((row - 1) * width + 2)
    dst[o:o + (width - 4) * 3] = brow[1][2:width - 2].reshape(-1)
    return dst.reshape(height, width, 3)


def vng_per_pixel(bayer_img, tile):
    """the pure form for H >= 6 and W >= 6: every pixel of rows 2..H-3, columns 2..W-3 from the
    5x5 neighbourhood of the bilinear image, the ring kept; one site of the 2x2 cell at a time,
    all its pixels at once.  Returns interleaved int64 [H][W][3]"""
    H, W = bayer_img.shape
    assert H >= 6 and W >= 6
    bil = bayer_bilinear(bayer_img, tile).astype(np.int64)
    out = bil.copy()
    for py in (0, 1):
        for px in (0, 1):
            ys, xs = 2 + py, 2 + px                     # first row / column of this site

            def B(dy, dx, c):
                return bil[ys + dy:H - 2 + dy:2, xs + dx:W - 2 + dx:2, c]
            shape = B(0, 0, 0).shape
            if shape[0] == 0 or shape[1] == 0:
                continue
            gval = np.zeros((8,) + shape, dtype=np.int64)
            for y1, x1, y2, x2, shift, mask in VNG_TERMS:
                color = cfa_color(tile, py + y1, px + x1)
                if cfa_color(tile, py + y2, px + x2) != color:
                    continue
                diag = 2 if (cfa_color(tile, py, px + 1) == color and cfa_color(tile, py + 1, px) == color) else 1
                if abs(y1 - y2) == diag and abs(x1 - x2) == diag:
                    continue
                diff = np.abs(B(y1, x1, color) - B(y2, x2, color)) << shift
                for g in range(8):
                    if mask & (1 << g):
                        gval[g] += diff
            gmin, gmax = gval.min(axis=0), gval.max(axis=0)
            thold = gmin + (gmax >> 1)
            color = cfa_color(tile, py, px)
            sums = np.zeros((3,) + shape, dtype=np.int64)
            num = np.zeros(shape, dtype=np.int64)
            for g, (y, x) in enumerate(VNG_DIRS):
                take = gval[g] <= thold
                half = cfa_color(tile, py + y, px + x) != color
                for c in range(3):
                    v = (B(0, 0, c) + B(2 * y, 2 * x, color)) >> 1 if (c == color and half) else B(y, x, c)
                    sums[c] += np.where(take, v, 0)
                num += take
            for c in range(3):
                t = B(0, 0, color).copy()
                if c != color:
                    d = sums[c] - sums[color]
                    t = t + np.sign(d) * (np.abs(d) // np.maximum(num, 1))      # toward zero
                out[ys:H - 2:2, xs:W - 2:2, c] = np.where(gmax == 0, B(0, 0, c), np.clip(t, 0, 65535))
    return out


# ------------------------------------------------------------------------------- the read paths

def demosaic(bayer_img, tile, inter, literal=False):
    """debayer_buffer (:667-727) of an image of its own: interleaved int64 [H][W][3]"""
    if inter == INTER_NEAREST:
        f = bayer_nearest_literal if literal else nearest_per_pixel
        return f(bayer_img, tile).astype(np.int64)
    assert inter == INTER_VNG
    H, W = bayer_img.shape
    if literal or H < 6 or W < 6:
        return bayer_vng_literal(bayer_img, tile)
    return vng_per_pixel(bayer_img, tile)


def frame_memory_order(bayer_img, tile, inter, depth=16, literal=False):
    """ser_read_frame (ser.c:708-768): debayer() on the whole frame, round_to_BYTE for an 8-bit
    SER (demosaicing.c:755-765), fits_flip_top_to_bottom: planar uint16 [3][H][W], bottom-up"""
    rgb = demosaic(bayer_img, tile, inter, literal)
    if depth <= 8:
        rgb = np.minimum(rgb, 255)
    return np.ascontiguousarray(np.transpose(rgb, (2, 0, 1))[:, ::-1, :]).astype(np.uint16)


def get_debayer_area(area, image):
    """area (x, y, w, h) in the image (w, h) -> (debayer area (x, y, w, h), xoffset, yoffset)"""
    ax, ay, aw, ah = area
    iw, ih = image
    xoff = 3 if ax & 1 else 2
    if ax - xoff < 0:
        dx, xoff = 0, ax
    else:
        dx = ax - xoff
    xend = ax + aw - 1
    right = 2 if xend & 1 else 3
    if xend + right >= iw:
        right = iw - xend - 1
    dw = aw + (ax - dx) + right
    yoff = 3 if ay & 1 else 2
    if ay - yoff < 0:
        dy, yoff = 0, ay
    else:
        dy = ay - yoff
    yend = ay + ah - 1
    bottom = 2 if yend & 1 else 3
    if yend + bottom >= ih:
        bottom = ih - yend - 1
    dh = ah + (ay - dy) + bottom
    assert dx < iw and dy < ih and dh > 2 and dw > 2
    return (dx, dy, dw, dh), xoff, yoff


def region_band(bayer_img, tile, inter, y, h):
    """ser_read_opened_partial's CFA branch (ser.c:820-913) for the full-width band of top-down
    rows y .. y+h-1: the widened area demosaiced with the literal loop as an image of its own,
    no round_to_BYTE, cropped; int64 [h][W][3]"""
    H, W = bayer_img.shape
    (dx, dy, dw, dh), xoff, yoff = get_debayer_area((0, y, W, h), (W, H))
    assert dx == 0 and dw == W and xoff == 0
    rgb = demosaic(bayer_img[dy:dy + dh], tile, inter, literal=True)
    return rgb[yoff:yoff + h]
