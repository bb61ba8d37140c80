"""DFT registration (sg_register_dft_u16) launched at the sides and on the re-run paths where the
host plan (siril-0.9_amd/csrc/sg_reg_plan.hpp, checked on its own by test_reg_plan_cpu.py) reaches
a limit, with answers that do not come from the code under test.

A. Large and edge sides.  Frames are exact circular rolls of one non-periodic scene.  By
   Cauchy-Schwarz sum_n a(n + k) a(n) < sum_n a(n)^2 for every k != 0 unless a is periodic, so the
   exact correlation of ref with roll(ref, (dy, dx)) has a strict, unique maximum at the roll: the
   expected shifts are _wrap(+-dx, S), _wrap(+-dy, S), the sign read from the oracle at S = 64.
   The runner-up of that scene is 0.933 of the maximum (numpy, float64, S = 4096, 4093, 4032), far
   outside the fp32 tolerance 2^-15, so the main passes decide and nothing is re-run.  Sides:
   512, 1024, 4096 (half spectra; 4096: 16 elements per thread, the 147 KB fp64 strip), 4000
   (mixed radix, fused columns at 2 x 512 threads), 4032 = 7 x 576 and 3920 (a radix-7 pass, 576
   threads, the most a mixed-radix plan takes up to 4096: too wide to fuse, so the three-kernel
   column sequence), 2047, 2049, 4095 (Bluestein, m = 4096 / 8192 / 8192, the chirp's wrap m - j
   tight against S - 1 at 2047 and 4095).  What rolls cannot show, frames that are no roll of the
   reference, is compared with an independent float64 FFT (numpy) at 4096, 4032 and 2049.

B. fp32 -> fp64 re-runs of several pairs (reg_rerun_fp64 and its subset tables).  A pair is
   re-run when !(v - v2 > 2^e S^2 ||ref|| ||img||), e = -15 in fp32 and -32 in fp64 (sg_reg_tol,
   k_reg_final).  With g = (max - runner-up) / (||ref|| ||img||) of the exact circular correlation
   sum_n ref(n + k) img(n): a roll of the reference 59950 + e (e uniform in 0..100) has
   g ~ 2.3e-7, ambiguous in fp32 and clear in fp64; a roll of e alone has g ~ 2.4e-4, clear in
   both.  test_rerun_premise computes g for every frame of every case on the CPU and holds it a
   factor 4 away from each tolerance, which covers the passes' own error (1.3e-6 of the scale per
   fp32 transform, the comment above sg_reg_tol), so each verdict, and with it the number of
   re-run pairs, is known beforehand.  Rolls of the same pedestal reference also go through the
   generic route (fp64, nothing re-run): their gap of 2.3e-7 asks a thousand times more of the
   mixed-radix and Bluestein transforms than the scene of part A.

C. Bookkeeping on the generic route at its smallest sides (105 mixed radix, 97 Bluestein): a
   reference that is not frame 0, masks leaving an odd and an even count, a single frame.  The
   frames are distinct rolls of the scene, so the oracle's answer differs from frame to frame.

The premise test runs without a GPU, so the GPU tests carry the mark one by one instead of a
module-wide pytestmark.
"""
import functools
import os

import numpy as np
import pytest

import oracle_lib as orc
import sirilgpu as sg

gpu = pytest.mark.gpu


# ---- helpers (modelled on test_gpu_edges.py and test_gpu_register.py) ----

def _with_env(env, fn):
    """fn(ctx) on a context created while the knobs are set (knobs are read at sg_init)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with sg.Context() as ctx:
            return fn(ctx)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _same_q(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _scene(S, seed):
    rng = np.random.default_rng(seed)
    scene = rng.integers(0, 3000, size=(S, S)).astype(np.float64)
    scene = (scene + np.roll(scene, 1, 0) + np.roll(scene, 1, 1)) / 3
    scene[S // 3:S // 3 + 5, S // 5:S // 5 + 5] += 30000
    return scene


def _roll_shifts(S, rolls):
    sc = _scene(S, 3).astype(np.uint16)
    return np.stack([np.roll(sc, (dy, dx), axis=(0, 1)) for dx, dy in rolls])


def _wrap(v, S):
    v = v % S
    return v - S if v > S // 2 else v


@functools.lru_cache(maxsize=None)
def _signs():
    """sign convention of (shiftx, shifty) for a circular roll (dx, dy), from the oracle"""
    rx, ry, _ = orc.register_dft(_roll_shifts(64, [(0, 0), (3, -5)]))
    kx, ky = int(rx[1]) // 3, int(ry[1]) // -5
    assert abs(kx) == 1 and abs(ky) == 1 and rx[1] == 3 * kx and ry[1] == -5 * ky
    return kx, ky


def _expected_shifts(S, rolls, ref=0):
    """the rolls relative to the reference's, wrapped as register_shift_dft wraps them"""
    kx, ky = _signs()
    ex = np.array([_wrap(kx * (dx - rolls[ref][0]), S) for dx, _ in rolls], np.int32)
    ey = np.array([_wrap(ky * (dy - rolls[ref][1]), S) for _, dy in rolls], np.int32)
    return ex, ey


def _raw_quality(sel):
    return np.array([orc.quality(f) for f in sel])


def _normalized_quality(rq, ref=0, included=None):
    """normalizeQualityData with register_shift_dft's min / max: seeded by the reference, then the
    registered frames in index order"""
    n = len(rq)
    keep = [f for f in range(n) if included is None or included[f]]
    q_min = q_max = rq[ref]
    for f in keep:
        if f == ref:
            continue
        q = rq[f]
        q_max = q if q > q_max else q_max
        q_min = q_min if q_min < q else q
    with np.errstate(invalid="ignore", divide="ignore"):
        return (rq - q_min) / np.float64(q_max - q_min)


def _numpy_shifts(sel, ref=0):
    """register_shift_dft's arg-max with an independent FFT (numpy pocketfft, float64, real
    transforms: half the work of the complex ones)"""
    n, S, _ = sel.shape
    R = np.fft.rfft2(sel[ref].astype(np.float64))
    sx, sy = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for f in range(n):
        if f == ref:
            continue
        c = np.fft.irfft2(R * np.conj(np.fft.rfft2(sel[f].astype(np.float64))), s=(S, S))
        y, x = divmod(int(np.argmax(c)), S)
        sy[f] = y - S if y > S // 2 else y
        sx[f] = x - S if x > S // 2 else x
    return sx, sy


def _main_fp32():
    """the main passes of a power-of-two side run in fp32 unless the suite itself runs under
    SG_REG_FP=64 (as test_gpu_register.py allows): only then is anything re-run in fp64"""
    return os.environ.get("SG_REG_FP", "32") == "32"


def _assert_stats(st, reruns, resolved=0, unresolved=0):
    """the call's re-run and tie counts; `reruns` is what fp32 main passes hand to fp64"""
    got = (st.reg_fp64_reruns, st.reg_ties_resolved, st.reg_ties_unresolved)
    assert got == (reruns if _main_fp32() else 0, resolved, unresolved), got


# ---- A. large and edge sides ----

def _side_rolls(S, n=5):
    """the reference, a small mixed-sign roll, one of several hundred pixels, and the wrap boundary
    on both axes: h = S // 2 is the largest shift reported positive, h + 1 must come back negative.
    As inputs -h is the roll h of an even side and the roll h + 1 of an odd one, so the two
    boundary frames are chosen by parity to put both distinct rolls on both axes"""
    h = S // 2
    rolls = [(0, 0), (3, -5), (-300, 411), (h, h + 1), (h + 1, -h) if S % 2 == 0 else (-h, h)]
    if n == 4:      # a half-empty last pair: the boundary frames stay
        rolls = [rolls[0], rolls[3], rolls[4], rolls[2]]
    return rolls[:n]


@functools.lru_cache(maxsize=1)
def _roll_case(S, n):
    """one case at a time: 4096, the only side two tests share, comes last in the side list and
    the test that shares it follows and drops it (5 x 4096^2 u16 are 160 MB)"""
    rolls = _side_rolls(S, n)
    sel = _roll_shifts(S, rolls)
    return rolls, sel, _raw_quality(sel)


def _check_rolls(got, S, rolls, rq, ref=0):
    gx, gy, gq = got
    ex, ey = _expected_shifts(S, rolls, ref)
    assert np.array_equal(gx, ex) and np.array_equal(gy, ey), (S, ref, gx, ex, gy, ey)
    assert _same_q(gq, _normalized_quality(rq, ref)), (gq, rq)


HALF_SIDES = [512, 1024, 4096]
MIXED_SIDES = [4000, 4032, 3920]
BLUESTEIN_SIDES = [2047, 2049, 4095]
REF2_SIDES = (4032, 2047)       # one mixed-radix and one Bluestein side also with ref_image = 2
ROLL_CASES = [(S, 5) for S in MIXED_SIDES + BLUESTEIN_SIDES + HALF_SIDES]
ROLL_CASES.insert(-1, (2049, 4))        # 4096 stays last


@gpu
@pytest.mark.parametrize("S,n", ROLL_CASES)
def test_register_rolls_at_side(gpu_ctx, S, n):
    """every frame's shift is its roll and its quality the oracle's QualityEstimate; the main passes
    decide these frames themselves (no fp64 re-run, no tie)"""
    rolls, sel, rq = _roll_case(S, n)
    _check_rolls(gpu_ctx.register_dft(sel), S, rolls, rq)
    _assert_stats(gpu_ctx.stats(), 0)
    if S in REF2_SIDES and n == 5:
        _check_rolls(gpu_ctx.register_dft(sel, ref_image=2), S, rolls, rq, ref=2)
        _assert_stats(gpu_ctx.stats(), 0)


@gpu
def test_register_rolls_4096_fp64_route(gpu_ctx):
    """SG_REG_FP=64 at S = 4096: the fp64 half-spectrum kernels at their largest LDS strip
    (2 x (4608 + 1) x 16 B) give the same shifts and qualities"""
    S = 4096
    rolls, sel, rq = _roll_case(S, 5)

    def run(c):
        return c.register_dft(sel), c.stats()
    try:
        got, st = _with_env({"SG_REG_FP": "64"}, run)
        _check_rolls(got, S, rolls, rq)
        _assert_stats(st, 0)
    finally:
        _roll_case.cache_clear()


@gpu
@pytest.mark.parametrize("S", [4096, 4032, 2049])
def test_register_non_roll_frames_at_side(gpu_ctx, S):
    """frames that are no roll of the reference (translated windows of a scene, non-periodic
    edges): the arg-max of an independent float64 FFT"""
    sel = orc.synth(3, 1, S, S, seed=S, maxshift=12)[:, 0].copy()
    gx, gy, _ = gpu_ctx.register_dft(sel)
    nx, ny = _numpy_shifts(sel)
    assert np.array_equal(gx, nx) and np.array_equal(gy, ny), (gx, nx, gy, ny)


def _periodic_pair(S, dx, dy, seed):
    """ref periodic with period S/2 along x, img = ref circularly translated by (dy, dx):
    the correlation has two exactly equal maxima, at kx and kx + S/2"""
    rng = np.random.default_rng(seed)
    half = rng.integers(500, 3000, size=(S, S // 2)).astype(np.int64)
    ref = np.concatenate([half, half], axis=1)
    img = np.roll(ref, (dy, dx), axis=(0, 1))
    return ref, img


@gpu
def test_register_tie_rerun_on_fresh_context_4096(gpu_ctx):
    """an exact tie at S = 4096 on a FRESH context: the fp32 pair goes to fp64 in a work buffer no
    earlier call has grown (the fp64 plane, 256 MiB, is twice the fp32 pair plane), stays a tie
    there and is decided by the exact integer correlations: the lowest index among equals"""
    S = 4096
    ref, img = _periodic_pair(S, 3, 5, seed=S)
    sel = np.stack([ref, img]).astype(np.uint16)
    with sg.Context() as c:
        gx, gy, _ = c.register_dft(sel)
        st = c.stats()
    k1 = ((-5) % S, (-3) % S)
    k2 = (k1[0], (k1[1] + S // 2) % S)
    e1, e2 = orc.xcorr_at(ref, img, *k1), orc.xcorr_at(ref, img, *k2)
    assert e1 == e2
    lo = min(k1[0] * S + k1[1], k2[0] * S + k2[1])
    y, x = divmod(lo, S)
    assert (gx[1], gy[1]) == (x - S if x > S // 2 else x, y - S if y > S // 2 else y)
    assert st.reg_ties_resolved >= 1
    if _main_fp32():
        assert st.reg_fp64_reruns >= 1


# ---- B. fp64 re-runs of more than one pair ----

PEDESTAL = 59950
AMB_LO, AMB_HI, CLEAR_LO = 2.0 ** -30, 2.0 ** -17, 2.0 ** -13

# frame kinds: R the reference, A ambiguous in fp32 against it, C clear, X excluded.  The re-run
# count is the number of pairs (registered frames two by two, in index order) holding an A.
#   six:     pairs (1,2) (3,4) (5,-), frame 2 clear                             -> 3 pairs
#   eight:   pairs (1,2) (3,4) (5,6) (7,-), pair (3,4) clear: the subset {0,2,3} -> 3 pairs
#   eight_ref4: the same eight frames against frame 4, frame 6 excluded: pairs (0,1) (2,3) (5,7).
#            Frame 4 is a roll of e alone, and against it every frame is clear, with or without
#            the pedestal (a constant adds P sum(e) to every correlation entry: the gap stays
#            S^2 var(e), the scale drops to ||e|| ||img||)                       -> 0 pairs
#   ped_ref4: eight frames whose reference, frame 4, carries the pedestal: pairs (0,1) (2,3)
#            (5,7), pair (2,3) clear: the subset {0,2} behind a reference slot   -> 2 pairs
RERUN_CASES = {
    "six": ("RACAAA", 0, 3),
    "eight": ("RAACCAAA", 0, 3),
    "eight_ref4": ("CCCCRCXC", 4, 0),
    "ped_ref4": ("AACCRAXA", 4, 2),
}
# which frames carry the pedestal (a roll of 59950 + e; the others are rolls of e alone)
RERUN_PEDESTAL = {
    "six": "110111",
    "eight": "11100111",
    "eight_ref4": "11100111",
    "ped_ref4": "11001111",
}
RERUN_ROLLS = [(0, 0), (3, -5), (-7, 2), (11, 13), (-1, -1), (6, -20), (-15, 9), (25, 4)]


def _pair_count(kinds):
    todo = [k for k in kinds if k in "AC"]
    return sum("A" in todo[i:i + 2] for i in range(0, len(todo), 2))


def _rerun_case(name, S):
    """(sel, rolls, ref, included or None, re-run pairs)"""
    kinds, ref, reruns = RERUN_CASES[name]
    ped = RERUN_PEDESTAL[name]
    assert _pair_count(kinds) == reruns and kinds[ref] == "R" and len(ped) == len(kinds)
    rng = np.random.default_rng(1000 + S)
    e = rng.integers(0, 101, size=(S, S))
    rolls = RERUN_ROLLS[:len(kinds)]     # a reference other than frame 0 is itself rolled
    sel = np.stack([np.roll(e + (PEDESTAL if ped[f] == "1" else 0), (dy, dx), axis=(0, 1))
                    for f, (dx, dy) in enumerate(rolls)]).astype(np.uint16)
    inc = None
    if "X" in kinds:
        inc = np.array([k != "X" for k in kinds], np.int32)
    return sel, rolls, ref, inc, reruns


def _gap(a, A, img):
    """(g, arg-max (y, x)) of the exact circular correlation sum_n a(n + k) img(n), float64
    (A = rfft2(a))"""
    S = a.shape[0]
    b = img.astype(np.float64)
    c = np.fft.irfft2(A * np.conj(np.fft.rfft2(b)), s=(S, S))
    k = int(np.argmax(c))
    top = c.flat[k]
    c.flat[k] = -np.inf
    return (top - c.max()) / (np.linalg.norm(a) * np.linalg.norm(b)), divmod(k, S)


def _check_premise(sel, kinds, rolls, ref):
    S = sel.shape[1]
    ex, ey = _expected_shifts(S, rolls, ref)
    a = sel[ref].astype(np.float64)
    A = np.fft.rfft2(a)
    for f, kind in enumerate(kinds):
        if kind in "RX":
            continue
        g, (y, x) = _gap(a, A, sel[f])
        assert (_wrap(x, S), _wrap(y, S)) == (ex[f], ey[f]), (S, f, x, y)
        if kind == "A":
            assert AMB_LO < g < AMB_HI, (S, f, g)
        else:
            assert g > CLEAR_LO, (S, f, g)


def _pedestal_pair_4096():
    S = 4096
    e = np.random.default_rng(4096).integers(0, 101, size=(S, S))
    rolls = [(0, 0), (-1234, 2049)]
    ref = (e + PEDESTAL).astype(np.uint16)
    return np.stack([ref, np.roll(ref, rolls[1][::-1], axis=(0, 1))]), rolls


@pytest.mark.parametrize("S", [64, 2048])
@pytest.mark.parametrize("name", list(RERUN_CASES))
def test_rerun_premise(name, S):
    """CPU only: every ambiguous frame's gap lies between the fp64 and the fp32 tolerance, every
    clear frame's above the fp32 one, a factor 4 away each, and the exact arg-max is the roll"""
    sel, rolls, ref, _, _ = _rerun_case(name, S)
    _check_premise(sel, RERUN_CASES[name][0], rolls, ref)


def test_rerun_premise_4096():
    sel, rolls = _pedestal_pair_4096()
    _check_premise(sel, "RA", rolls, 0)


@gpu
@pytest.mark.parametrize("S", [64, 2048])
@pytest.mark.parametrize("name", list(RERUN_CASES))
def test_register_reruns_several_pairs(gpu_ctx, name, S):
    """the pairs holding an ambiguous frame, and only those, are re-run in fp64, in one batch
    (default), or one pair at a time (SG_REG_BATCH=1 and 2: B64 = 1); every frame's shift is its
    roll, also the clear frame's that shares a re-run pair; fp64 decides, so no tie is counted;
    SG_REG_FP=64 gives the same answers without a re-run"""
    sel, rolls, ref, inc, reruns = _rerun_case(name, S)
    ex, ey = _expected_shifts(S, rolls, ref)
    eq = _normalized_quality(_raw_quality(sel), ref, inc)
    keep = np.ones(len(sel), bool) if inc is None else inc.astype(bool)

    def run(c):
        return c.register_dft(sel, ref_image=ref, included=inc), c.stats()

    def check(tag, res, want):
        (gx, gy, gq), st = res
        assert np.array_equal(gx[keep], ex[keep]) and np.array_equal(gy[keep], ey[keep]), (tag, gx, ex, gy, ey)
        assert _same_q(gq[keep], eq[keep]), (tag, gq, eq)
        _assert_stats(st, want)
    check("default", run(gpu_ctx), reruns)
    check("batch1", _with_env({"SG_REG_BATCH": "1"}, run), reruns)
    check("batch2", _with_env({"SG_REG_BATCH": "2"}, run), reruns)
    check("fp64", _with_env({"SG_REG_FP": "64"}, run), 0)


@gpu
def test_register_rerun_on_fresh_context_4096(gpu_ctx):
    """one pedestal pair at S = 4096 on a fresh context: the first fp32 -> fp64 re-run at the
    largest side, in a work buffer sized by this call alone; fp64 decides; the shift is the roll
    and the qualities are the oracle's, as under SG_REG_FP=64 without a re-run"""
    sel, rolls = _pedestal_pair_4096()
    ex, ey = _expected_shifts(4096, rolls)
    eq = _normalized_quality(_raw_quality(sel))

    def run(c):
        return c.register_dft(sel), c.stats()
    for env, want in (({}, 1), ({"SG_REG_FP": "64"}, 0)):
        (gx, gy, gq), st = _with_env(env, run)
        assert np.array_equal(gx, ex) and np.array_equal(gy, ey), (env, gx, ex, gy, ey)
        assert _same_q(gq, eq), (env, gq, eq)
        _assert_stats(st, want)


# The scene of part A leaves its runner-up 6.7 % below the maximum, so passes wrong by a part in a
# thousand still put the maximum at the roll: a radix-7 pass reading every twiddle one table entry
# late passes every roll and numpy case of part A at 4032 and 3920.  The pedestal frames ask more.
#   - The generic route is fp64 throughout and re-runs nothing.  A roll of the pedestal reference
#     leaves a gap of 2.3e-7 of the scale: any error of its transforms above that moves the arg-max.
#   - The fp32 half-spectrum passes must decide a clear frame (a roll of e alone, gap 2.4e-4)
#     themselves, without a re-run: their error has to stay below that gap, 300 times less than
#     the scene allows, at the sides part B does not visit.
GENERIC_PEDESTAL_SIDES = [97, 105, 2047, 2049, 3920, 4000, 4032, 4095]
FP32_CLEAR_SIDES = [512, 1024, 4096]


def _pedestal_rolls(S, clear=False):
    """the pedestal reference and two rolls of it (clear: of e alone)"""
    h = S // 2
    rolls = [(0, 0), (h, h + 1), (-300 % S, 411 % S)]
    e = np.random.default_rng(2000 + S).integers(0, 101, size=(S, S))
    ref = e + PEDESTAL
    sel = [ref] + [np.roll(e if clear else ref, (dy, dx), axis=(0, 1)) for dx, dy in rolls[1:]]
    return np.stack(sel).astype(np.uint16), rolls


@pytest.mark.parametrize("S,clear", [(S, False) for S in GENERIC_PEDESTAL_SIDES] + [(S, True) for S in FP32_CLEAR_SIDES])
def test_pedestal_rolls_premise(S, clear):
    """CPU only.  The correlation of the reference with a roll of itself (or of e alone, which
    differs from it by a constant) is one and the same plane moved to the roll, so the first
    frame's gap is every frame's: a factor 4 above the tolerance of the passes that decide it"""
    sel, rolls = _pedestal_rolls(S, clear)
    _check_premise(sel[:2], "RC" if clear else "RA", rolls[:2], 0)


@gpu
@pytest.mark.parametrize("S", GENERIC_PEDESTAL_SIDES)
def test_register_pedestal_rolls_generic_side(gpu_ctx, S):
    """rolls of the pedestal reference through the mixed-radix (105, 4000 fused, 4032 and 3920
    unfused) and Bluestein passes (97, 2047, 2049, 4095): the shifts are the rolls, decided by the
    fp64 passes"""
    sel, rolls = _pedestal_rolls(S)
    gx, gy, _ = gpu_ctx.register_dft(sel)
    ex, ey = _expected_shifts(S, rolls)
    assert np.array_equal(gx, ex) and np.array_equal(gy, ey), (S, gx, ex, gy, ey)
    _assert_stats(gpu_ctx.stats(), 0)


@gpu
@pytest.mark.parametrize("S", FP32_CLEAR_SIDES)
def test_register_clear_frames_fp32_side(gpu_ctx, S):
    """rolls of e alone against the pedestal reference: the fp32 passes decide them, no re-run"""
    sel, rolls = _pedestal_rolls(S, clear=True)
    gx, gy, _ = gpu_ctx.register_dft(sel)
    ex, ey = _expected_shifts(S, rolls)
    assert np.array_equal(gx, ex) and np.array_equal(gy, ey), (S, gx, ex, gy, ey)
    _assert_stats(gpu_ctx.stats(), 0)


# ---- C. bookkeeping on the generic route ----

# no roll puts the scene's bright block across an edge, where QualityEstimate gives NaN and the
# normalisation makes every quality NaN: the qualities stay finite and tell the frames apart too
C_ROLLS = [(0, 0), (3, -5), (-7, 2), (11, 13), (-1, -1), (6, -20), (16, -9), (25, 4)]


def _small_case(S, n):
    """distinct rolls of the scene, the first one none: against any reference every frame has a
    shift of its own, so a pair loaded from, or a result scattered to, the wrong frame shows"""
    return _roll_shifts(S, C_ROLLS[:n])


def _assert_oracle(gpu_ctx, sel, ref=0, inc=None):
    gx, gy, gq = gpu_ctx.register_dft(sel, ref_image=ref, included=inc)
    rx, ry, rq = orc.register_dft(sel, ref_image=ref, included=inc)
    keep = np.ones(len(sel), bool) if inc is None else np.asarray(inc, bool)
    # the expected answer tells the registered frames apart: no shift is zero, no two are equal
    todo = [f for f in range(len(sel)) if keep[f] and f != ref]
    want = [(int(rx[f]), int(ry[f])) for f in todo]
    assert (0, 0) not in want and len(set(want)) == len(want), want
    assert len(sel) == 1 or (np.isfinite(rq[keep]).all() and len(set(rq[keep])) == keep.sum()), rq
    ex, ey = _expected_shifts(sel.shape[1], C_ROLLS[:len(sel)], ref)
    assert np.array_equal(rx[todo], ex[todo]) and np.array_equal(ry[todo], ey[todo]), (rx, ex, ry, ey)
    assert np.array_equal(gx[keep], rx[keep]) and np.array_equal(gy[keep], ry[keep]), (gx, rx, gy, ry)
    assert _same_q(gq[keep], rq[keep]), (gq, rq)
    assert gx[ref] == 0 and gy[ref] == 0


@gpu
@pytest.mark.parametrize("S", [105, 97])
def test_register_generic_reference_not_first(gpu_ctx, S):
    """six frames against frame 3: the reference's slot behind the pairs, its own shift 0"""
    _assert_oracle(gpu_ctx, _small_case(S, 6), ref=3)


@gpu
@pytest.mark.parametrize("S", [105, 97])
@pytest.mark.parametrize("mask,ref,todo", [((1, 0, 1, 1, 0, 1, 1), 2, 4), ((1, 1, 0, 1, 0, 0, 1, 0), 0, 3)],
                         ids=["four_to_register", "three_to_register"])
def test_register_generic_included_mask(gpu_ctx, S, mask, ref, todo):
    """an even count to register (two full pairs) and an odd one (a last pair with no second
    frame), the reference inside the mask"""
    inc = np.array(mask, np.int32)
    assert inc.sum() - 1 == todo and inc[ref]
    _assert_oracle(gpu_ctx, _small_case(S, len(mask)), ref=ref, inc=inc)


@gpu
@pytest.mark.parametrize("S", [105, 97, 64])
def test_register_single_frame(gpu_ctx, S):
    """n = 1, nothing to register: shift 0, the quality as the oracle gives it"""
    _assert_oracle(gpu_ctx, _small_case(S, 1))
