"""The seeded cases of the automatic cosmetic correction shared by tests/test_cosme_cpu.py and
tests/test_gpu_cosme.py: frames [N][C][H][W], the parameters, and the literal restatement's answer
(tests/cosme_ref.py), computed once per case and left unchanged.

The main pass works on 64 x 32 tiles (siril-0.9_amd/csrc/sg_cosme.h), so the shapes are one tile
-1 / +1 in each direction, two tiles + 1, an odd width, planes with one dimension <= step, and
runs longer than two tiles that cross tile corners."""
import numpy as np

import cosme_ref as cr

_frames = {}
_literal = {}


def _small(H, W, seed):
    """a tiny plane with one planted hot and one planted cold pixel"""
    rng = np.random.default_rng(seed)
    p = rng.integers(995, 1006, size=(H, W)).astype(np.uint16)
    flat = p.reshape(-1)
    flat[(2 * seed + 2) % flat.size] = 3000
    flat[(2 * seed + 5) % flat.size] = 100
    return p[None, None]


def _layers3(seed):
    """C = 3 with different statistics per layer, two frames"""
    out = np.zeros((2, 3, 36, 70), dtype=np.uint16)
    for f in range(2):
        for c, (level, scale) in enumerate([(1000, 1), (5000, 4), (20000, 16)]):
            p = cr.dense_plane(36, 70, seed + 10 * f + c).astype(np.int64)
            out[f, c] = np.clip((p - 1000) * scale + level, 0, 65535).astype(np.uint16)
    return out


def _fail_layer1():
    fr = np.stack([_layers3(40)[0], _layers3(41)[0], _layers3(42)[1]])
    fr[1, 1] = 0
    return fr


def _all_65535():
    fr = np.zeros((1, 2, 20, 30), dtype=np.uint16)
    fr[0, 0] = cr.dense_plane(20, 30, 5)
    fr[0, 1] = 65535
    return fr


def _chain(H, W, seed, runs):
    return lambda: cr.chain_plane(H, W, seed, runs)[None, None]


def _dense(H, W, seed, n=1):
    return lambda: np.stack([cr.dense_plane(H, W, seed + f)[None] for f in range(n)])


CHAIN_SIG = (3.0, 1.0)

CASES = {
    # planes with one dimension <= step, H x W
    "s_1x7": dict(make=lambda: _small(1, 7, 0), sig=(1.0, 1.0), amount=1.0, is_cfa=False),
    "s_7x1": dict(make=lambda: _small(7, 1, 1), sig=(1.0, 1.0), amount=1.0, is_cfa=False),
    "s_3x3": dict(make=lambda: _small(3, 3, 2), sig=(1.0, 1.0), amount=1.0, is_cfa=False),
    "s_5x7_cfa": dict(make=lambda: _small(5, 7, 3), sig=(1.0, 1.0), amount=1.0, is_cfa=True),
    "s_2x9_cfa": dict(make=lambda: _small(2, 9, 4), sig=(1.0, 1.0), amount=1.0, is_cfa=True),
    # one tile - 1 / + 1 in each direction, two tiles + 1 (odd widths)
    "tile_m1": dict(make=_dense(31, 63, 10), sig=(3.0, 3.0), amount=1.0, is_cfa=False),
    "tile_p1": dict(make=_dense(33, 65, 11), sig=(3.0, 3.0), amount=1.0, is_cfa=False),
    "tile_p1_cfa": dict(make=_dense(33, 65, 12), sig=(3.0, 3.0), amount=1.0, is_cfa=True),
    "tiles2_p1": dict(make=_dense(65, 129, 13), sig=(3.0, 3.0), amount=1.0, is_cfa=False),
    "tiles2_p1_cfa": dict(make=_dense(65, 129, 14), sig=(3.0, 3.0), amount=1.0, is_cfa=True),
    # layers and frames
    "layers3": dict(make=lambda: _layers3(20), sig=(3.0, 3.0), amount=1.0, is_cfa=False),
    "frames3": dict(make=_dense(20, 30, 30, n=3), sig=(3.0, 3.0), amount=1.0, is_cfa=False),
    # chains longer than two tiles, across tile corners
    "chain_h": dict(make=_chain(40, 150, 50, [("h", 5, 32, 140)]), sig=CHAIN_SIG, amount=1.0, is_cfa=False),
    "chain_h_cfa": dict(make=_chain(40, 150, 51, [("h", 5, 31, 140)]), sig=CHAIN_SIG, amount=1.0, is_cfa=True),
    "chain_v": dict(make=_chain(80, 70, 52, [("v", 64, 5, 70)]), sig=CHAIN_SIG, amount=1.0, is_cfa=False),
    "chain_v_cfa": dict(make=_chain(80, 70, 53, [("v", 63, 5, 70)]), sig=CHAIN_SIG, amount=1.0, is_cfa=True),
    "chain_d": dict(make=_chain(92, 130, 54, [("d", 40, 8, 80)]), sig=CHAIN_SIG, amount=1.0, is_cfa=False),
    "chain_d_cfa": dict(make=_chain(92, 130, 55, [("a", 88, 8, 80)]), sig=CHAIN_SIG, amount=1.0, is_cfa=True),
    # a comb of runs two rows apart (four with CFA): the chains couple through the 5 x 5 window
    "chain_comb": dict(make=_chain(44, 150, 56, [("h", 5, y, 140) for y in (28, 30, 32, 34)]), sig=CHAIN_SIG, amount=1.0,
                       is_cfa=False),
    "chain_comb_cfa": dict(make=_chain(48, 150, 57, [("h", 5, y, 140) for y in (24, 28, 32, 36)]), sig=CHAIN_SIG,
                           amount=1.0, is_cfa=True),
    # 5 % random outliers of both signs
    "dense": dict(make=_dense(48, 100, 60), sig=(3.0, 3.0), amount=1.0, is_cfa=False),
    "dense_cfa": dict(make=_dense(48, 100, 61), sig=(3.0, 3.0), amount=1.0, is_cfa=True),
    # parameters
    "cold_off": dict(make=_dense(33, 65, 70), sig=(-1.0, 3.0), amount=1.0, is_cfa=False),
    "hot_off": dict(make=_dense(33, 65, 70), sig=(3.0, -1.0), amount=1.0, is_cfa=False),
    "both_off": dict(make=_dense(33, 65, 70), sig=(-1.0, -1.0), amount=1.0, is_cfa=False),
    "amount_05": dict(make=_dense(33, 65, 71), sig=(3.0, 3.0), amount=0.5, is_cfa=False),
    "amount_03": dict(make=_dense(33, 65, 71), sig=(3.0, 3.0), amount=0.3, is_cfa=False),
    "amount_0": dict(make=_dense(33, 65, 71), sig=(3.0, 3.0), amount=0.0, is_cfa=False),
    # failures
    "fail_layer1": dict(make=_fail_layer1, sig=(3.0, 3.0), amount=1.0, is_cfa=False),
    "all_65535": dict(make=_all_65535, sig=(3.0, 3.0), amount=1.0, is_cfa=False),
}


def frames_of(name):
    if name not in _frames:
        fr = np.ascontiguousarray(CASES[name]["make"](), dtype=np.uint16)
        assert fr.ndim == 4
        fr.setflags(write=False)
        _frames[name] = fr
    return _frames[name]


def literal_of(name):
    """[(corrected frame, result dict)] per frame, from cosme_ref.autodetect_literal"""
    if name not in _literal:
        c = CASES[name]
        _literal[name] = [cr.autodetect_literal(fr, c["sig"], c["amount"], c["is_cfa"]) for fr in frames_of(name)]
    return _literal[name]
