"""Scenes of the deposit's reference tests (tests/deposit_reference.py), shared by the run over the CPU oracle
(tests/test_deposit_reference.py) and the run on the device (tests/test_gpu_deposit_reference.py).  A scene is
(spec, inputs for set(), entropy, rand); the smallest shapes at which each path of the deposit exists: tile side 32,
16384 particles per work item, 2048 records per outbox piece."""
import numpy as np

from helpers import frame_sink, make_spec, uniform_plasma

EDGE_GRIDS = [(1, 1), (1, 40), (33, 2), (31, 65), (64, 64)]
EDGE_COUNTS = [5, 4097, 4098]      # one lane; a tail of one particle; a tail of two (one whole lane in fp64)


def _fields(nr, nz, on=True):
    rng = np.random.default_rng(7)
    B = rng.normal(0, 0.5, size=(nr, nz, 3))
    B[..., 2] += 1.0
    E = rng.normal(0, 2e4, size=(nr, nz, 3))
    if not on:
        E, B = np.zeros_like(E), np.zeros_like(B)
    return E, B


def routes(side=160, v_th=0.02, nr=96, nz=72):
    """the scene of tests/test_gpu_rebin_outbox.py: radius 0.5, height 0.4, the frame sink as sink and source, random E and B"""
    spec = make_spec(nr, nz, side, radius=0.5, height=0.4)
    E, B = _fields(nr, nz)
    pos, vel, entropy, rand = uniform_plasma(side * side, spec, seed=8, v_th=v_th)
    return spec, dict(E=E, B=B, position=pos, velocity=vel, sink_mask=frame_sink(nr, nz), source_pdf=frame_sink(nr, nz)), entropy, rand


def spill():
    """128 x 128, 40 000 particles of v_th = 4e-3 in no field: after 20 steps without a re-binning many have left the halo"""
    spec = make_spec(128, 128, 200)
    E, B = _fields(128, 128, on=False)
    pos, vel, entropy, rand = uniform_plasma(200 * 200, spec, seed=52, v_th=4e-3)
    return spec, dict(E=E, B=B, position=pos, velocity=vel, sink_mask=frame_sink(128, 128), source_pdf=frame_sink(128, 128)), entropy, rand


def hand_placed(nr, nz, T):
    """(position, velocity, names): the edge cases of the cell rule, every coordinate a value of T (radius = height = 1, so
    set() stores them as given)"""
    k = max(1, nr // 2)
    rows = [
        ("r = 0", (0.0, 0.0, 0.5)),
        ("r = 1", (1.0, 0.0, 0.25)),
        ("z = 1", (0.5, 0.0, 1.0)),
        ("r = 1 and z = 1", (0.0, -1.0, 1.0)),
        ("r > 1", (0.75, 0.75, 0.5)),
        ("z < 0", (0.25, 0.0, -0.125)),
        ("NaN", (np.nan, 0.25, 0.5)),
        ("r = k / nr", (float(T(k) / T(nr)), 0.0, 0.75)),
        ("z = 0", (0.0, 0.5, 0.0)),
        ("just inside r = 1", (float(np.nextafter(T(1), T(0))), 0.0, 0.5)),
    ]
    pos = np.array([p for _, p in rows], dtype=np.float64)
    rng = np.random.default_rng(nr * 1000 + nz)
    vel = rng.normal(0, 1e-3, size=pos.shape).astype(T).astype(np.float64)
    return pos, vel, [n for n, _ in rows]


def edges(nr, nz, count, T, seed=3):
    """`count` particles on an nr x nz grid: for count = 5 the first five hand-placed ones (r = 0 among them), otherwise all of
    them and uniform random ones.  No field, nothing absorbed."""
    spec = make_spec(nr, nz, 1)
    hp, hv, _ = hand_placed(nr, nz, T)
    if count <= len(hp):
        pos, vel = hp[:count], hv[:count]
    else:
        rng = np.random.default_rng(seed)
        n = count - len(hp)
        r, th = np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
        z = rng.random(n)
        if nr * nz < 8:     # so few cells that they would hold more than 1000 particles each (deposit_reference.CELL_LIMIT):
            z = 5 * z - 2   # four in five are clipped
        p = np.stack([r * np.cos(th), r * np.sin(th), z], axis=1).astype(T).astype(np.float64)
        pos = np.concatenate([hp, p])
        vel = np.concatenate([hv, rng.normal(0, 1e-3, size=(n, 3)).astype(T).astype(np.float64)])
    rng = np.random.default_rng(seed + 1)
    entropy = rng.random(1024 * 1024 * 4, dtype=np.float32)
    rand = rng.random((count, 4), dtype=np.float32)
    E, B = _fields(nr, nz, on=False)
    return spec, dict(E=E, B=B, position=pos, velocity=vel, sink_mask=np.ones((nr, nz)), source_pdf=np.ones((nr, nz))), entropy, rand


def raster(T, nr=40, nz=24, n=3000, seed=11):
    """particles up to six cells outside every edge of the unit square (a sprite reaches 5.5), a band of them at tiny r (the
    only way to column -1), one at r = 0, and some exactly on pixel edges and centres; slow, in no field"""
    spec = make_spec(nr, nz, 1)
    rng = np.random.default_rng(seed)
    r = rng.random(n) * (1 + 6.0 / nr)
    r[:200] = rng.random(200) * 1e-3 / nr
    r[200:400] = 1 + rng.random(200) * 6.0 / nr
    z = rng.random(n) * (1 + 12.0 / nz) - 6.0 / nz
    z[400:600] = -rng.random(200) * 6.0 / nz
    z[600:800] = 1 + rng.random(200) * 6.0 / nz
    r[800:900] = rng.integers(0, 2 * nr + 1, 100) / (2.0 * nr)          # pixel edges and centres
    z[900:1000] = rng.integers(0, 2 * nz + 1, 100) / (2.0 * nz)
    th = 2 * np.pi * rng.random(n)
    pos = np.stack([r * np.cos(th), r * np.sin(th), z], axis=1)
    pos[800:900, 0], pos[800:900, 1] = r[800:900], 0.0
    pos[0] = (0.0, 0.0, 0.5)
    pos = pos.astype(T).astype(np.float64)
    vel = rng.normal(0, 2e-4, size=(n, 3)).astype(T).astype(np.float64)
    entropy = rng.random(1024 * 1024 * 4, dtype=np.float32)
    rand = rng.random((n, 4), dtype=np.float32)
    E, B = _fields(nr, nz, on=False)
    return spec, dict(E=E, B=B, position=pos, velocity=vel, sink_mask=np.ones((nr, nz)), source_pdf=np.ones((nr, nz))), entropy, rand


def cic():
    """70 x 45, 14 400 particles uniform over the whole cylinder (so within half a cell of every edge), random E and B"""
    return routes(side=120, v_th=0.02, nr=70, nz=45)
