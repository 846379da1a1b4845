"""A numpy model of the pedestrian map as a function of the pedestrian vector (imgenv_ped_maps_draw, csrc/ped_draw.h), written from
the reference's _draw_ped_map (yaml_env.py:409-427) and the definition in include/imgenv.h.  Python floats are float64: the float32
inputs are widened exactly, every operation below is one IEEE float64 operation in the order the definition gives, and ``//`` is
Python's own float floor division -- the one the reference's ``(tmx - r) // resolution`` runs."""
import math

import numpy as np

ONE = np.float32(1.0).view(np.uint32)


def geometry(Hp, Wp, ped_image_r=0.3):
    """(Hp, Wp, resolution, r, r ** 2) as the reference holds them (yaml_env.py:164, 425)"""
    return int(Hp), int(Wp), 6.0 / Hp, float(ped_image_r), float(ped_image_r) ** 2.0


def count(v0, PV):
    """the pedestrians of a row: v[0] truncated and clamped to [0, (PV - 1) / 7]; 0 where it is negative or not finite"""
    v0 = float(v0)
    if not math.isfinite(v0) or v0 < 0:
        return 0
    return min(int(v0), (PV - 1) // 7)


def draw_row(v, geo):
    """the map of one row ``v`` (float32 [PV]) as uint32 words [3, Hp, Wp]: words, so that -0.0f and every NaN payload stay"""
    Hp, Wp, res, r, r2 = geo
    v = np.ascontiguousarray(v, np.float32)
    words = v.view(np.uint32)
    img = np.zeros((3, Hp, Wp), np.uint32)
    for j in range(count(v[0], len(v))):
        px, py = float(v[7 * j + 1]), float(v[7 * j + 2])
        if px > 3 or px < -3 or py > 3 or py < -3:
            continue
        if math.isnan(px) or math.isnan(py):
            continue
        tmx, tmy = -px + 3, -py + 3
        x0, x1 = int((tmx - r) // res), int((tmx + r) // res)
        y0, y1 = int((tmy - r) // res), int((tmy + r) // res)
        for jj in range(x0, x1):
            for kk in range(y0, y1):
                if jj < 0 or jj >= Hp or kk < 0 or kk >= Wp:
                    continue
                dx, dy = (jj + 0.5) * res - tmx, (kk + 0.5) * res - tmy
                if dx * dx + dy * dy < r2:
                    img[:, jj, kk] = ONE, words[7 * j + 3], words[7 * j + 4]
    return img


def draw(vectors, geo, rows=None):
    """float32 [n, 3, Hp, Wp]: map i from row ``rows[i]`` of ``vectors`` (below 0: zeros), or from row i.  A row that occurs
    several times is drawn once."""
    vectors = np.ascontiguousarray(vectors, np.float32)
    src = np.arange(len(vectors)) if rows is None else np.asarray(rows, np.int64)
    Hp, Wp = geo[0], geo[1]
    out = np.zeros((len(src), 3, Hp, Wp), np.uint32)
    done = {}
    for i, s in enumerate(src):
        if s < 0:
            continue
        if int(s) not in done:
            done[int(s)] = draw_row(vectors[int(s)], geo)
        out[i] = done[int(s)]
    return out.view(np.float32)


# ---- the synthetic rows of the tests (tests/test_ped_draw_model.py on the host, tests/test_gpu_ped_draw.py on the device) ----
def ped(px, py, vx, vy):
    return (px, py, vx, vy, 0.3, 0.47, math.hypot(px, py))


def row(PV, peds, n=None):
    v = np.zeros(PV, np.float32)
    v[0] = len(peds) if n is None else n
    for q, p in enumerate(peds):
        v[1 + 7 * q:8 + 7 * q] = p
    return v


def synthetic_rows(PV=1 + 7 * 80):
    """(vectors float32 [m, PV], names): every case of the list in tests/test_gpu_ped_draw.py"""
    f32 = np.float32
    up, down = np.nextafter(f32(3), f32(4)), np.nextafter(f32(-3), f32(-4))
    rng = np.random.default_rng(17)
    cases = [("n = 0", row(PV, []))]
    cases.append(("one disc at the centre", row(PV, [ped(0.0, 0.0, 0.25, -0.5)])))
    for name, (x, y) in {"edge +x": (2.9, 0.1), "edge -x": (-2.9, 0.1), "edge +y": (0.1, 2.9), "edge -y": (0.1, -2.9), "corner ++": (2.85, 2.85),
                         "corner +-": (2.85, -2.85), "corner -+": (-2.85, 2.85), "corner --": (-2.85, -2.85)}.items():
        cases.append(("cut by " + name, row(PV, [ped(x, y, 0.1, 0.2)])))
    for name, (x, y) in {"px = 3": (3.0, 0.0), "px = -3": (-3.0, 0.0), "py = 3": (0.0, 3.0), "py = -3": (0.0, -3.0), "both 3": (3.0, -3.0)}.items():
        cases.append((name + " (drawn)", row(PV, [ped(x, y, 0.3, 0.4)])))
    for name, (x, y) in {"px > 3": (up, 0.0), "px < -3": (down, 0.0), "py > 3": (0.0, up), "py < -3": (0.0, down)}.items():
        cases.append((name + " (skipped)", row(PV, [ped(x, y, 0.3, 0.4), ped(1.0, 1.0, 0.6, 0.7)])))
    two = [ped(0.5, 0.5, 0.11, 0.12), ped(0.7, 0.6, 0.21, 0.22)]
    three = two + [ped(0.6, 0.35, 0.31, 0.32)]
    cases += [("two overlapping", row(PV, two)), ("two overlapping, reversed", row(PV, two[::-1])),
              ("three overlapping", row(PV, three)), ("three overlapping, reversed", row(PV, three[::-1]))]
    pile = [ped(*(rng.uniform(-0.4, 0.4, 2) + (1.5, -1.0)), *rng.uniform(-1, 1, 2)) for _ in range(80)]
    cases.append(("80 piled on a few cells", row(PV, pile)))
    spread = [ped(*rng.uniform(-3.2, 3.2, 2), *rng.uniform(-1, 1, 2)) for _ in range(80)]
    cases.append(("80 spread over the box and beyond", row(PV, spread)))
    cases.append(("v[0] above the cap", row(PV, spread, n=1000)))
    cases.append(("v[0] far above the cap", row(PV, spread, n=3e9)))
    cases.append(("v[0] infinite", row(PV, spread, n=np.inf)))
    cases.append(("v[0] negative", row(PV, spread, n=-3)))
    cases.append(("v[0] NaN", row(PV, spread, n=np.nan)))
    cases.append(("v[0] fractional", row(PV, three, n=2.9)))
    cases.append(("v[0] below the pedestrians written", row(PV, three, n=1)))
    for name, (x, y) in {"px NaN": (np.nan, 0.0), "py NaN": (0.0, np.nan), "px inf": (np.inf, 0.0), "py -inf": (0.0, -np.inf)}.items():
        cases.append((name, row(PV, [ped(x, y, 0.3, 0.4), ped(-1.0, 1.0, 0.6, 0.7)])))
    cases.append(("-0.0f velocities", row(PV, [ped(1.0, -1.0, -0.0, 0.0), ped(-1.0, -1.0, 0.0, -0.0)])))
    cases.append(("NaN velocity", row(PV, [ped(2.0, 2.0, np.nan, 1.0)])))
    names, vectors = zip(*cases)
    return np.stack(vectors).astype(np.float32), list(names)


def crowded_rows(PV=1 + 7 * 300):
    """(vectors, names) of rows with more pedestrians than k_ped_draw's workgroup has lanes (256): further rounds of the lanes"""
    rng = np.random.default_rng(23)
    spread = [ped(*rng.uniform(-3.1, 3.1, 2), *rng.uniform(-1, 1, 2)) for _ in range(300)]
    pile = [ped(*(rng.uniform(-0.5, 0.5, 2) + (-1.0, 2.0)), *rng.uniform(-1, 1, 2)) for _ in range(300)]
    late = [ped(9.0, 9.0, 0.5, 0.5)] * 299 + [ped(0.2, -0.3, 0.7, -0.7)]  # only the last pedestrian, of the second round, is in the box
    cases = [("300 spread", row(PV, spread)), ("300 piled", row(PV, pile)), ("256 of 300", row(PV, pile, n=256)), ("257 of 300", row(PV, pile, n=257)),
             ("the 300th alone in the box", row(PV, late)), ("the 300th not counted", row(PV, late, n=299))]
    names, vectors = zip(*cases)
    return np.stack(vectors).astype(np.float32), list(names)


def synthetic_index(m, n, seed=3):
    """int32 [n] over m rows: -1s and repeats among them"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, m, n).astype(np.int32)
    if n >= 3:
        rows[rng.integers(0, n, max(1, n // 7))] = -1
        rows[0], rows[1] = -1, max(int(rows[1]), 1)
        rows[-1] = rows[1]
    return rows
