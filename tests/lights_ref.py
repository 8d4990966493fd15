"""NumPy restatement of the light table's construction (include/render_mi355x.h "several lights": apt_build_lights_host), its
invariants, and the scenes with several lights that the tests share, for the tests only.  The renderer that reads the table is
tests/materials_ref.py's (trace(table=...)), and so is the table as the kernels read it (Table)."""
import numpy as np

from materials_ref import DIFF, F, LIGHTS_HEAD as HEAD, LIGHTS_MAGIC as MAGIC, Table

DEV_LIGHTS_MISMATCH = 32


# ---- the table ------------------------------------------------------------------------------------------------------------------
def build_table(spheres, ns, indices=None):
    """apt_build_lights_host restated -> uint32 array, or ValueError where the library refuses.  float64 scalars, one operation at a
    time in the header's order (Python floats ARE IEEE float64; no pairwise numpy sums)."""
    sph = np.asarray(spheres, dtype=F).ravel()[:10 * ns].reshape(10, ns)
    if ns == 0:
        raise ValueError("num_spheres is 0")
    if indices is None:
        g = [k for k in range(ns) if sph[4][k] > 0 or sph[5][k] > 0 or sph[6][k] > 0]
    else:
        g = [int(k) for k in indices]
    if not g:
        raise ValueError("empty")
    if any(not 0 <= k < ns for k in g):
        raise ValueError("out of range")
    if len(set(g)) != len(g):
        raise ValueError("duplicate")
    n = len(g)
    w = []
    W = 0.0
    for k in g:
        e = (float(sph[4][k]) + float(sph[5][k])) + float(sph[6][k])
        p = e * float(sph[0][k])
        p = p if 0.0 < p < float("inf") else 0.0
        w.append(p)
        W = W + p
    by_power = 0.0 < W < float("inf")
    fl = 0.5 / float(n)
    m, S, before = [], 0.0, 0
    for i in range(n):
        a = (0.5 * w[i]) / W if by_power else fl
        S = S + (a + fl)
        mi = 1 << 24 if i + 1 == n else int(np.floor(S * 16777216.0 + 0.5))
        if mi <= before or mi > 1 << 24:
            raise ValueError("a probability below 2^-24")
        m.append(mi)
        before = mi
    nbits = (ns + 31) // 32
    out = np.zeros(HEAD + 3 * n + nbits, dtype=np.uint32)
    bits = np.zeros(nbits, dtype=np.uint32)
    for k in g:
        bits[k >> 5] |= np.uint32(1 << (k & 31))
    out[:5] = [MAGIC, ns, n, out.size, bits[0]]
    out[HEAD:HEAD + n] = g
    mm = np.array(m, dtype=np.int64)
    cdf = mm.astype(F) * F(2.0 ** -24)
    P = np.diff(mm, prepend=0).astype(F) * F(2.0 ** -24)
    invp = F(1) / P
    assert cdf.dtype == F and invp.dtype == F
    out[HEAD + n:HEAD + 2 * n] = cdf.view(np.uint32)
    out[HEAD + 2 * n:HEAD + 3 * n] = invp.view(np.uint32)
    out[HEAD + 3 * n:] = bits
    return out


def check_table_invariants(words):
    t = Table(words)
    m = t.cdf.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(m, np.round(m)) and (np.diff(m, prepend=0.0) >= 1).all() and m[-1] == 2.0 ** 24     # on the grid, increasing, ends at 1
    P = (np.diff(m, prepend=0.0) * 2.0 ** -24).astype(F)
    assert np.array_equal((F(1) / P).view(np.uint32), t.invp.view(np.uint32))
    assert t.listed.sum() == t.n and t.listed[t.idx].all() and len(set(t.idx.tolist())) == t.n
    return t


# ---- scenes the tests share ----------------------------------------------------------------------------------------------------------
def table_of(rows):
    """rows of (radius, centre, emission, albedo) -> the zero-padded [10][Ns] table."""
    rows = np.array(rows, dtype=np.float64)
    rows[:, 0] = rows[:, 0] ** 2
    ns = rows.shape[0]
    out = np.zeros((ns * 10 + 127) // 128 * 128, dtype=np.float32)
    out[:10 * ns] = rows.T.astype(np.float32).ravel()
    return out


def demo_two_lights(gen_data):
    """The demo scene (9 spheres, glass ball) with the mirror ball, sphere 6 (APT_MAT_SPEC), given emission next to the stock light 7."""
    sph, mat = gen_data.gen_spheres_materials()
    sph = np.array(sph, dtype=F)
    sph[:90].reshape(10, 9)[4:7, 6] = [F(3.0), F(6.0), F(9.0)]
    return sph, np.asarray(mat, dtype=np.int32), 9


def furnace(lamp):
    """The white furnace of tests/test_gpu_materials.py (albedo 0.5, emission 0.25, radius 1000 around the camera; render it with
    eps = 0.5); lamp: a small bright sphere inside it as sphere 1."""
    rows = [[1000.0, 50.0, 52.0, 295.6, 0.25, 0.25, 0.25, 0.5, 0.5, 0.5]]
    if lamp:
        rows.append([20.0, 120.0, 200.0, -100.0, 30.0, 20.0, 10.0, 0.0, 0.0, 0.0])
    return table_of(rows), np.full(len(rows), DIFF, dtype=np.int32), len(rows)


def two_lamps(gen_data):
    """The 8-sphere DIFF scene with spheres 6 and 7 both lamps, of different colour and radius (sphere 6 keeps its place: the mirror
    ball's, on the floor; sphere 7 is smallpt's lamp under the ceiling)."""
    sph, mat, ns, _ = gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 8, 7
    sph = gen_data.with_lamps(sph, ns, [6, 7], radius=[4.0, 1.5], centres=[(27.0, 16.5, 47.0), (50.0, 81.6 - 16.5, 81.6)],
                              emission=[(60.0, 30.0, 15.0), 400.0])
    mat = mat.copy()
    mat[6] = DIFF
    return sph, mat, ns


def sixteen_lamps(gen_data, ns=1030, seed=5):
    """gen_scene's big scene with 16 of its small spheres turned into lamps of unequal power (radius 0.6 .. 2.1, emission 20 .. 320)."""
    sph, mat = gen_data.gen_scene_materials(ns, seed=seed)
    idx = [6 + 61 * i for i in range(16)]
    sph = gen_data.with_lamps(sph, ns, idx, radius=[0.6 + 0.1 * i for i in range(16)],
                              emission=[(20.0 * (i + 1), 10.0 * (i + 1), 5.0 * (16 - i)) for i in range(16)])
    return sph, np.asarray(mat, dtype=np.int32), ns, idx


def three_lights_point(j, per):
    """One point of the closed-form scene: a floor sphere under three listed sphere lights, two unoccluded with different radius,
    distance and emission, one below the horizon -> (rays [6][per], table, materials, ns, paths, the closed form per channel)."""
    R, alb = 1000.0, 0.75
    lights = [(2.0, (0.0, 10.0, 0.0), (50.0, 20.0, 5.0)), (1.0, (6.0, 7.0, -3.0), (10.0, 80.0, 40.0)), (3.0, (0.0, -2000.0 - 20.0, 0.0), (70.0, 70.0, 70.0))]
    rows = [[R, 0, -R, 0, 0, 0, 0, alb, alb, alb]] + [[r, *c, *e, 0, 0, 0] for r, c, e in lights]
    sph = table_of(rows)
    mat = np.array([DIFF] * 4, dtype=np.int32)
    px = 2.0 * j - 6.0
    tgt = np.array([px, np.sqrt(R * R - px * px) - R, 0.0])                           # on the floor sphere
    o = tgt + np.array([0.0, 5.0, 0.5])
    dd = (tgt - o) / np.linalg.norm(tgt - o)
    rays = np.tile(np.concatenate([o, dd])[:, None], (1, per)).astype(F)
    paths = np.arange(j * per, (j + 1) * per, dtype=np.uint64)
    nrm = (tgt - np.array([0.0, -R, 0.0])) / R
    want = np.zeros(3)
    for r, c, e in lights[:2]:
        w = np.array(c) - tgt
        dist = np.linalg.norm(w)
        want += alb * np.array(e) * (r / dist) ** 2 * (w @ nrm) / dist
    return rays, sph, mat, 4, paths, want
