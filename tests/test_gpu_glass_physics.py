"""GPU: glass and mirror shading of the material renderer against the expectation tree of tests/physics_ref.py, which shares no text
with the kernels or their restatements, and -- on the same buffers -- bit for bit against the restatements.

16 rays x 16384 copies in buffer mode (262 144 paths of depth 7 per launch): every lane of every wave holds the same ray and differs
from its neighbours by its path index alone, so the lanes of a wave diverge only through their random branch at each glass hit.  The
scenes, the rays, the two rules (5 standard errors; 1e-6 where all copies agree) and what they were measured at on the restatements are
in tests/test_glass_physics_cpu.py; the kernels equal the restatements bit for bit, so the same figures hold here.

Forms: box8 (the 8-sphere form), box9 by tiles, box9 through its grid; entries: plain, APT_FLAG_NEE (a wall as the light) and a light
table of two walls, each with and without APT_FLAG_RR.  The walls have albedo 0, so nothing is gathered after a wall hit and all six
entries have the expectation of the plain one.  box8_glow (the glass ball also emits) is the scene in which a path that ends at a total
internal reflection, instead of reflecting, shows: see physics_ref.box8_glow."""
import numpy as np
import pytest

import lights_ref as lr
import materials_ref as mr
import physics_ref as ph
from gpu_harness import apt, assert_bits_equal, dev  # noqa: F401

pytestmark = pytest.mark.gpu

N = 16384
DEPTH = 7
RAY_SEED, RENDER_SEED = 5, 1             # as tests/test_glass_physics_cpu.py, which says why the render seed is 1
EPS = 1e-4
LIGHT, TABLE_LIGHTS = 0, [0, 2]          # walls


class Work:
    """What the cases share, each piece computed once: the rays, the trees, the restatements' colours, the scenes on the device and
    the colours of every launch (the grid form is compared with the tile form's)."""

    def __init__(self, apt):
        self.apt = apt
        self.rays16 = ph.rays(RAY_SEED)
        self.rays = ph.copies(self.rays16, N)
        self.d_rays = dev(self.rays.ravel())
        self.paths = np.arange(16 * N, dtype=np.uint64)
        self.scenes, self.trees, self.want, self.dev, self.got = {}, {}, {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = getattr(ph, name)()
        return self.scenes[name]

    def tree(self, name):
        if name not in self.trees:
            self.trees[name] = ph.tree(self.rays16, DEPTH, self.scene(name))
        return self.trees[name]

    def restated(self, name, mode, rr):
        key = (name, mode, rr)
        if key not in self.want:
            sc = self.scene(name)
            kw = {"plain": {}, "nee": dict(light=LIGHT, nee=True), "lights": dict(table=lr.build_table(sc.table, sc.ns, TABLE_LIGHTS))}[mode]
            L, bad, _ = mr.trace(self.rays, sc.table, sc.materials, sc.ns, DEPTH, EPS, RENDER_SEED, self.paths, rr_start=2 if rr else 0, gloss=False, **kw)
            assert not bad.any()
            self.want[key] = L
        return self.want[key]

    def device(self, name, grid):
        import torch
        key = (name, grid)
        if key not in self.dev:
            apt, sc = self.apt, self.scene(name)
            table = apt.gen_data.build_lights(sc.table, sc.ns, TABLE_LIGHTS)
            assert np.array_equal(table, lr.build_table(sc.table, sc.ns, TABLE_LIGHTS))
            d = dict(sph=dev(sc.table), mat=dev(sc.materials, np.int32), lights=dev(table.view(np.int32)), grid=None, flags=0)
            if grid:
                hgrid = apt.gen_data.build_grid(sc.table, sc.ns)
                d["flags"] = apt.gen_data.grid_flags(hgrid, sc.ns)
                assert d["flags"] == apt.APT_FLAG_GRID_SLOTS
                d["grid"] = torch.from_numpy(hgrid.view(np.int32)).cuda()
            self.dev[key] = d
        return self.dev[key]

    def launch(self, name, grid, mode, rr):
        """One launch -> float32 [3][16 N]; the status word is clean after it."""
        import torch
        key = (name, grid, mode, rr)
        if key not in self.got:
            apt, sc, d = self.apt, self.scene(name), self.device(name, grid)
            flags = d["flags"] | (apt.APT_FLAG_NEE if mode == "nee" else 0) | (apt.APT_FLAG_RR if rr else 0)
            p = apt.make_params(128, 128, 4, depth=DEPTH, num_spheres=sc.ns, light_index=LIGHT, eps=EPS, seed=RENDER_SEED, flags=flags,
                                rr_start=2 if rr else 0, accel=d["grid"].data_ptr() if grid else 0)
            assert p.num_paths == 16 * N
            colors = apt.render.render_paths(p, self.d_rays, d["sph"], materials=d["mat"], lights=d["lights"] if mode == "lights" else None)
            torch.cuda.synchronize()
            apt.render.check_device_status()
            self.got[key] = colors.cpu().numpy()
        return self.got[key]


@pytest.fixture(scope="module")
def work(apt):
    return Work(apt)


def _check(work, name, grid, mode, rr):
    got = work.launch(name, grid, mode, rr)
    c = ph.compare(got, work.tree(name), N)
    print("%s%s %-6s%s  max |z| %.2f at %s over %d components, all-equal error %.2e at %s" % (
        name, " grid" if grid else "", mode, " rr" if rr else "", c["zmax"], c["z_at"], c["differing"], c["exact"], c["exact_at"]))
    assert c["finite"]
    assert c["zmax"] <= ph.Z_CAP and c["exact"] <= ph.EXACT_TOL
    assert c["differing"] >= 8
    assert_bits_equal(got, work.restated(name, mode, rr))
    return got


FORMS = [("box8", False), ("box9", False), ("box9", True)]


@pytest.mark.parametrize("rr", [False, True], ids=["", "rr"])
@pytest.mark.parametrize("mode", ["plain", "nee", "lights"])
@pytest.mark.parametrize("name,grid", FORMS, ids=["box8", "box9-tiles", "box9-grid"])
def test_tree_and_restatement(work, name, grid, mode, rr):
    got = _check(work, name, grid, mode, rr)
    assert not got[:, 12 * N:].any()                                      # the trapped rays: exactly dark
    if grid:
        assert_bits_equal(got, work.launch(name, False, mode, rr))              # the grid form is the tile form


def test_a_total_internal_reflection_reflects(work):
    """The glass ball emits: a trapped ray shows exactly depth * GLOW, not the GLOW of a path that ended at its first hit."""
    got = _check(work, "box8_glow", False, "plain", False)
    assert np.array_equal(got[:, 12 * N:], np.repeat(np.float32(DEPTH) * np.array(ph.GLOW, dtype=np.float32)[:, None], 4 * N, axis=1))
