"""CPU-only, on the restatement alone: the scenes of tests/degenerate_scenes.py reach the rules they were built for, so that a green run
of tests/test_gpu_degenerate_scenes.py means something.  For every scene and light mode (4096 aimed rays, depth 6, eps 1e-4, seed 3):

  bad      no path meets a bad material word
  NaN      at most 1 / 16 of the paths of `values` / `values8` contain a NaN (more would hide a failure behind NaN == NaN); none elsewhere
  length   the finite scenes are closed: every path traces `depth` segments, shadow segments not counted
  ties     twins*, cluster40, tiles1030: at least 1 % of the paths have a segment whose smallest t is attained by two or more spheres
           of different material (counted on a local copy of _intersect's t matrix)
  lights   nested, lights, in each of the two sampling modes (plain takes no sample): at least 32 sample attempts of a DIFF bounce find
           the point inside the light (ok false) and at least 32 shadow segments end on a sphere that shares the chosen light's record
           without being it
  mutants  five wrong renderers each change an output bit in a scene that the test names: _intersect keeping the LAST minimum, the skip
           applied to every sphere that shares the skip sphere's record, light_sample with ok = True, the table's noem without
           g != kprev, roulette with np.fmax (which passes over a NaN throughput)

The counters wrap mr._intersect and mr.light_sample and read the bounce's own variables (live, k, j, bounce, rows) from the calling frame
of _trace_chunk: tests/test_restatement_frozen.py holds that function to recorded bytes, so the names stay.  materials_ref.py itself
is not changed; the mutants are patched in from here."""
import inspect
import sys

import numpy as np
import pytest

import degenerate_scenes as ds
import materials_ref as mr
from gpu_harness import host  # noqa: F401

F, U = np.float32, np.uint64
DEPTH, EPS, SEED = 6, 1e-4, 3
MODES = ("plain", "nee", "table")
TIE_SCENES = ("twins", "cluster40", "tiles1030", "twins8")
LIGHT_SCENES = ("nested", "lights")


_BUILT = {}


def built(host, name):
    if name not in _BUILT:
        d = ds.build(host.gen_data, name)
        _BUILT[name] = (d, host.gen_data.build_lights(d.sph, d.ns, d.lights))
    return _BUILT[name]


def trace(host, name, mode, rr=0):
    d, table = built(host, name)
    return mr.trace(d.rays, d.sph, d.mat, d.ns, DEPTH, EPS, SEED, np.arange(d.rays.shape[1], dtype=U), None, rr, light=d.light,
                    nee=mode == "nee", table=table if mode == "table" else None, gloss=bool(mr.flags_of(d.mat)))


def t_matrix(o, d, geo, eps):
    """A local copy of _intersect's t matrix [paths][spheres], before the skip."""
    cx, cy, cz, r2 = geo
    ocx, ocy, ocz = cx[None, :] - o[0][:, None], cy[None, :] - o[1][:, None], cz[None, :] - o[2][:, None]
    b = ocx * d[0][:, None]
    b = b + ocy * d[1][:, None]
    b = b + ocz * d[2][:, None]
    c = ocx * ocx
    c = c + ocy * ocy
    c = c + ocz * ocz
    c = c - r2[None, :]
    disc = b * b
    disc = disc - c
    q = np.sqrt(disc)
    t0, t1 = b - q, b + q
    t = np.where(t0 > eps, t0, t1)
    return mr.f32(np.where(t > eps, t, mr.MISS))


def intersect(o, d, geo, eps, skip, last=False, by_record=False):
    """_intersect, with the two wrong rules at hand: the LAST minimum, and the skip applied to every sphere of the skip sphere's record."""
    t = t_matrix(o, d, geo, eps)
    rows = np.nonzero(skip >= 0)[0]
    if by_record:
        rec = np.stack(geo).view(np.uint32)                              # [4][Ns] bit patterns
        shares = (rec[:, skip[rows]][:, :, None] == rec[:, None, :]).all(axis=0)   # [rows][Ns]
        t[rows] = np.where(shares, mr.MISS, t[rows])
    t[rows, skip[rows]] = mr.MISS
    idx = t.shape[1] - 1 - np.argmin(t[:, ::-1], axis=1) if last else np.argmin(t, axis=1)
    tmin = t[np.arange(t.shape[0]), idx]
    return tmin, np.where(tmin < mr.MISS, idx, -1)


class Probe:
    """Counts, over one mr.trace, what the bounce decides; changes nothing."""

    def __init__(self, d):
        self.codes = np.asarray(d.mat).astype(np.int64) & 0xFF
        self.n = d.rays.shape[1]
        self.tie = np.zeros(self.n, dtype=bool)
        self.inside = self.twin_end = self.shadow = 0
        self._intersect, self._light_sample = mr._intersect, mr.light_sample

    def intersect(self, o, d, geo, eps, skip):
        out = self._intersect(o, d, geo, eps, skip)
        f = sys._getframe(1).f_locals
        if f.get("skip") is skip:                                        # a bounce segment of _trace_chunk
            t = t_matrix(o, d, geo, eps)
            rows = np.nonzero(skip >= 0)[0]
            t[rows, skip[rows]] = mr.MISS
            at_min = (t == out[0][:, None]) & (out[0] < mr.MISS)[:, None]
            lo = np.where(at_min, self.codes[None, :], 99).min(axis=1)
            hi = np.where(at_min, self.codes[None, :], -1).max(axis=1)
            self.tie[f["paths"].astype(np.int64)] |= f["live"] & (at_min.sum(axis=1) >= 2) & (lo != hi)
        else:                                                            # a light's shadow segment: rows of the bounce
            ks, j = out[1], f["j"][f["rows"]]
            rec = np.stack(geo).view(np.uint32)
            g = np.where(ks < 0, 0, ks)
            self.shadow += ks.size
            self.twin_end += int(((ks >= 0) & (ks != j) & (rec[:, g] == rec[:, j]).all(axis=0)).sum())
        return out

    def light_sample(self, h, nl, nkey, bounce, lc, lr2):
        out = self._light_sample(h, nl, nkey, bounce, lc, lr2)
        f = sys._getframe(1).f_locals
        self.inside += int((f["bounce"] & (f["j"] != f["k"]) & ~out[0]).sum())
        return out


@pytest.fixture(scope="module")
def runs(host):
    """Every scene in every light mode without roulette, the `values` scenes with it as well -> {(scene, mode, rr): (L, bad, segments, Probe)}."""
    out = {}
    for name in ds.NAMES:
        d, _ = built(host, name)
        for mode in MODES:
            for rr in ((0, 2) if name.startswith("values") else (0,)):
                probe = Probe(d)
                with pytest.MonkeyPatch.context() as mp:
                    mp.setattr(mr, "_intersect", probe.intersect)
                    mp.setattr(mr, "light_sample", probe.light_sample)
                    out[name, mode, rr] = trace(host, name, mode, rr) + (probe,)
    return out


def test_scenes_are_what_they_say(host):
    for name in ds.NAMES:
        d, table = built(host, name)
        tab = d.sph[:10 * d.ns].reshape(10, d.ns)
        assert d.ns == {"tiles1030": 1030, "twins8": 8, "values8": 8}.get(name, 97) and d.mat.size == d.ns
        assert d.rays.shape == (6, ds.N_RAYS) and d.rays.dtype == F and np.isfinite(d.rays).all()
        for (lo, hi), o in zip(ds.ROOM, d.rays[:3]):
            assert (o >= lo).all() and (o <= hi).all()
        assert np.isfinite(tab).all() == (name in ds.FINITE)
        t = mr.Table(table)
        assert t.idx.tolist() == d.lights and d.light in d.lights
        if name != "tiles1030":                                          # the reference room's walls, bit for bit
            room = np.asarray(host.gen_data.gen_spheres(), dtype=F)[:80].reshape(10, 8)
            walls = [0, 1, 2, 3, 4, 7 if name == "twins8" else 5]       # twins8: the emitter has the ceiling's record
            assert np.array_equal(tab[0:4, walls].view(np.uint32), room[0:4, :6].view(np.uint32))
    tw = built(host, "twins")[0].sph[:970].reshape(10, 97)
    assert len({tw[0:4, k].tobytes() for k in range(10, 20)}) == 1 and len({tw[7:10, k].tobytes() for k in range(10, 20)}) == 10
    assert (tw[4:7, 32] > 0).all() and not tw[4:7, 30].any() and (tw[0, 40:46] == 0).all()
    c40 = built(host, "cluster40")[0]
    assert len({c40.sph[:970].reshape(10, 97)[0:4, k].tobytes() for k in range(10, 50)}) == 1 and len(set(c40.mat[10:50].tolist())) == 3
    t1030 = built(host, "tiles1030")[0]
    tab = t1030.sph[:10300].reshape(10, 1030)
    assert tab[0:4, 1023].tobytes() == tab[0:4, 1024].tobytes() and t1030.mat[1023] != t1030.mat[1024]
    v = built(host, "values")[0]
    assert mr.flags_of(v.mat) == mr.FLAG_GLOSS and {ds.GLOSS_MIN, ds.GLOSS_MAX} <= set(v.mat.tolist())
    assert mr.decode([ds.GLOSS_MIN, ds.GLOSS_MAX], True)[1].tolist() == [2.0 ** -16, 65535 * 2.0 ** -16]


def test_the_builder_accepts_a_listed_light_of_radius_zero(host):
    """Its power is 0, so it keeps the uniform half of its probability: 0.5 / n."""
    d, table = built(host, "lights")
    t = mr.Table(table)
    i = d.lights.index(40)
    assert d.sph[:970].reshape(10, 97)[0, 40] == 0 and t.listed[40] and abs(t.prob()[i] - 0.5 / t.n) <= 2.0 ** -24


def test_no_bad_word_few_nan_and_full_length(runs):
    for (name, mode, rr), (L, bad, seg, probe) in sorted(runs.items()):
        n = L.shape[1]
        nan = int(np.isnan(L).any(axis=0).sum())
        mean = (seg - probe.shadow) / n
        print("%-10s %-5s rr %d: NaN paths %4d, segments per path %.4f, shadow segments %6d" % (name, mode, rr, nan, mean, probe.shadow))
        assert not bad.any(), (name, mode)
        assert nan <= n // 16, (name, mode, nan)
        if name in ds.FINITE:
            assert nan == 0 and np.isfinite(L).all(), (name, mode, nan)
            assert mean >= DEPTH, (name, mode, mean)
        else:
            assert nan > 0, (name, mode)                                 # the NaN albedo is reached


def test_ties_between_spheres_of_different_material_are_reached(runs):
    for name in TIE_SCENES:
        for mode in MODES:
            share = float(runs[name, mode, 0][3].tie.mean())
            print("%-10s %-5s: %.2f %% of the paths have a tie between different materials" % (name, mode, 100 * share))
            assert share >= 0.01, (name, mode, share)


def test_points_inside_a_light_and_twins_of_a_light_are_reached(runs):
    for name in LIGHT_SCENES:
        for mode in ("nee", "table"):
            probe = runs[name, mode, 0][3]
            print("%-7s %-5s: %4d sample attempts inside the light, %5d of %5d shadow segments end on a twin of the light"
                  % (name, mode, probe.inside, probe.twin_end, probe.shadow))
            assert probe.inside >= 32 and probe.twin_end >= 32, (name, mode, probe.inside, probe.twin_end)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def _without_kprev():
    """_trace_chunk with the table's noem lacking `g != kprev`."""
    src = inspect.getsource(mr._trace_chunk)
    assert src.count("& (g != kprev) ") == 1
    scope = dict(vars(mr))
    exec(compile(src.replace("& (g != kprev) ", ""), "<_trace_chunk without g != kprev>", "exec"), scope)
    return scope["_trace_chunk"]


def _roulette_fmax(T, alive, key, bounce):
    q = np.fmax(np.fmax(T[0], T[1]), T[2])
    act = alive & (q > F(0))
    p = np.where(q < F(0.05), F(0.05), q)
    p = np.where(p > F(0.95), F(0.95), p)
    with np.errstate(over="ignore"):
        h = mr.splitmix64(key + U(0x9E3779B97F4A7C15) * U(bounce + 1))
    u = (h >> U(40)).astype(F) * F(2.0 ** -24)
    kill = act & (u >= p)
    inv = F(1) / p
    return [np.where(kill, F(0), np.where(act, t * inv, t)) for t in T]


def _ok_true(h, nl, nkey, bounce, lc, lr2, inner=mr.light_sample):
    ok, l, cosl, wgt = inner(h, nl, nkey, bounce, lc, lr2)
    return np.ones_like(ok), l, cosl, wgt


# mutant -> (what to patch, with what, the scene, mode and rr_start that show it)
MUTANTS = {
    "the last minimum wins a tie": ("_intersect", lambda: lambda *a: intersect(*a, last=True), ("twins", "plain", 0)),
    "the skip goes by record": ("_intersect", lambda: lambda *a: intersect(*a, by_record=True), ("twins8", "plain", 0)),
    "a sample from inside the light": ("light_sample", lambda: _ok_true, ("twins", "nee", 0)),
    "noem without g != kprev": ("_trace_chunk", _without_kprev, ("lights", "table", 0)),
    "roulette by fmax": ("roulette", lambda: _roulette_fmax, ("values", "plain", 2)),
}


def differs(a, b):
    """-> per path: at least one output bit differs, a NaN on both sides counting as equal."""
    return ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any(axis=0)


def test_the_local_copy_is_the_restatement(host, runs):
    for name in ("twins", "values8"):
        d, _ = built(host, name)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(mr, "_intersect", intersect)
            L, _, seg = trace(host, name, "table")
        assert not differs(L, runs[name, "table", 0][0]).any() and seg == runs[name, "table", 0][2]


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_changes_the_image(host, runs, monkeypatch, mutant):
    attr, make, (name, mode, rr) = MUTANTS[mutant]
    monkeypatch.setattr(mr, attr, make())
    L, _, _ = trace(host, name, mode, rr)
    changed = int(differs(L, runs[name, mode, rr][0]).sum())
    print("%s: %d paths of %s (%s, rr_start %d) change" % (mutant, changed, name, mode, rr))
    assert changed > 0, (mutant, name, mode)
