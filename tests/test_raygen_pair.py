"""Ray-generate of the two-paths-per-lane frame kernel: both rays of a lane's pair in one routine (pt_core.h camera_ray_pair), the
generator states by addition, and the direction from ONE refined reciprocal square root that is accepted only where it provably rounds
to the float32 the reference's float64 sqrt and divisions give (pt_core.h fast_direction).
CPU: the accept rule on >= 10^7 vectors with a stand-in for v_rsq_f64; the states against the generator's definition; the headline
kernel's ISA.  GPU: the accept rule with the instruction itself."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascendpathtracing_amd", "csrc")
HEADLINE = "_ZN12_GLOBAL__N_119render_frame_kernelILi0ELi0ELi8ELb0ELb1EEEvPKfNS_9FrameArgsENS_9TraceArgsEN3apt8LeafProgE"
D = 256                                 # pt_core.h kDirMidD: the half-width of the rejected window around a float32 midpoint, float64 ulps
OFFSETS = (0, 1, -1, D - 1, -(D - 1), D, -D, D + 1, -(D + 1))
# relative errors of the stand-in for v_rsq_f64.  One Newton step squares the error (x 1.5) and the certificate sees twice that: up to
# about 2^-20.8 it passes (tau = 2^-40) -- 2^-23 is the instruction's documented accuracy --; 2^-20 exercises its refusal.
RELS_TIGHT = (0.0, 2.0 ** -26, -2.0 ** -26, 2.0 ** -23, -2.0 ** -23)
RELS_WIDE = (2.0 ** -21, -2.0 ** -21, 2.0 ** -20, -2.0 ** -20)


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()                   # a no-op when the in-tree library is current
    import ascendpathtracing_amd as pkg
    return pkg


# ---- the vectors -----------------------------------------------------------------------------------------------------------------------
def camera_vectors(n, seed):
    """Random d = cx*a + cy*b + g of the reference camera at 1920 x 1080 (pt_core.h camera_init), a and b uniform in (-0.5, 0.5)."""
    rng = np.random.default_rng(seed)
    a, b = rng.random(n) - 0.5, rng.random(n) - 0.5
    g = np.array([0.0, -0.042612, -1.0]) / np.sqrt(0.042612 ** 2 + 1.0)
    cx0 = 1920 * 0.5135 / 1080
    cy = np.cross([cx0, 0.0, 0.0], g)
    cy = cy / np.linalg.norm(cy) * 0.5135
    return np.ascontiguousarray(np.stack([cx0 * a, cy[1] * b + g[1], cy[2] * b + g[2]], axis=1))


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp; no overflow or underflow in the range used here)."""
    p = a * b
    ca, cb = a * 134217729.0, b * 134217729.0
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma_sq(y, acc):
    """fma(y, y, acc) from float64 operations: y*y = p + e and acc + p = s + t exactly, then one rounding of s + (t + e) (the inner
    sum is far below an ulp of s: wrong only where the exact sum lies within ~2^-50 ulp of a rounding boundary)."""
    p, e = _two_prod(y, y)
    s = acc + p
    bb = s - acc
    t = (acc - (s - bb)) + (p - bb)
    return s + (t + e)


def norm3_sq(d):
    """pt_core.h norm3_sq: x*x, then two FMAs."""
    return _fma_sq(d[:, 2], _fma_sq(d[:, 1], d[:, 0] * d[:, 0]))


def _ulps(x, k):
    """x moved by k float64 ulps (k an integer array; same binade assumed by the callers' tolerance)."""
    return (x.view(np.int64) + np.where(x < 0, -k, k)).view(np.float64)


def midpoint_vectors(n, seed):
    """Camera-range vectors with one component moved so that the REFERENCE quotient d_k / sqrt(n2) (float64, correctly rounded steps) sits
    at a chosen offset from a float32 rounding midpoint: exactly on it, 1 ulp off, D - 1, D, D + 1 ulps off, either side.  Found by
    search: the quotient moves by less than one of its ulps per ulp of d_k, so a neighbour of the first guess hits the target.  ->
    (vectors, share that hit)."""
    rng = np.random.default_rng(seed)
    d = camera_vectors(n, seed + 1)
    k = rng.integers(0, 3, n)
    off = np.array(OFFSETS, dtype=np.int64)[rng.integers(0, len(OFFSETS), n)]
    rows = np.arange(n)
    nrm = np.sqrt(norm3_sq(d))
    q = d[rows, k] / nrm
    # the float32 midpoint next to q (low 29 bits = 2^28), then the offset
    target = ((np.abs(q).view(np.int64) & ~np.int64((1 << 29) - 1)) | np.int64(1 << 28)) + off
    target = np.where(q < 0, -target.view(np.float64), target.view(np.float64))
    # first guess: d_k = t * sqrt(s / (1 - t^2)), s the other components' squares
    s = nrm * nrm - d[rows, k] ** 2
    guess = target * np.sqrt(s / (1.0 - target * target))
    best = guess.copy()
    hit = np.zeros(n, dtype=bool)
    for step in range(-12, 13):
        cand = d.copy()
        cand[rows, k] = _ulps(guess, np.full(n, step, dtype=np.int64))
        qc = cand[rows, k] / np.sqrt(norm3_sq(cand))
        ok = (qc == target) & ~hit
        best[ok] = cand[rows, k][ok]
        hit |= ok
    d[rows, k] = best
    return np.ascontiguousarray(d), float(hit.mean())


def edge_vectors():
    """Zeros, signed zeros, denormals and tiny or huge components, alone and next to ordinary ones."""
    vals = [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1030, 2.0 ** -1000, -2.0 ** -600, 2.0 ** -150, 2.0 ** -127, 2.0 ** -126, 2.0 ** -61,
            2.0 ** -60, -2.0 ** -60, 2.0 ** -59, 1e-30, -1e-12, 0.25, -0.999, 1.0, 3.0, 2.0 ** 59, 2.0 ** 61, 2.0 ** 400, -2.0 ** 600,
            float("inf"), float("nan")]
    g = np.array(np.meshgrid(vals, vals, vals, indexing="ij")).reshape(3, -1).T
    return np.ascontiguousarray(g)


def selftest_host(apt, d3, rel, want_flags=False):
    L = apt._lib.lib()
    res = np.zeros(5, dtype=np.uint64)
    flags = np.zeros(len(d3), dtype=np.uint8) if want_flags else None
    rc = L.apt_selftest_direction_host(d3.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(len(d3)), ctypes.c_double(rel),
                                       res.ctypes.data_as(ctypes.c_void_p), flags.ctypes.data_as(ctypes.c_void_p) if want_flags else None)
    assert rc == 0, L.apt_last_error()
    out = dict(accepted=int(res[0]), rejected=int(res[1]), bad=int(res[2]), ray_rejected=int(res[3]),
               max_cert=float(res[4:5].view(np.float64)[0]))
    return (out, flags) if want_flags else out


# ---- CPU: the accept rule --------------------------------------------------------------------------------------------------------------
def test_the_midpoint_vectors_sit_where_they_claim(apt):
    """The construction itself: the emulated FMA chain is the C library's fma(), and nearly every vector hits its target offset."""
    d, share = midpoint_vectors(20000, seed=5)
    assert share >= 0.9, share
    fma = ctypes.CDLL("libm.so.6").fma
    fma.restype, fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    want = [fma(z, z, fma(y, y, x * x)) for x, y, z in d[:2000].tolist()]
    assert np.array_equal(norm3_sq(d[:2000]), np.array(want))
    # and the low 29 bits of the reference quotients do lie in the nine places
    q = d / np.sqrt(norm3_sq(d))[:, None]
    low = (np.abs(q).view(np.int64) & ((1 << 29) - 1)) - (1 << 28)
    near = np.isin(low, OFFSETS).any(axis=1)
    assert near.mean() >= 0.9, near.mean()


def test_accepted_directions_equal_the_exact_form_on_ten_million_vectors(apt):
    """>= 10^7 vectors: random camera directions; quotients on and around float32 midpoints; zeros, signed zeros, tiny components.  With
    every relative error of the stand-in up to 2^-20, either sign: no accepted component differs from (float)(d_k / sqrt(n2)); with the
    realistic ones, at most 1e-4 of the random rays are sent to the exact path (derived: 3 * 513 / 2^29 = 2.9e-6)."""
    total = 0
    shares = {}
    for chunk in range(4):                                         # 4 x 2.5 M random vectors, each at the five realistic errors
        d = camera_vectors(2_500_000, seed=100 + chunk)
        for rel in RELS_TIGHT:
            r = selftest_host(apt, d, rel)
            print("random", chunk, rel, r)
            assert r["bad"] == 0, (chunk, rel, r)
            assert r["accepted"] + r["rejected"] == len(d)
            shares.setdefault(rel, []).append(r["rejected"] / len(d))
        total += len(d)
        if chunk == 0:
            for rel in RELS_WIDE:                                  # the certificate's turn: sound whatever the instruction returned
                r = selftest_host(apt, d[:500_000], rel)
                print("random, wide", rel, r)
                assert r["bad"] == 0, (rel, r)
                if abs(rel) >= 2.0 ** -20:
                    assert r["accepted"] == 0 and r["ray_rejected"] == 500_000, (rel, r)    # 3 * rel^2 = 3 * 2^-40 > tau
                else:
                    assert r["ray_rejected"] == 0 and r["rejected"] <= 50, (rel, r)
    for rel, s in shares.items():
        assert max(s) <= 1e-4, (rel, s)
        assert min(s) > 0.0, (rel, s)                              # (the window is there: some ray of 2.5 M does fall into it)
    mid, share = midpoint_vectors(400_000, seed=9)
    assert share >= 0.9
    for rel in RELS_TIGHT + RELS_WIDE:
        r, flags = selftest_host(apt, mid, rel, want_flags=True)
        print("midpoints", rel, r)
        assert r["bad"] == 0, (rel, r)
        assert not (flags & (flags >> 3) & 7).any()
    total += len(mid)
    # with an exact reciprocal square root the rule is sharp where it has to be: most of these vectors have a component inside the
    # window and are rejected; the ones D + 1 out are mostly accepted
    r, flags = selftest_host(apt, mid, 0.0, want_flags=True)
    assert 0.5 < r["rejected"] / len(mid) < 0.95, r
    edge = edge_vectors()
    for rel in RELS_TIGHT + RELS_WIDE:
        r, flags = selftest_host(apt, edge, rel, want_flags=True)
        print("edge", rel, r)
        assert r["bad"] == 0, (rel, r)
        # a zero, a denormal or anything below 2^-60 in ANY component refuses the whole ray (signs of zero, float32 denormals)
        small = (np.abs(edge) < 2.0 ** -60).any(axis=1) | ~np.isfinite(edge).all(axis=1)
        assert not (flags[small] & 71).any()
    total += len(edge)
    assert total >= 10_000_000, total


def test_selftest_entries_check_their_arguments(apt):
    L = apt._lib.lib()
    d = camera_vectors(4, seed=1)
    res = np.zeros(5, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.apt_selftest_direction_host(None, ctypes.c_uint64(4), ctypes.c_double(0.0), p(res), None) == 1
    assert L.apt_selftest_direction_host(p(d), ctypes.c_uint64(4), ctypes.c_double(0.0), None, None) == 1
    assert L.apt_selftest_direction_host(p(d), ctypes.c_uint64(4), ctypes.c_double(2.0 ** -19), p(res), None) == 1
    assert L.apt_selftest_direction_host(p(d), ctypes.c_uint64(4), ctypes.c_double(float("nan")), p(res), None) == 1
    assert L.apt_selftest_direction_host(p(d), ctypes.c_uint64(0), ctypes.c_double(0.0), p(res), None) == 0 and not res.any()
    assert L.apt_selftest_chain_states_host(ctypes.c_uint32(0), ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(1), p(res)) == 1
    assert L.apt_selftest_chain_states_host(ctypes.c_uint32(8), ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(1), None) == 1
    assert L.apt_selftest_direction(None, None, ctypes.c_uint64(4), None, None) == 1          # (before any use of the GPU)


# ---- CPU: the generator states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", (8, 64, 200))
def test_states_by_addition_are_the_generators_integers(apt, samples):
    """Every sample of every lane of a frame (48 x 36 pixels), and pixels whose path indices lie above 2^32."""
    L = apt._lib.lib()
    for seed, begin, count in ((0, 0, 48 * 36), (0x9E3779B97F4A7C15, 1, 700), (7, (1 << 33) // samples + 5, 300), (3, (1 << 61) // samples, 64)):
        res = np.zeros(3, dtype=np.uint64)
        assert L.apt_selftest_chain_states_host(ctypes.c_uint32(samples), ctypes.c_uint64(seed), ctypes.c_uint64(begin), ctypes.c_uint64(count),
                                                res.ctypes.data_as(ctypes.c_void_p)) == 0
        checked, differ, single = (int(x) for x in res)
        assert differ == 0, (samples, seed, begin)
        assert checked + single == count * 4 * samples            # every sample of every lane: in a pair, or one at a time
        # numpy's plan: leaves of <= 128 samples; within a leaf, pairs while 16 samples are left of its multiple of 8
        if samples == 8:
            assert checked == 0
        elif samples == 64:
            assert single == 0
        else:
            assert 0 < single < checked


# ---- CPU: the ISA ----------------------------------------------------------------------------------------------------------------------
def _regions(lines):
    """Straight-line regions of a kernel's ISA (cut after every branch), as instruction lists."""
    out, cur = [], []
    for line in lines:
        s = line.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        op = s.split()[0]
        cur.append(op)
        if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
            out.append(cur)
            cur = []
    return out


def _count(ops, prefix):
    return sum(1 for o in ops if o.startswith(prefix))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_headline_kernel_generates_a_pair_in_one_block():
    subprocess.run(["make", "-s", "-C", CSRC, "asm"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(os.path.join(CSRC, "render_kernels.s")).read()
    begin = text.index("\n" + HEADLINE + ":")
    end = text.index(".end_amdhsa_kernel", begin)
    regions = _regions(text[begin:end].split("\n"))
    gen = [r for r in regions if _count(r, "v_rsq_f64")]
    hot_pair = [r for r in gen if _count(r, "v_rsq_f64") == 6 and _count(r, "v_rcp_f64") == 0]
    # sample2's two call sites (the chain's first pair, the loop): the four tent roots and the two directions of a pair in ONE straight
    # line -- a second validity branch would cut it in two --, no float64 reciprocal, the generator's 4 x 4 low multiplies and nothing
    # for the path index
    assert len(hot_pair) == 2, [(_count(r, "v_rsq_f64"), _count(r, "v_rcp_f64")) for r in gen]
    for r in hot_pair:
        assert _count(r, "v_mul_lo_u32") <= 16, _count(r, "v_mul_lo_u32")
        assert _count(r, "v_mad_u64_u32") == 8
        assert _count(r, "v_min3_u32") == 2 and _count(r, "v_lshl_add_u32") + _count(r, "v_add_lshl_u32") == 6     # the six midpoint keys
        assert _count(r, "v_mov_b") == 0 and _count(r, "v_readlane_b32") <= 1
        # 254 VALU up to the pair's validity branch (profiles/raygen_pair_ab.json counts the whole of it: 254 + 12 origins + 12 conversions
        # = 278 against the parent's 305); four instructions of slack, so that a copy or v_mov that creeps back in fails here
        valu = sum(1 for o in r if o.startswith("v_"))
        print("pair ray-generate up to its validity branch:", valu, "VALU")
        assert valu <= 258, valu
    # every other block with float64 roots is a one-ray form (3 roots, hot) or an exact form (its divisions' v_rcp_f64)
    for r in gen:
        if r not in hot_pair:
            assert _count(r, "v_rcp_f64") >= 5 or (_count(r, "v_rsq_f64") == 3 and _count(r, "v_rcp_f64") == 0), \
                (_count(r, "v_rsq_f64"), _count(r, "v_rcp_f64"))
    tail = text[end:end + 4000]
    res = {k: int(v) for k, v in re.findall(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)$", tail, re.M)[:3]}
    assert set(res) == {"NumVgprs", "ScratchSize", "Occupancy"}, res
    assert res["ScratchSize"] == 0 and res["NumVgprs"] <= 128 and res["Occupancy"] >= 4, res


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _selftest_device(apt, d3, want_flags=False):
    import torch
    from ascendpathtracing_amd import render
    d = torch.from_numpy(d3).cuda()
    out = render.selftest_direction(d, flags=want_flags)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
def test_device_accepts_only_what_equals_its_exact_form(apt):
    """v_rsq_f64 itself: on the midpoint vectors (and the edge values, and random camera directions) no accepted component differs from
    the device's sqrt() and '/'; the instruction is accurate enough for the certificate, so that the rejected share of random rays stays
    what the midpoint window alone makes it."""
    from ascendpathtracing_amd import _lib
    _lib.require_gpu()
    mid, share = midpoint_vectors(400_000, seed=9)
    assert share >= 0.9
    r, flags = _selftest_device(apt, mid, want_flags=True)
    print("device, midpoints", r)
    assert r["bad"] == 0 and r["accepted"] + r["rejected"] == len(mid), r
    assert not (flags & (flags >> 3) & 7).any()
    assert r["ray_rejected"] == 0, r                                  # camera-range operands: the certificate never refuses
    assert 0.5 < r["rejected"] / len(mid) < 0.95, r
    # the device and the host (exact reciprocal square root) draw the line at the same components, up to the few ulps between their F_k
    _, host_flags = selftest_host(apt, mid, 0.0, want_flags=True)
    assert (((flags ^ host_flags) & 7) != 0).mean() < 0.05
    r = _selftest_device(apt, edge_vectors())
    print("device, edge", r)
    assert r["bad"] == 0, r
    d = camera_vectors(4_000_000, seed=200)
    r = _selftest_device(apt, d)
    print("device, random", r, "max |certificate| = 2^%.2f" % np.log2(r["max_cert"]))
    assert r["bad"] == 0 and r["ray_rejected"] == 0, r
    assert r["rejected"] / len(d) <= 1e-4, r
    assert r["max_cert"] <= 2.0 ** -40
