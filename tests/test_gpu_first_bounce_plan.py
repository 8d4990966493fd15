"""GPU (run with -m gpu on an MI355X): the two-path frame kernel with its first-bounce plan (csrc/pt_first_plan.h) against the CPU
restatement, bit for bit -- float32 as bits and the 8-bit image, K- and O-mode.  S = 16 is the smallest sample count that takes the
pair path; depth 1 is the bounce that is first and last at once, depth 2 the first bounce followed by the last, depth 3 has a loop
bounce between them.  The pixel range starts and ends mid-column, so waves straddle two columns and the plan's boundaries."""
import numpy as np
import pytest

import first_plan_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).ravel()).cuda()


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.render, pkg.gen_data = render, gen_data
    return pkg


def modes(apt, oracle):
    return ((apt.APT_MODE_KERNEL, oracle.MODE_K), (apt.APT_MODE_ORACLE, oracle.MODE_O))


def check(apt, oracle, sph_h, w, h, depth, mode, omode, begin=0, count=None, seed=3, eps=1e-4):
    count = w * h - begin if count is None else count
    fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(w, h, 16, depth=depth, mode=omode, seed=seed, eps=eps), sph_h, pixel_begin=begin,
                                           pixel_count=count, threads=oracle.max_threads())
    fb, u8 = apt.render.render_frame(apt.make_params(w, h, 16, depth=depth, mode=mode, seed=seed, eps=eps), dev(sph_h), pixel_begin=begin, pixel_count=count)
    torch.cuda.synchronize()
    assert np.array_equal(bits(fb), bits(fb_w)), (w, h, depth, mode, begin, count)
    assert np.array_equal(u8.cpu().numpy(), u8_w), (w, h, depth, mode, begin, count)


def plan_marks_every_rule(w, h, sph_h):
    """The plan of this shape through its CPU twin: every rule (spheres 0, 1, 3, 4, 5, 6, 7) leaves its sphere out for some pixel, so a
    frame that equals the oracle's was rendered with spheres left out, not with an empty plan."""
    L = first_plan_ref.twin()
    rec = first_plan_ref.record(L, w, h, sph_h, eps=1e-4)
    return int(np.bitwise_or.reduce(first_plan_ref.masks(L, rec, w, h, range(w), range(h)).ravel())) == 0xFB


@pytest.mark.parametrize("w,h", [(64, 36), (33, 19)])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_frames_equal_the_oracle(apt, oracle, w, h, depth):
    sph_h = apt.gen_data.gen_spheres()
    assert plan_marks_every_rule(w, h, sph_h)
    for mode, omode in modes(apt, oracle):
        check(apt, oracle, sph_h, w, h, depth, mode, omode)


@pytest.mark.parametrize("w,h", [(64, 36), (33, 19)])
def test_a_range_that_starts_and_ends_mid_column(apt, oracle, w, h):
    """Pixel q is column q / h, row q % h: an odd begin makes every wave's two pixels straddle the rows the plan's row boundaries fall
    between, and at each column's end the two pixels lie in different columns."""
    sph_h = apt.gen_data.gen_spheres()
    begin, count = 3 * h + h // 2 + 1, (w - 7) * h - 5
    for mode, omode in modes(apt, oracle):
        check(apt, oracle, sph_h, w, h, 3, mode, omode, begin=begin, count=count)


def test_tables_the_plan_refuses(apt, oracle):
    """The same launch with tables that are not the room: one coordinate of the reference table moved by one ulp (the general form of the
    intersections) and a random table with the shared-planes pattern (the shared-planes form with an empty plan)."""
    ref = apt.gen_data.gen_spheres().copy()
    near = ref.copy()
    near[8 + 5] = np.nextafter(near[8 + 5], np.float32(1e9))          # cx of sphere 5
    rng = np.random.RandomState(11)
    tab = np.zeros((10, 8), dtype=np.float32)
    r = np.where(rng.rand(8) < 0.3, rng.uniform(2, 30, 8), rng.uniform(200, 1e5, 8))
    tab[0] = (r * r).astype(np.float32)
    tab[1:4] = rng.uniform(-60, 160, size=(3, 8))
    X, Y, Z = (np.float32(v) for v in rng.uniform(0, 100, 3))
    tab[1, [2, 3, 4, 5, 7]] = X
    tab[2, [0, 1, 2, 3]] = Y
    tab[3, [0, 1, 4, 5, 7]] = Z
    tab[7:10] = rng.uniform(0.1, 1.0, size=(3, 8))
    planes = np.zeros(128, dtype=np.float32)
    planes[:80] = tab.ravel()
    for sph_h in (near, planes):
        for mode, omode in modes(apt, oracle):
            check(apt, oracle, sph_h, 64, 36, 3, mode, omode)


FAMILY_SEED, FAMILY_FRAMES = 7, 24


@pytest.fixture(scope="module")
def family_frames():
    """24 members of the test family (tests/first_plan_ref.py) that the plan accepts under the reference's camera -- the render ABI has no
    other for this kernel -- alternately 33 x 19 and 64 x 36, eps going round the family's set; across them every rule marks pixels in
    at least five."""
    L = first_plan_ref.twin()
    found, marks, i = [], {k: 0 for k in first_plan_ref.RULE_BITS}, 0
    while len(found) < FAMILY_FRAMES:
        w, h = ((33, 19), (64, 36))[len(found) % 2]
        eps = first_plan_ref.FAMILY_EPS[len(found) % len(first_plan_ref.FAMILY_EPS)]
        sph, _, _, _ = first_plan_ref.family_case(FAMILY_SEED, i, shape=(w, h), reference_camera=True)
        rec = first_plan_ref.record(L, w, h, sph, eps=eps)
        if rec.any():
            seen = int(np.bitwise_or.reduce(first_plan_ref.masks(L, rec, w, h, range(w), range(h)).ravel()))
            for k in marks:
                marks[k] += (seen >> k) & 1
            found.append((i, sph, eps, w, h))
        i += 1
    assert all(v >= 5 for v in marks.values()), marks
    return found


@pytest.mark.parametrize("n", range(FAMILY_FRAMES))
def test_family_frames_equal_the_oracle(apt, oracle, family_frames, n):
    """The product build at tables nobody rendered before: other rooms, walls at the ends of their radius range, balls that are tiny, huge,
    far away or on the origins, lights of radius 10 .. 1e7, eps up to 1.  Depth 2, S = 16, K- and O-mode, bit for bit."""
    member, sph_h, eps, w, h = family_frames[n]
    for mode, omode in modes(apt, oracle):
        check(apt, oracle, sph_h, w, h, 2, mode, omode, eps=eps, seed=100 + member)


def test_a_captured_launch_replays(apt, oracle):
    """The plan kernel and the frame kernel captured in a graph and replayed, with the table's contents changed behind the unchanged
    pointer between the replays: the plan is made again on every replay."""
    w, h = 64, 36
    ref = apt.gen_data.gen_spheres()
    near = ref.copy()
    near[8 + 5] = np.nextafter(near[8 + 5], np.float32(1e9))
    sph = dev(ref)
    p = apt.make_params(w, h, 16, depth=3, seed=3)
    fb = torch.zeros((3, w * h), device="cuda")
    u8 = torch.zeros((w * h, 3), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # warm-up outside capture: the context's device buffer is made here
        apt.render.render_frame(p, sph, fb=fb, fb_u8=u8)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        apt.render.render_frame(p, sph, fb=fb, fb_u8=u8)
    for table in (ref, near, ref):
        sph.copy_(dev(table))
        fb.zero_(); u8.zero_()
        g.replay()
        torch.cuda.synchronize()
        fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(w, h, 16, depth=3, seed=3), table, threads=oracle.max_threads())
        assert np.array_equal(bits(fb), bits(fb_w)) and np.array_equal(u8.cpu().numpy(), u8_w)


def test_two_streams_on_one_context_with_different_shapes(apt, oracle):
    """One context, two streams: a larger frame on one while the other enqueues more small frames of another shape than the context
    has plan record slots (pt_first_plan.h kFirstPlanSlots = 64), so their plan kernels come round to the slot the large frame's
    record lives in.  A record carries its launch's ticket in every entry and a wave that reads a foreign one skips nothing: every
    frame equals the oracle's whatever the two streams' kernels do to each other."""
    sph_h = apt.gen_data.gen_spheres()
    sph = dev(sph_h)
    (bw, bh), (sw, sh), n_small = (480, 270), (33, 19), 70
    pb, ps = apt.make_params(bw, bh, 16, depth=3, seed=5), apt.make_params(sw, sh, 16, depth=3, seed=6)
    fb_b, u8_b = torch.zeros((3, bw * bh), device="cuda"), torch.zeros((bw * bh, 3), dtype=torch.uint8, device="cuda")
    fb_s = [torch.zeros((3, sw * sh), device="cuda") for _ in range(n_small)]
    u8_s = [torch.zeros((sw * sh, 3), dtype=torch.uint8, device="cuda") for _ in range(n_small)]
    apt.render.render_frame(ps, sph, fb=fb_s[0], fb_u8=u8_s[0])      # the context's device buffer exists before the streams start
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for rounds in range(2):
        with torch.cuda.stream(a):
            apt.render.render_frame(pb, sph, fb=fb_b, fb_u8=u8_b)
        with torch.cuda.stream(b):
            for k in range(n_small):
                apt.render.render_frame(ps, sph, fb=fb_s[k], fb_u8=u8_s[k])
    torch.cuda.synchronize()
    fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(bw, bh, 16, depth=3, seed=5), sph_h, threads=oracle.max_threads())
    assert np.array_equal(bits(fb_b), bits(fb_w)) and np.array_equal(u8_b.cpu().numpy(), u8_w)
    fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(sw, sh, 16, depth=3, seed=6), sph_h, threads=oracle.max_threads())
    for k in range(n_small):
        assert np.array_equal(bits(fb_s[k]), bits(fb_w)) and np.array_equal(u8_s[k].cpu().numpy(), u8_w), k
