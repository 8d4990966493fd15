"""CPU-only: the deep end of the pairwise-sum plans (ascendpathtracing_amd/csrc/pt_leaf.h), held to NumPy itself.

  * tests/plan_ref.py's plans, written from numpy's rule, have the shapes the GPU tests rely on: stack depths 3 .. 7, 64 leaves at the
    contract's limit of 7688 samples, 44 leaves at the camera's limit of 4199;
  * the oracle's decode_color IS np.mean at those counts (the goldens pin it up to 300 samples only);
  * every input of tests/test_gpu_deep_plans.py is sensitive to the summation order: the frame of numpy's tree equals the reference
    frame, and two wrong orders over the same samples give other frames.  Only then does a bitwise comparison of a kernel's frame see
    the order in which the kernel summed, and not merely its samples."""
import numpy as np
import pytest

import plan_ref as pr

F = np.float32


@pytest.fixture(scope="module")
def gen_data():
    import __graft_entry__ as g
    g.build()
    from ascendpathtracing_amd import gen_data as gd
    return gd


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the plans -------------------------------------------------------------------------------------------------------------------------
def test_plans_have_the_shapes_the_deep_tests_rely_on():
    assert pr.plan(257) == [(128, 0), (64, 0), (65, 2)]
    assert pr.plan(136) == [(64, 0), (72, 1)] and pr.plan(128) == [(128, 0)] and pr.plan(7) == [(7, 0)]
    want = {257: dict(leaves=3, maxleaf=128, ncomb=2, depth=3, tails=[65]),
            521: dict(leaves=5, maxleaf=128, ncomb=3, depth=4, tails=[73]),
            1025: dict(leaves=9, maxleaf=128, ncomb=4, depth=5, tails=[65]),
            4096: dict(leaves=32, maxleaf=128, ncomb=5, depth=6, tails=[]),
            4199: dict(leaves=44, maxleaf=128, ncomb=6, depth=7, tails=[79]),
            7688: dict(leaves=64, maxleaf=128, ncomb=6, depth=7, tails=[])}
    assert tuple(want) == pr.DEEP
    for s, w in want.items():
        assert pr.stats(s) == w, s
    assert pr.plan(4096) == [(128, c) for c in [0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0, 4] + [0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0, 5]]
    assert pr.stats(4200)["leaves"] == 45                      # the first count past the camera's 44 leaves
    assert pr.stats(256) == dict(leaves=2, maxleaf=128, ncomb=1, depth=2, tails=[])


def test_no_plan_of_the_contract_is_deeper_than_seven():
    """Over every count the contract admits: at most 64 leaves, stack depth at most 7 (of the kernels' 8 entries); the depths 4 .. 7
    first appear at 489, 969, 1929 and 3849 samples."""
    first, leaves = {}, 0
    for s in range(1, 7689):
        st = pr.stats(s)
        first.setdefault(st["depth"], s)
        leaves = max(leaves, st["leaves"])
    assert max(first) == 7 and leaves == 64
    assert [first[d] for d in (4, 5, 6, 7)] == [489, 969, 1929, 3849]


# ---- the oracle's decode_color is np.mean ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", pr.DEEP)
def test_oracle_decode_color_is_numpy_mean_bit_for_bit(oracle, s):
    """np.mean of each sub-pixel's contiguous float32 run (numpy's own pairwise sum), then the float64 steps of decode_color."""
    w = h = 3
    col = pr.mixed_colors(w * h, s, seed=1000 + s)
    runs = col.reshape(3, w * h, 4, s)
    means = np.empty((3, w * h, 4), dtype=F)
    for c in range(3):
        for q in range(w * h):
            for sub in range(4):
                run = runs[c, q, sub]
                assert run.flags.c_contiguous and run.dtype == F
                means[c, q, sub] = np.mean(run)
    assert means.dtype == F
    acc = np.zeros((3, w * h))
    for sub in range(4):
        acc = acc + means[:, :, sub].astype(np.float64)
    pre_w = np.ascontiguousarray((acc / 4).T)
    pre, fb, u8 = oracle.decode_color(col, w, h, s)
    assert np.array_equal(pre.view(np.uint64), pre_w.view(np.uint64))
    cl = np.clip(pre_w, 0, 1)
    assert np.array_equal(_bits(fb), _bits(cl.T.astype(F))) and np.array_equal(u8, (cl * 255).astype(np.uint8))
    assert 0 < (pre_w > 1).sum() < pre_w.size                  # some values clipped, some not
    # and plan_ref's tree is the same sum
    pre_t, fb_t, u8_t = pr.frames(col, w * h, s)["tree"]
    assert np.array_equal(pre_t.view(np.uint64), pre_w.view(np.uint64)) and np.array_equal(_bits(fb_t), _bits(fb)) and np.array_equal(u8_t, u8)


# ---- sensitivity of the GPU tests' inputs ---------------------------------------------------------------------------------------------
def _check(colours, npix, s, fb_ref, u8_ref):
    """The tree frame is the reference frame; the mutants differ (pr.check_sensitive's conditions)."""
    if pr.stats(s)["leaves"] == 2:
        # two leaves: one addition, nothing to reorder -- both mutants ARE the tree (256 = 128 + 128 is run for its launch, see the GPU test)
        fr = pr.frames(colours, npix, s)
        assert pr.differing(fr["left"][1], fr["tree"][1]) == 0 == pr.differing(fr["blocks"][1], fr["tree"][1])
        assert 3 * pr.saturated(fr["tree"][1]) <= fr["tree"][1].size
    else:
        fr, (d1, d2, sat) = pr.check_sensitive(colours, npix, s)
        print("samples %d: %d / %d of %d values differ for the two mutants, %d at 0 or 1" % (s, d1, d2, fr["tree"][1].size, sat))
    _, fb, u8 = fr["tree"]
    assert np.array_equal(_bits(fb), _bits(fb_ref)) and np.array_equal(u8, u8_ref)


MIRROR_CASES = pr.mirror_cases()


def test_the_mirror_cases_cover_what_the_issue_names():
    cases = set(MIRROR_CASES)
    assert len(cases) == len(MIRROR_CASES)
    for s in pr.DEEP:
        for m in (pr.K, pr.O):
            assert {("ref", m, f, s) for f in (0, pr.RR, pr.RETIRE, pr.RETIRE | pr.RR)} <= cases
        assert any(c[0] == "tiles" and c[3] == s and c[2] == pr.RETIRE for c in cases)
    assert any(c[0] == "tiles" and c[3] == 256 and c[2] == pr.RETIRE for c in cases)
    for s in (257, 1025, 7688):
        assert any(c[0] == "grid" and c[3] == s and c[2] == 0 for c in cases) and any(c[0] == "grid" and c[3] == s and c[2] == pr.RETIRE | pr.RR for c in cases)


@pytest.mark.parametrize("scene,mode,flags,s", MIRROR_CASES, ids=["%s-%s-f%d-s%d" % (c[0], "KO"[c[1]], c[2], c[3]) for c in MIRROR_CASES])
def test_mirror_inputs_are_sensitive_to_the_summation_order(oracle, scene, mode, flags, s):
    sph, _ = pr.mirror_scene(oracle, scene)
    p = pr.mirror_params(oracle, scene, mode, flags, s)
    col, _ = oracle.render_paths(p, oracle.gen_rays_counter(p), sph, threads=oracle.max_threads())
    fb_w, u8_w, _, _ = oracle.render_frame(p, sph, threads=oracle.max_threads())
    _check(col, pr.W * pr.H, s, fb_w, u8_w)


@pytest.mark.parametrize("s", pr.DEEP)
def test_decode_inputs_are_sensitive_to_the_summation_order(oracle, s):
    """The colours the device decode kernels are given (12 pixels)."""
    col = pr.decode_colors(s)
    _, fb_w, u8_w = oracle.decode_color(col, pr.W, pr.H, s)
    _check(col, pr.W * pr.H, s, fb_w, u8_w)


@pytest.mark.parametrize("s", pr.MT_SAMPLES)
def test_mt_inputs_are_sensitive_to_the_summation_order(oracle, s):
    col = pr.mt_colours(oracle, s)
    _, fb_w, u8_w = oracle.decode_color(col, pr.MT_W, pr.MT_H, s)
    _check(col, pr.MT_W * pr.MT_H, s, fb_w, u8_w)


@pytest.mark.parametrize("s", pr.MAT_SAMPLES)
@pytest.mark.parametrize("name,mode", pr.MAT_CASES)
def test_material_inputs_are_sensitive_to_the_summation_order(oracle, gen_data, name, mode, s):
    col = pr.mat_colours(oracle, gen_data, name, mode, s)
    _, fb_w, u8_w = oracle.decode_color(col, pr.W, pr.H, s)
    _check(col, pr.W * pr.H, s, fb_w, u8_w)


def test_camera_input_is_sensitive_to_the_summation_order(oracle, gen_data):
    assert pr.stats(pr.CAMERA_SAMPLES)["leaves"] == 44
    col = pr.mat_colours(oracle, gen_data, "demo9lamp", "table", pr.CAMERA_SAMPLES, cam=pr.lens_camera(gen_data))
    _, fb_w, u8_w = oracle.decode_color(col, pr.W, pr.H, pr.CAMERA_SAMPLES)
    _check(col, pr.W * pr.H, pr.CAMERA_SAMPLES, fb_w, u8_w)
