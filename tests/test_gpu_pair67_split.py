"""From its second bounce on, a wave of the two-path bounce decides per sphere of pair (6,7), and with the ray's direction, what it
solves (pt_trace.h sphere_reachable_mask, intersect_ns8_v2<.., SKIP> bit 7; pt_trace2.h kPairSkip): nothing, the light alone, the
ball alone, or the full stage.  The frame must not change: framebuffer (float32 as bits) and 8-bit image of the fused frame against the
oracle, in K- and O-mode, at 48x32, 16 samples -- the smallest count that takes the two-path loop -- and depth 1, 2, 3 and 8 (the bounce
that is first and last, first + last, first + one ping-pong step + last, and the headline's loop), on five scene tables
(tests/pair67_ref.py):

  ref         the reference scene
  ball_front  the ball moved in front of the camera, into the middle of the view: the waves of the middle reach it
  ball_big    the same with the ball grown so that EVERY wave reaches it at the first two bounces (a ball of its own size cannot cover
              the camera rays' origins)
  light_r1    the light's radius 1: it cannot be hit anywhere
  both_away   ball and light moved far outside the room: no wave can hit either

Which arm a wave takes is invisible in the product build (its statistics block counts segments and exact re-runs; TraceCounter reads the
same block), and the counting build is a profiling variant that a test would have to compile.  So the arms are asserted on the CPU: the
bounce restated in float32 with the oracle's operation order (checked against the oracle's colours, bit for bit), the kernel's predicate on
the restated (b, c, disc) of spheres 6 and 7, the paths grouped as the kernel's waves hold them."""
import numpy as np
import pytest

import pair67_ref as pr

K, O = 0, 1
DEPTHS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()                   # a no-op when the in-tree library is current
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.render, pkg.gen_data = render, gen_data
    return pkg


_WANT = {}


def _oracle_frame(oracle, name, depth, mode):
    key = (name, depth, mode)
    if key not in _WANT:
        fb, u8, _, _ = oracle.render_frame(oracle.make_params(pr.W, pr.H, pr.S, depth=depth, mode=mode, seed=pr.SEED), pr.scene(oracle, name),
                                           threads=oracle.max_threads())
        fb.setflags(write=False)
        u8.setflags(write=False)
        _WANT[key] = (fb, u8)
    return _WANT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", pr.SCENES)
def test_fused_frame_equals_the_oracle(apt, oracle, name, depth, mode):
    import torch
    fb_w, u8_w = _oracle_frame(oracle, name, depth, mode)
    fb, u8 = apt.render.render_frame(apt.make_params(pr.W, pr.H, pr.S, depth=depth, mode=mode, seed=pr.SEED),
                                     torch.from_numpy(pr.scene(oracle, name)).cuda())
    torch.cuda.synchronize()
    ok, where = pr.same(fb.cpu().numpy(), fb_w)
    assert ok, (name, depth, mode, where)
    assert np.array_equal(u8.cpu().numpy(), u8_w), (name, depth, mode)


@pytest.mark.gpu
def test_exact_reruns_stay_rare(apt):
    """The level tests/test_gpu_parity.py test_fast_path_is_rarely_left pins, for the two-path kernel: a one-sphere stage that read a
    v_rsq_f32 result too early would show here and nowhere else (the exact form of a bounce is bit-exact)."""
    import torch
    sph = torch.from_numpy(apt.gen_data.gen_spheres()).cuda()
    with apt.render.TraceCounter() as tc:
        apt.render.render_frame(apt.make_params(480, 270, 16, depth=8, seed=0), sph)
    waves = 480 * 270 * 4 * 16 // 64
    reruns = int(tc.buf[3].item())
    print("exact re-runs:", reruns, "of", waves, "waves")
    assert tc.value == 480 * 270 * 4 * 16 * 8
    assert reruns <= waves * 4 // 1000


# ---- which arms the scenes reach (CPU) ---------------------------------------------------------------------------------------------

ARMS = ("nothing", "light alone", "ball alone", "full stage")


def _arm_counts(oracle, name, bounces, half):
    """-> how many (wave, bounce) sites of path half `half` take each arm of the per-sphere form, over the bounce indices `bounces`"""
    u6, u7 = pr.arms(oracle, name)
    u6, u7 = u6[list(bounces)][:, half::2], u7[list(bounces)][:, half::2]
    return np.array([(u6 & u7).sum(), (u6 & ~u7).sum(), (~u6 & u7).sum(), (~u6 & ~u7).sum()])


@pytest.mark.parametrize("depth", (2, 3, 8))
def test_the_scenes_run_every_arm(oracle, depth):
    """Path A takes the per-sphere form at bounces 2 .. depth, path B at 2 .. depth - 1 (its last bounce has no test)."""
    for half, bounces in ((0, range(1, depth)), (1, range(1, depth - 1))):
        if len(bounces) == 0:
            continue
        total = np.zeros(4, dtype=np.int64)
        for name in pr.SCENES:
            n = _arm_counts(oracle, name, bounces, half)
            print("depth", depth, "path", "AB"[half], name, dict(zip(ARMS, n.tolist())))
            total += n
        assert (total > 0).all(), (depth, half, total)
    # the last bounce is a form of its own (no shading step): path A's must see every arm there as well
    last = sum(_arm_counts(oracle, name, (depth - 1,), 0) for name in pr.SCENES)
    assert (last > 0).all(), (depth, last)


def test_what_each_scene_is_for(oracle):
    u6, u7 = pr.arms(oracle, "ref")
    for n in range(4):                                           # every arm, within one frame of the reference scene
        assert _arm_counts(oracle, "ref", range(1, 8), 0)[n] > 0 and _arm_counts(oracle, "ref", range(1, 7), 1)[n] > 0
    u6, _ = pr.arms(oracle, "ball_front")
    assert (~u6[0]).any() and u6[0].any()                        # the middle of the view reaches the ball, the rim does not
    u6, _ = pr.arms(oracle, "ball_big")
    assert not u6[0].any() and not u6[1].any()                   # every wave reaches the ball at its first two bounces
    u6, u7 = pr.arms(oracle, "light_r1")
    assert u7.all() and (~u6).any()                              # the light is out of reach everywhere: nothing, or the ball alone
    u6, u7 = pr.arms(oracle, "both_away")
    assert u6.all() and u7.all()


def test_first_bounce_takes_both_arms_of_the_pair_test(oracle):
    """The first bounce keeps the pair's two-instruction test (both discriminants negative or NaN in all 64 lanes)."""
    seen = np.zeros(2, dtype=bool)
    for name in pr.SCENES:
        _, _, disc = pr.trace(oracle, name)
        miss = pr.wave_groups(~((disc[:1, 6] >= 0) | (disc[:1, 7] >= 0))).all(axis=2)
        seen |= np.array([miss.any(), (~miss).any()])
    assert seen.all()
