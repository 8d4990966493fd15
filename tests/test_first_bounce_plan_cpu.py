"""CPU-only: the first-bounce plan of the two-path frame kernel (csrc/pt_first_plan.h) through its CPU twin, libfirstplan_mi355x.so.

For every pixel the plan marks, camera rays over the pixel's whole jitter footprint (corners and edges included) are intersected with
all eight spheres in float32, in the kernel's operation order (b = (px + py) + pz, c = ((qx + qy) + qz) - r2, disc = b*b - c, the
correctly rounded square root, t0 = b - q, t1 = b + q, a root counts when it is > eps): no marked sphere may hold a key <= the
winner's.  A perturbed camera, a permuted table and a camera whose origins lie outside the room must yield a record that skips
nothing, and the plan must not be vacuous.

The rays are restated, not reproduced: origin and direction are made in float64 from the camera's definition and rounded once, without
the kernel's fast sequences, so a ray here can differ from the kernel's in its last float32 bit.  The rules' margins (pt_first_plan.h)
are many orders of magnitude wider than that; the frames themselves are compared bit for bit by tests/test_gpu_first_bounce_plan.py."""
import numpy as np
import pytest

import first_plan_ref
from first_plan_ref import RULE_BITS, camera, first_bounce_keys, jitters, masks, record


@pytest.fixture(scope="module")
def twin():
    return first_plan_ref.twin()


@pytest.fixture(scope="module")
def table():
    return first_plan_ref.reference_table()


def check_shape(L, sph, w, h, cols, rows, seed):
    rec = record(L, w, h, sph)
    cam = camera(L, w, h)
    m = masks(L, rec, w, h, cols, rows)
    fx, fy = jitters(np.random.default_rng(seed), 256)
    cc, rr = np.meshgrid(cols, rows, indexing="ij")
    pc, pr, flat = cc.ravel().astype(np.float64), rr.ravel().astype(np.float64), m.ravel()
    for at in range(0, flat.size, 512):                 # (in chunks of pixels: the arrays stay small)
        part = slice(at, at + 512)
        keys = first_bounce_keys(cam, w, h, sph, pc[part], pr[part], fx, fy)
        win = keys.min(axis=-1)
        assert np.isfinite(win).all()                   # a camera ray of the room always hits something
        for k in RULE_BITS:
            marked = ((flat[part] >> k) & 1).astype(bool)
            if marked.any():
                assert (keys[marked, :, k] > win[marked]).all(), f"{w}x{h}: a marked sphere {k} holds a key <= the winner's"
    assert not ((flat >> 2) & 1).any()
    return m


@pytest.mark.parametrize("w,h", [(64, 36), (96, 54), (33, 19)])
def test_no_marked_sphere_wins_small_frames(twin, table, w, h):
    m = check_shape(twin, table, w, h, np.arange(w), np.arange(h), seed=w)
    if (w, h) == (96, 54):                              # not vacuous: every rule marks a pixel and leaves one
        for k in RULE_BITS:
            bit = (m >> k) & 1
            assert bit.any() and not bit.all(), f"rule of sphere {k} is vacuous at 96x54"


def test_no_marked_sphere_wins_c2_sample(twin, table):
    w, h = 1920, 1080
    rec = record(twin, w, h, table)
    edges_c = [0, 1, w - 2, w - 1, w // 2 - 1, w // 2] + [int(v) + s for v in (rec[0], rec[1], rec[5], w - rec[4], rec[9], w - rec[10]) for s in (-1, 0)]
    edges_r = [0, 1, h - 2, h - 1, h // 2 - 1, h // 2] + [int(v) + s for v in (rec[2], rec[3], rec[7], h - rec[6], rec[11], h - rec[12], rec[13]) for s in (-1, 0)]
    cols = np.unique(np.clip(np.concatenate([np.arange(0, w, 97), edges_c]), 0, w - 1))
    rows = np.unique(np.clip(np.concatenate([np.arange(0, h, 61), edges_r]), 0, h - 1))
    m = check_shape(twin, table, w, h, cols, rows, seed=2)
    assert all(((m >> k) & 1).any() for k in RULE_BITS)


def test_broken_premises_skip_nothing(twin, table):
    w, h = 96, 54
    assert record(twin, w, h, table).any()
    cam = camera(twin, w, h)
    tilted = cam.copy(); tilted[9] = 1e-3               # cy[0] != 0: not the reference camera frame
    assert not record(twin, w, h, table, tilted).any()
    rolled = cam.copy(); rolled[7] = 1e-6               # cx[1] != 0
    assert not record(twin, w, h, table, rolled).any()
    swapped = table.copy()                              # spheres 0 and 6 exchanged: not the room any more
    for row in range(10):
        swapped[row * 8 + 0], swapped[row * 8 + 6] = table[row * 8 + 6], table[row * 8 + 0]
    assert not record(twin, w, h, swapped).any()
    outside = cam.copy(); outside[2] = 400.0            # the origins pos + 140 d lie in front of the room
    assert not record(twin, w, h, table, outside).any()
    assert not record(twin, w, h, table, eps=0.0).any() and not record(twin, w, h, table, eps=2.0).any()
    all_zero = np.zeros(16, dtype=np.int32)             # the record a context's buffer holds before any plan kernel ran
    assert not masks(twin, all_zero, w, h, np.arange(w), np.arange(h)).any()
