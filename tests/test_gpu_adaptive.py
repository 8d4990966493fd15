"""Adaptive sampling on the GPU (libadaptive_mi355x.so, include/render_mi355x_adaptive.h): the device entries of select,
accumulate-list and mean against their CPU twins and the restatement (tests/adaptive_ref.py) on the CPU test's sizes and predicates
-- the count, the list in ascending order and the list words beyond the count untouched included --, and a 48 x 32 film of the lamp room
end to end through render.Film: 2 uniform passes and 3 adaptive rounds, with the film, the moments, the extra counts, each round's
list and the resolved bytes bit for bit the restatement's."""
import numpy as np
import pytest

import adaptive_ref as ar
import film_ref as fr
from gpu_harness import apt, assert_bits_equal, dev, oracle_params, scene  # noqa: F401

F, U32 = np.float32, np.uint32
FILL = 0x5EADBEEF                                  # (an int32 tensor's fill: below 2^31)


def _u32(t):
    return t.cpu().numpy().view(U32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("n", ar.SIZES)
def test_device_select_equals_the_twin(apt, n, kind):
    import torch
    _, mom, extra = ar.synthetic(n, kind)
    L = apt._lib.adaptive_lib()
    words = L.apt_film_select_work_words(n)
    for rec in [ar.REC] + ([dict(ar.REC, floor=0.0)] if kind == "floor" else []):
        want = ar.select(mom, extra, **rec)
        rc, twin, count, untouched = ar.select_host(apt, mom, extra, ar.record(apt, **rec))
        assert rc == 0 and untouched and np.array_equal(twin, want)
        d_list = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
        d_work = torch.full((words + 4,), FILL, dtype=torch.int32, device="cuda")
        d_count = torch.full((1,), FILL, dtype=torch.int32, device="cuda")
        got_list, got_count = apt.render.film_select(ar.record(apt, **rec), dev(mom), dev(extra.view(np.int32)), d_work, d_list, d_count)
        torch.cuda.synchronize()
        c = int(_u32(got_count)[0])
        assert c == want.size
        lst = _u32(got_list)
        assert np.array_equal(lst[:c], want) and (lst[c:] == FILL).all()
        assert (_u32(d_work)[words:] == FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "nan"])
@pytest.mark.parametrize("n", ar.SIZES)
def test_device_accumulate_list_and_mean_equal_the_twins(apt, n, kind):
    import torch
    film, mom, extra = ar.synthetic(n, kind)
    lst = ar.select(mom, extra, **ar.REC)
    if lst.size >= 3:                                                 # entries beyond the image among them: skipped
        lst = lst.copy()
        lst[lst.size // 2], lst[-1] = n, 0xFFFFFFFF
    rng = np.random.default_rng(n)
    planes = (rng.random((3, lst.size)) * 3).astype(F)
    if kind == "nan" and lst.size:
        planes[1, 0] = np.nan
    rc, f, m, e, intact = ar.accumulate_list_host(apt, planes, lst, film, mom, extra)
    assert rc == 0 and intact
    for g, w in zip((f, m, e), ar.accumulate_list(planes, lst, film, mom, extra)):
        ar.assert_same(g, w)
    guard = 5
    d_planes = torch.cat([dev(planes.ravel()), torch.full((guard,), -7.0, device="cuda")])
    d_f, d_m, d_e = dev(film), dev(mom), dev(extra.view(np.int32))
    apt.render.film_accumulate_list(d_planes, dev(np.concatenate([lst, [0]]).astype(U32).view(np.int32)), lst.size, d_f, d_m, d_e)
    torch.cuda.synchronize()
    assert_bits_equal(d_f.cpu().numpy(), f)
    assert_bits_equal(d_m.cpu().numpy(), m)
    assert np.array_equal(_u32(d_e), e)
    for ex in (None, d_e):
        out = apt.render.film_mean(d_f, ar.REC["base"], ex)
        torch.cuda.synchronize()
        rc, twin = ar.mean_host(apt, f, ar.REC["base"], None if ex is None else e)
        assert rc == 0
        assert_bits_equal(out.cpu().numpy(), twin)
        assert_bits_equal(twin, ar.mean(f, ar.REC["base"], None if ex is None else e))


@pytest.mark.gpu
def test_device_refusals_write_nothing(apt):
    import torch
    n = 70
    _, mom, extra = ar.synthetic(n, "all")
    d_list = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    d_count = torch.full((1,), FILL, dtype=torch.int32, device="cuda")
    bad = ar.record(apt, **ar.REC)
    bad.min_passes = 1
    with pytest.raises(apt.AptError, match="min_passes"):
        apt.render.film_select(bad, dev(mom), dev(extra.view(np.int32)), None, d_list, d_count)
    bad = ar.record(apt, **ar.REC)
    bad.struct_size = 20
    with pytest.raises(apt.AptError, match="struct_size"):
        apt.render.film_select(bad, dev(mom), dev(extra.view(np.int32)), None, d_list, d_count)
    with pytest.raises(apt.AptError, match="base_passes"):
        apt.render.film_mean(dev(np.ones((3, n), dtype=F)), 1)
    torch.cuda.synchronize()
    assert (_u32(d_list) == FILL).all() and (_u32(d_count) == FILL).all()


# ---- end to end through Film ------------------------------------------------------------------------------------------------------------------
W, H, S, DEPTH, BASE, ROUNDS = 48, 32, 3, 4, 2, 3
SELECT = dict(min_passes=2, max_passes=5, threshold=0.125, floor=0.0625)


@pytest.mark.gpu
def test_film_adaptive_rounds_equal_the_restatement(apt):
    """diff8-lamp with NEE: 2 uniform passes, then 3 rounds whose pass indices are 2, 3, 4.  Every round's list is the restatement's
    select of the restatement's moments; the pass it renders is the whole pass of that index gathered at the list."""
    import torch
    sc = scene(apt, "diff8-lamp")
    p = sc.params(W, H, S, DEPTH, mode="nee", seed=7)
    q = oracle_params(p)
    n = W * H
    passes = [fr.render_pass(q, sc.sph, sc.mat, pass_index=k)[0] for k in range(BASE + ROUNDS)]
    film, mom, extra = fr.accumulate(passes[:BASE]), ar.moments_of(passes[:BASE]), np.zeros(n, dtype=U32)

    f = apt.render.Film(W, H, moments=True, adaptive=True)
    for _ in range(BASE):
        f.add_pass(p, sc.d_sph, sc.d_mat)
    torch.cuda.synchronize()
    assert_bits_equal(f.buffer.cpu().numpy(), film)
    assert_bits_equal(f.moments.cpu().numpy(), mom)
    plain_u8 = f.resolve(exposure=1.5).cpu().numpy()                              # no round yet: the resolve divides by passes
    assert np.array_equal(plain_u8, fr.resolve(film, BASE, 1.5, fr.TONEMAP_CLIP, 0.0, apt.gen_data.film_curve("srgb"))[1])

    counts = []
    for r in range(ROUNDS):
        lst = ar.select(mom, extra, base=BASE, **SELECT)
        got = f.add_adaptive_pass(p, sc.d_sph, sc.d_mat, **SELECT)
        torch.cuda.synchronize()
        apt.render.check_device_status()
        assert got == lst.size and f.rounds == r + 1 and f.passes == BASE
        assert np.array_equal(_u32(f.pixel_list)[:got], lst)
        film, mom, extra = ar.accumulate_list(ar.list_pass(passes[BASE + r], lst), lst, film, mom, extra)
        assert_bits_equal(f.buffer.cpu().numpy(), film)
        assert_bits_equal(f.moments.cpu().numpy(), mom)
        assert np.array_equal(_u32(f.extra), extra)
        counts.append(got)
    # the rounds are worth the name: every one selected something, none everything, and some pixels were in all three
    assert all(0 < c < n for c in counts) and extra.max() == ROUNDS and np.unique(extra).size == ROUNDS + 1, counts

    mean = ar.mean(film, BASE, extra)
    assert_bits_equal(f.mean().cpu().numpy(), mean)
    table = apt.gen_data.film_curve("srgb")
    for kw, tm, iw2 in ((dict(exposure=1.5), fr.TONEMAP_CLIP, 0.0), (dict(exposure=2.0, tonemap="reinhard", white=4.0), fr.TONEMAP_REINHARD, 1.0 / 16.0)):
        u8, out = f.resolve(want_float=True, **kw)
        torch.cuda.synchronize()
        want_out, want_u8 = fr.resolve(mean, 1, kw["exposure"], tm, iw2, table)
        assert_bits_equal(out.cpu().numpy(), want_out)
        assert np.array_equal(u8.cpu().numpy(), want_u8)

    # the three refusals
    with pytest.raises(apt.AptError, match="adaptive rounds"):
        f.add_pass(p, sc.d_sph, sc.d_mat)
    with pytest.raises(apt.AptError, match="extra adaptive passes"):
        f.denoise(p, sc.d_sph)
    with pytest.raises(apt.AptError, match="moments=True"):
        apt.render.Film(W, H, adaptive=True)
    # reset() forgets the rounds: the film is a new one
    f.reset()
    assert f.rounds == 0 and f.passes == 0 and not _u32(f.extra).any()
    f.add_pass(p, sc.d_sph, sc.d_mat)
    with pytest.raises(apt.AptError, match="at least 2"):
        f.add_adaptive_pass(p, sc.d_sph, sc.d_mat)
    torch.cuda.synchronize()
    assert_bits_equal(f.buffer.cpu().numpy(), passes[0])


@pytest.mark.gpu
def test_a_round_that_selects_nothing_advances_and_a_plain_film_is_unchanged(apt):
    import torch
    sc = scene(apt, "diff8-lamp")
    p = sc.params(W, H, S, DEPTH, mode="nee", seed=7)
    f = apt.render.Film(W, H, moments=True, adaptive=True)
    g = apt.render.Film(W, H, moments=True)
    for _ in range(2):
        f.add_pass(p, sc.d_sph, sc.d_mat)
        g.add_pass(p, sc.d_sph, sc.d_mat)
    before = f.buffer.clone()
    assert f.add_adaptive_pass(p, sc.d_sph, sc.d_mat, min_passes=2, max_passes=2) == 0 and f.rounds == 1     # every pixel has max_passes
    torch.cuda.synchronize()
    assert torch.equal(f.buffer.view(torch.int32), before.view(torch.int32)) and not _u32(f.extra).any()
    assert_bits_equal(f.mean().cpu().numpy(), g.mean().cpu().numpy())            # film_mean with extra all zero: the plain mean
    assert np.array_equal(f.resolve().cpu().numpy(), g.resolve().cpu().numpy())
    with pytest.raises(apt.AptError, match="adaptive=True"):
        g.add_adaptive_pass(p, sc.d_sph, sc.d_mat)
    assert g.extra is None and g.rounds == 0
