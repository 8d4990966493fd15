#!/usr/bin/env python3
"""Adaptive sampling (include/render_mi355x_adaptive.h; include/render_mi355x.h "List passes"): what a list pass, the select, the list
accumulate and the mean cost.  Needs an MI355X (no fallback).

    python profiles/adaptive_cost.py [--reps 5] [--parent-lib PATH] [--out profiles/adaptive_cost.jsonl]

profiles/film_cost.py's method: 1920x1080, depth 8, 64 samples, HIP events around each launch, one warm-up per shape, all shapes
alternated in one process; every line carries all repetitions, their median, minimum and maximum.  The scene is the closed diffuse room
with smallpt's lamp under APT_FLAG_NEE.
  (a) one film pass (pass index 4) on this build and -- with --parent-lib, a librender_mi355x.so built from the parent commit and
      loaded next to this tree's -- on the parent's: the same code object, so a difference beyond the parent's own spread is a finding;
  (b) a list pass over every pixel in order;
  (c) list passes over 50 % and 10 % of the pixels: a random subset (ascending, as a select leaves it) and the room's own selection
      after 4 uniform passes with apt_film_select_default_host's record, and with a threshold that selects about a tenth;
  (d) the select, the list accumulate (of the room's own selection) and the mean, each alone.
For the lists: milliseconds per listed pixel relative to the full pass's milliseconds per pixel.
Nothing here says what bounds these kernels: that takes a counter run of its own."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, DEPTH, SAMPLES, BASE = 1920, 1080, 8, 64, 4
N = W * H


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(here, "adaptive_cost.jsonl"))
    ap.add_argument("--parent-lib", help="librender_mi355x.so of the parent commit: its film pass (a) is timed in the same run")
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    sph = dev(gen_data.with_lamp(gen_data.gen_spheres(), 8, 7))
    mat = dev(np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32))
    p = apt.make_params(W, H, SAMPLES, depth=DEPTH, num_spheres=8, light_index=7, seed=0, flags=apt.APT_FLAG_NEE)

    # the room's own film: BASE uniform passes with moments, and what the select makes of them
    film = render.Film(W, H, moments=True, adaptive=True)
    for _ in range(BASE):
        film.add_pass(p, sph, mat)
    torch.cuda.synchronize()
    render.check_device_status()

    def selection(**fields):
        rec = _lib.film_select_record(BASE, **fields)
        lst, cnt = render.film_select(rec, film.moments, film.extra)
        torch.cuda.synchronize()
        return lst[: int(cnt.cpu()[0])].clone(), rec

    own, own_rec = selection()
    # a threshold whose selection is about a tenth of the image: bisection on the film's own moments (measurement set-up, not a default)
    lo_t, hi_t = 0.0, 4.0
    for _ in range(24):
        mid = 0.5 * (lo_t + hi_t)
        if selection(threshold=mid)[0].numel() > N // 10:
            lo_t = mid
        else:
            hi_t = mid
    tenth, tenth_rec = selection(threshold=hi_t)
    rng = np.random.default_rng(5)
    lists = {"all_in_order": torch.arange(N, dtype=torch.int32, device="cuda"),
             "random_50": dev(np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)),
             "random_10": dev(np.sort(rng.choice(N, N // 10, replace=False)).astype(np.int32)),
             "own_default": own, "own_about_a_tenth": tenth}
    lists = {k: v for k, v in lists.items() if v.numel() > 0}

    scratch = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    plain = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    mean_out = torch.empty((3, N), dtype=torch.float32, device="cuda")
    sel_list = torch.empty(N, dtype=torch.int32, device="cuda")
    sel_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    sel_work = torch.empty(_lib.adaptive_lib().apt_film_select_work_words(N), dtype=torch.int32, device="cuda")
    acc_film, acc_mom, acc_extra = film.buffer.clone(), film.moments.clone(), film.extra.clone()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def parent_pass():
        rc = parent.apt_render_frame_film(ctypes.byref(p), None, ctypes.c_void_p(sph.data_ptr()), ctypes.c_void_p(mat.data_ptr()), None,
                                          ctypes.c_uint64(0), ctypes.c_uint64(N), ctypes.c_void_p(plain.data_ptr()), ctypes.c_uint32(BASE))
        assert rc == 0, rc

    def list_pass(lst):
        return lambda: render.render_frame_film(p, sph, mat, film=scratch.view(-1)[:3 * lst.numel()], pass_index=BASE, pixel_list=lst)

    shapes = {}
    if parent is not None:
        shapes["a_film_pass_parent"] = parent_pass
    shapes["a_film_pass"] = lambda: render.render_frame_film(p, sph, mat, film=plain, pass_index=BASE)
    for name, lst in lists.items():
        shapes["bc_list_pass_" + name] = list_pass(lst)
    shapes["d_select_default"] = lambda: render.film_select(own_rec, film.moments, film.extra, sel_work, sel_list, sel_count)
    shapes["d_select_about_a_tenth"] = lambda: render.film_select(tenth_rec, film.moments, film.extra, sel_work, sel_list, sel_count)
    acc = lists.get("own_about_a_tenth", lists["random_10"])
    shapes["d_accumulate_list"] = lambda: render.film_accumulate_list(scratch.view(-1)[:3 * acc.numel()], acc, acc.numel(), acc_film, acc_mom, acc_extra)
    shapes["d_mean"] = lambda: render.film_mean(film.buffer, BASE, film.extra, mean_out)

    times = {k: [] for k in shapes}
    for name in shapes:                              # warm-up: code objects
        timed(shapes[name])
    render.check_device_status()
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name in shapes:
            times[name].append(round(timed(shapes[name]), 4))
    render.check_device_status()

    rows = []
    for name in shapes:
        t = times[name]
        r = {"shape": name, "frame": f"{W}x{H}", "ms": t, "median_ms": round(statistics.median(t), 4), "min_ms": min(t), "max_ms": max(t)}
        if name.startswith("bc_"):
            r["listed"] = lists[name[len("bc_list_pass_"):]].numel()
            r["listed_fraction"] = round(r["listed"] / N, 4)
        if name == "d_accumulate_list":
            r["listed"] = acc.numel()
        if name[0] in "abc":
            r.update({"depth": DEPTH, "samples": SAMPLES})
        rows.append(r)
    med = {r["shape"]: r["median_ms"] for r in rows}
    full = med["a_film_pass"] / N
    s = {"shape": "summary", "select_default": {"count": own.numel(), "threshold": own_rec.threshold, "floor": own_rec.floor, "min_passes": own_rec.min_passes,
                                                "max_passes": own_rec.max_passes},
         "select_about_a_tenth": {"count": tenth.numel(), "threshold": round(tenth_rec.threshold, 6)},
         "per_listed_pixel_over_per_pixel_of_the_full_pass": {r["shape"]: round(r["median_ms"] / r["listed"] / full, 4) for r in rows if r["shape"].startswith("bc_")}}
    if parent is not None:
        b = times["a_film_pass_parent"]
        s.update({"film_pass_minus_parent_ms": round(med["a_film_pass"] - med["a_film_pass_parent"], 4), "parent_spread_ms": round(max(b) - min(b), 4)})
    rows.append(s)
    meta = {"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps, "parent_lib": bool(parent),
            "scene": "closed diffuse room, smallpt's lamp, APT_FLAG_NEE", "base_passes": BASE}
    with open(args.out, "w") as f:
        for r in rows + [meta]:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
