"""GPU (run with -m gpu on an MI355X): what the first-bounce plan (csrc/pt_first_plan.h) does ON THE DEVICE, observed through a counting
build of the library (-DAPT_COUNT_FIRST_PLAN, csrc/pt_kernels.h: the layout of its counts) -- the plan kernel in it is the product's own
object.  Frames that equal the oracle's say nothing about a plan that is never taken; here, for every launch,

  * the record the frame kernel READ equals the CPU twin's (apt_first_plan_host) in all 14 entries, exactly: the plan kernel evaluates the
    same float64 text under -ffp-contract=off, so a difference is a finding about first_plan.hip's build, not a tolerance;
  * every wave took the record (all tickets matched): taken == waves == ceil(pixel_count / 2);
  * for every sphere k the number of waves that left it out equals the twin's prediction, the sum over the waves of bit k of
    mask(q0) & mask(q1).  q0 = begin + 2 i and q1 = q0 + 1 are wave i's pixels (pixel q is column q / h, row q % h); a second pixel past
    the range is read as the launch's FIRST pixel, q1 = begin (pt_frame.h frame_lane: q = pixel_begin + (valid ? pl : 0)), which is what
    happens in the last wave of a range with an odd pixel count;
  * the counting build's frames equal the oracle's bit for bit, the float32 plane and the 8-bit image.

All launches run in ONE child process (a second copy of the library in one process would register its kernels twice) under one timeout;
the child writes its counters and frames to a file and prints one JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import first_plan_ref as fpr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = fpr.ROOT
B = 448                      # pt_kernels.h, APT_COUNT_FIRST_PLAN
S = 16
FAMILY_SEED = 7

CHILD = r'''
import json, sys
import numpy as np, torch
root, src, dst = sys.argv[1:4]
sys.path.insert(0, root)
import ascendpathtracing_amd as apt
from ascendpathtracing_amd import render
lib = apt._lib.lib()
z = np.load(src)
cases = json.loads(str(z["cases"]))
counter = torch.zeros(512, dtype=torch.int64, device="cuda")
assert lib.apt_set_trace_counter(counter.data_ptr()) == 0
out = {}
for n, c in enumerate(cases):
    sph = torch.from_numpy(np.ascontiguousarray(z["table%d" % c["table"]], dtype=np.float32)).cuda()
    p = apt.make_params(c["w"], c["h"], c["samples"], depth=c["depth"], mode=c["mode"], seed=c["seed"], eps=c["eps"])
    if not c["graph"]:
        counter.zero_()
        fb, u8 = render.render_frame(p, sph, pixel_begin=c["begin"], pixel_count=c["count"])
        torch.cuda.synchronize()
        out["counts%d" % n] = counter.cpu().numpy()
    else:                    # one captured graph, replayed twice with the counter zeroed between the replays
        npix = c["w"] * c["h"]
        fb = torch.zeros((3, npix), device="cuda")
        u8 = torch.zeros((npix, 3), dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            render.render_frame(p, sph, fb=fb, fb_u8=u8)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            render.render_frame(p, sph, fb=fb, fb_u8=u8)
        for r in range(2):
            counter.zero_(); fb.zero_(); u8.zero_()
            g.replay()
            torch.cuda.synchronize()
            out["counts%d_%d" % (n, r)] = counter.cpu().numpy()
            out["fb%d_%d" % (n, r)] = fb.cpu().numpy()
    out["fb%d" % n] = fb.cpu().numpy()
    out["u8%d" % n] = u8.cpu().numpy()
lib.apt_set_trace_counter(None)
rc = lib.apt_check(None)
np.savez(dst, **out)
print(json.dumps({"cases": len(cases), "status": rc}))
'''


def variant_library():
    variant = os.path.join(ROOT, "profiles", "microbench", "lib_first_plan_count.so")
    product = os.path.join(ROOT, "ascendpathtracing_amd", "librender_mi355x.so")
    if not os.path.exists(variant) or os.path.getmtime(variant) < os.path.getmtime(product):   # a test build: made on demand, not by build()
        subprocess.run(["bash", os.path.join(ROOT, "profiles", "build_variant.sh"), "first_plan_count", "-DAPT_COUNT_FIRST_PLAN"], check=True)
    return variant


def accepted_family_tables(L, shapes):
    """The first three accepted members (reference camera) with three different eps, for the shapes in turn."""
    found, used, i = [], set(), 0
    while len(found) < 3:
        w, h = shapes[len(found) % len(shapes)]
        sph, eps, _, _ = fpr.family_case(FAMILY_SEED, i, shape=(w, h), reference_camera=True)
        if eps not in used and fpr.record(L, w, h, sph, eps=eps).any():
            used.add(eps)
            found.append((sph, eps, (w, h), i))
        i += 1
    return found


def predicted_counts(L, rec, w, h, begin, count):
    m = fpr.masks(L, rec, w, h, range(w), range(h)).ravel()        # [c * h + r]: pixel q
    q0 = begin + 2 * np.arange((count + 1) // 2)
    q1 = np.where(q0 + 1 < begin + count, q0 + 1, begin)
    both = m[q0] & m[q1]
    return [int(((both >> k) & 1).sum()) for k in range(8)]


@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    from ascendpathtracing_amd import _lib
    _lib.require_gpu()
    L = fpr.twin()
    ref = fpr.reference_table()
    near = ref.copy()
    near[8 + 5] = np.nextafter(near[8 + 5], np.float32(1e9))          # cx of sphere 5 moved by one ulp: the plan refuses the table
    fam = accepted_family_tables(L, [(64, 36), (33, 19)])
    tables = [ref, near] + [t[0] for t in fam]
    K, O = 0, 1
    cases = []

    def case(table, w, h, depth, mode, eps=1e-4, begin=0, count=None, graph=False, seed=3):
        cases.append(dict(table=table, w=w, h=h, depth=depth, mode=mode, eps=float(np.float32(eps)), begin=begin,
                          count=w * h - begin if count is None else count, graph=graph, seed=seed, samples=S))

    for (w, h) in ((64, 36), (33, 19)):                               # 33 x 19: an odd pixel count, the last wave holds one pixel
        for depth, mode in ((1, K), (3, O), (3, K), (1, O)):
            case(0, w, h, depth, mode)
        case(0, w, h, 3, K if w == 64 else O, begin=3 * h + h // 2 + 1, count=(w - 7) * h - 5)   # starts and ends mid-column
    for n, (sph, eps, (w, h), _) in enumerate(fam):
        case(2 + n, w, h, 1 if n == 1 else 3, K, eps=eps)
        case(2 + n, w, h, 3 if n == 1 else 1, O, eps=eps)
    case(1, 64, 36, 3, K)
    case(1, 33, 19, 1, O)
    case(0, 64, 36, 3, K, graph=True)
    d = tmp_path_factory.mktemp("first_plan_device")
    src, dst = str(d / "cases.npz"), str(d / "results.npz")
    np.savez(src, cases=json.dumps(cases), **{f"table{n}": t for n, t in enumerate(tables)})
    env = dict(os.environ, APT_LIB_PATH=variant_library())
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, src, dst], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    head = json.loads(r.stdout.strip().splitlines()[-1])
    assert head == {"cases": len(cases), "status": 0}, head
    return dict(cases=cases, tables=tables, results=np.load(dst), twin=L, family_members=[t[3] for t in fam])


def check_counts(run, c, counts, refused):
    L = run["twin"]
    w, h, begin, count = c["w"], c["h"], c["begin"], c["count"]
    rec = fpr.record(L, w, h, run["tables"][c["table"]], eps=c["eps"])
    assert rec.any() != refused, (c, rec)
    waves = (count + 1) // 2
    got = [int(v) for v in counts[B + 16:B + 30]]
    print(c, "record", got, "waves", int(counts[B]), "taken", int(counts[B + 1]), "left out", [int(v) for v in counts[B + 2:B + 10]])
    assert got == rec[:14].tolist(), (c, got, rec[:14].tolist())                      # the record the kernel read is the twin's, exactly
    assert int(counts[B + 30]) != 0, c                                                 # a launch's ticket is never 0
    assert int(counts[B]) == waves and int(counts[B + 1]) == waves, (c, int(counts[B]), int(counts[B + 1]), waves)
    want = predicted_counts(L, rec, w, h, begin, count)
    assert [int(v) for v in counts[B + 2:B + 10]] == want, (c, [int(v) for v in counts[B + 2:B + 10]], want)
    if refused:
        assert not any(got) and not any(want)
    return want


def test_the_device_reads_the_twins_record_and_every_wave_takes_it(device_run):
    for n, c in enumerate(device_run["cases"]):
        if c["graph"]:
            continue
        want = check_counts(device_run, c, device_run["results"][f"counts{n}"], refused=c["table"] == 1)
        if c["table"] == 0 and (c["w"], c["h"]) == (64, 36) and c["begin"] == 0:
            assert all(want[k] > 0 for k in fpr.RULE_BITS), want                       # every rule leaves its sphere out in some wave
        if c["table"] >= 2:
            assert any(want), (c, want)                                                # a family table's plan is not empty either


def test_a_replayed_graph_makes_and_takes_the_record_again(device_run):
    (n, c), = [(n, c) for n, c in enumerate(device_run["cases"]) if c["graph"]]
    first, second = device_run["results"][f"counts{n}_0"], device_run["results"][f"counts{n}_1"]
    check_counts(device_run, c, first, refused=False)
    check_counts(device_run, c, second, refused=False)
    # the captured launch keeps its ticket: both replays read a record that carries it, written again by the replayed plan kernel
    assert np.array_equal(first[B:B + 32], second[B:B + 32])
    assert np.array_equal(device_run["results"][f"fb{n}_0"].view(np.uint32), device_run["results"][f"fb{n}_1"].view(np.uint32))


def test_the_counting_builds_frames_equal_the_oracle(device_run, oracle):
    for n, c in enumerate(device_run["cases"]):
        p = oracle.make_params(c["w"], c["h"], S, depth=c["depth"], mode=oracle.MODE_O if c["mode"] else oracle.MODE_K, seed=c["seed"], eps=c["eps"])
        fb_w, u8_w, _, _ = oracle.render_frame(p, device_run["tables"][c["table"]], pixel_begin=c["begin"], pixel_count=c["count"],
                                               threads=oracle.max_threads())
        fb, u8 = device_run["results"][f"fb{n}"], device_run["results"][f"u8{n}"]
        assert np.array_equal(np.ascontiguousarray(fb, dtype=np.float32).view(np.uint32), np.ascontiguousarray(fb_w, dtype=np.float32).view(np.uint32)), c
        assert np.array_equal(u8, u8_w), c
