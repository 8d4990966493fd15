"""CPU-only: the six film-stage libraries are linked from one scaffold (csrc/film_stage_host.cpp), and each must still keep an error
record of its own: a refusal in one library leaves what the other five report, and a call that succeeds clears its own record alone.
And the binding's table of the stages names what the build makes: build_id() hashes the files a hand-written list names, in its order,
and the Makefile's STAGES are the table's."""
import ctypes
import glob
import hashlib
import os
import re

from ascendpathtracing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stage -> its *_default_host entry, its record type and the arguments after the record
DEFAULTS = {"denoise": ("apt_film_denoise_default_host", _lib.ApFilmDenoise, (4,)),
            "adaptive": ("apt_film_select_default_host", _lib.ApFilmSelect, (4,)),
            "history": ("apt_film_history_default_host", _lib.ApFilmHistory, ()),
            "post": ("apt_film_meter_default_host", _lib.ApFilmMeter, (4,)),
            "metrics": ("apt_film_compare_default_host", _lib.ApFilmCompare, (4, 1)),
            "upscale": ("apt_film_upscale_default_host", _lib.ApFilmUpscale, ())}


def _last_errors():
    return {name: getattr(_lib.stage_lib(name), st.last_error)() for name, st in _lib.STAGES.items()}


def test_each_stage_library_keeps_an_error_record_of_its_own():
    assert set(DEFAULTS) == set(_lib.STAGES)
    for name, (entry, _, args) in DEFAULTS.items():             # a null record: every library holds a refusal of its own
        assert getattr(_lib.stage_lib(name), entry)(None, *args) != _lib.APT_OK
    want = {name: f"{entry}: the record is null".encode() for name, (entry, _, _) in DEFAULTS.items()}
    assert _last_errors() == want
    for name, (entry, record, args) in DEFAULTS.items():
        assert getattr(_lib.stage_lib(name), entry)(ctypes.byref(record()), *args) == _lib.APT_OK
        assert _last_errors() == dict(want, **{name: b""})      # the call that succeeded cleared its own library's record alone
        assert getattr(_lib.stage_lib(name), entry)(None, *args) != _lib.APT_OK
        assert _last_errors() == want                           # and its next refusal touched no other


def test_the_stage_table_names_what_a_hand_written_list_would():
    csrc = os.path.join(ROOT, "ascendpathtracing_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")))
    files += [os.path.join(csrc, "Makefile"), os.path.join(csrc, "apt_exports.map")]
    files += [os.path.join(ROOT, "include", h) for h in ("render_mi355x.h", "render_mi355x_denoise.h", "render_mi355x_adaptive.h",
                                                         "render_mi355x_history.h", "render_mi355x_post.h", "render_mi355x_metrics.h",
                                                         "render_mi355x_upscale.h")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    assert _lib.build_id() == h.hexdigest()[:16]
    stages = re.search(r"^STAGES\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert stages == list(_lib.STAGES)
    for name, st in _lib.STAGES.items():
        assert os.path.basename(st.built_path) == f"lib{name}_mi355x.so" and st.last_error in st.prototypes
