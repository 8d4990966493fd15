"""CPU-only: the prototype table of the Python binding (ascendpathtracing_amd/_lib.py PROTOTYPES) is include/render_mi355x.h's, entry
by entry; the loaded library carries it; and with it a bare Python integer reaches a 64-bit parameter whole and an argument of the
wrong kind raises instead of being reinterpreted."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the binding's type rules: these C types and nothing else; every other pointer or array parameter is a c_void_p
SCALARS = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t}


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    return pkg


def _param(text):
    if "*" in text or "[" in text:
        return ctypes.c_char_p if re.fullmatch(r"const\s+char\s*\*\s*\w*", text) else ctypes.c_void_p
    words = [w for w in text.split() if w != "const"]
    assert len(words) == 2 and words[0] in SCALARS, f"no rule for the parameter {text!r}"
    return SCALARS[words[0]]


def _result(text):
    if text == "void":
        return None
    if "*" in text:
        kinds = {"const char *": ctypes.c_char_p, "apt_context *": ctypes.c_void_p}
        assert text in kinds, f"no rule for the return type {text!r}"
        return kinds[text]
    assert text in SCALARS, f"no rule for the return type {text!r}"
    return SCALARS[text]


def header_prototypes():
    """include/render_mi355x.h -> {name: (restype, [argtypes])} in the header's order, by the binding's type rules."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "render_mi355x.h")).read(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = {}
    for statement in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(render_do(?:_ex)?|render_frame|apt_[a-z0-9_]+)\s*\(([^()]*)\)\s*", statement)
        if m is None:
            continue
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        assert name not in found, f"{name} is declared twice"
        found[name] = (_result(ret), [] if params == "void" else [_param(a.strip()) for a in params.split(",")])
    return found


def test_the_table_is_the_headers(apt):
    table, header = apt._lib.PROTOTYPES, header_prototypes()
    assert len(header) == 85 and {"render_do", "render_do_ex", "render_frame", "apt_last_error", "apt_context_create"} <= set(header)
    assert header["apt_film_pass_seed"] == (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32])       # the parser itself
    assert header["apt_write_pfm"] == (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p])
    assert header["apt_film_curve_host"] == (ctypes.c_int, [ctypes.c_uint32, ctypes.c_void_p])
    for name, proto in header.items():
        assert name in table, f"{name} is declared in the header and missing from the table"
        assert (table[name][0], list(table[name][1])) == proto, name
    assert list(table) == list(header) + [apt._lib.CXX_RENDER_DO]          # nothing more, and in the header's order
    assert table[apt._lib.CXX_RENDER_DO] == table["render_do"]
    assert apt._lib.ABI_SYMBOLS == list(header)


def test_the_loaded_library_carries_the_table(apt):
    L = apt._lib.lib()
    for name, (restype, argtypes) in apt._lib.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_a_bare_64_bit_integer_arrives_whole(apt):
    """Without argtypes ctypes passes a bare int as a C int: a pixel_begin of 2^32 arrived as 0, an empty range at 0, and the call
    returned APT_OK.  With them it arrives whole and is refused as a range outside the 16 x 16 image."""
    L = apt._lib.lib()
    p = apt.make_params(16, 16, 1)
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first
    assert L.render_frame(ctypes.byref(p), None, one, 1 << 32, 0, one, None) == 1
    assert b"pixel range" in L.apt_last_error()


def test_a_mistyped_argument_raises(apt):
    L = apt._lib.lib()
    with pytest.raises(ctypes.ArgumentError):
        L.apt_film_pass_seed(1.5, 0)
    ctx = L.apt_context_create()
    try:
        with pytest.raises(ctypes.ArgumentError):
            L.apt_context_set_debug(ctx, b"queue_ppw", "x")
    finally:
        L.apt_context_destroy(ctx)
