"""The ctypes declaration of the C ABI (lm_abi.PROTOTYPES and the structures) held to include/amd_linemod.h and to the symbols
libamdlinemod.so exports.  CPU only.  The header is plain C with one prototype per statement, so a regular-expression reader is
enough: comments and preprocessor lines go, the struct typedefs are taken out, every remaining statement is a prototype."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import lm_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"lm_match": lm_abi._CMatch, "lm_timings": lm_abi.Timings, "lm_pose_result": lm_abi._CPoseResult,
           "lm_detection": lm_abi._CDetection, "lm_pipeline_timings": lm_abi.PipelineTimings, "lm_icp_options": lm_abi.IcpOptions,
           "lm_render_options": lm_abi.RenderOptions}
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
# exported lm_ symbols that are not in the header (name: reason)
NOT_PUBLIC = {"lm_detector_exchange_merge_group_strided": "csrc/exchange.cpp's common body of lm_detector_exchange_merge_group and "
                                                          "_merge_frame_strided, extern \"C\" without a prototype in the header; nothing calls it from outside"}


def _read_header():
    """(functions {name: (return type, [parameter declarations])}, structs {name: [(type, member, array length or 0)]})."""
    text = open(os.path.join(ROOT, "include", "amd_linemod.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    text = text.replace('extern "C" {', "")
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        members = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            ctype, first = stmt.split(",")[0].rsplit(None, 1)
            for decl in [first] + [d.strip() for d in stmt.split(",")[1:]]:
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", decl)
                members.append((ctype, m.group(1), int(m.group(2) or 0)))
        structs[name] = members
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", "", text)
    funcs = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        if stmt == "}":                                      # the end of extern "C"
            continue
        m = re.fullmatch(r"(.+?)\b(lm_\w+) ?\((.*)\)", stmt)
        assert m, "not a prototype: %r" % stmt
        assert m.group(2) not in funcs, m.group(2)
        params = [p.strip() for p in m.group(3).split(",")]
        funcs[m.group(2)] = (m.group(1).strip(), [] if params == ["void"] else params)
    return funcs, structs


FUNCS, HEADER_STRUCTS = _read_header()


def _is_int(t, size, signed):
    return (isinstance(t, type) and issubclass(t, ctypes._SimpleCData) and t._type_ in "bBhHiIlLqQ" and ctypes.sizeof(t) == size
            and (t(-1).value < 0) == signed)


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _return_ok(c, t):
    if "*" in c:
        return t is (ctypes.c_char_p if c.replace(" ", "") == "constchar*" else ctypes.c_void_p)
    return {"void": lambda: t is None, "int": lambda: t is ctypes.c_int, "int64_t": lambda: _is_int(t, 8, True),
            "uint64_t": lambda: _is_int(t, 8, False), "size_t": lambda: _is_int(t, 8, False)}[c]()


def _param_ok(decl, t):
    if "*" in decl or "[" in decl:
        return _is_pointer(t)
    c = decl.replace("const ", "").rsplit(None, 1)[0]
    return {"int": lambda: t is ctypes.c_int, "int32_t": lambda: t is ctypes.c_int, "float": lambda: t is ctypes.c_float,
            "double": lambda: t is ctypes.c_double, "int64_t": lambda: _is_int(t, 8, True), "uint64_t": lambda: _is_int(t, 8, False),
            "size_t": lambda: _is_int(t, 8, False)}[c]()


def test_the_reader_sees_the_whole_header():
    assert len(FUNCS) > 100 and set(HEADER_STRUCTS) == set(STRUCTS)
    assert FUNCS["lm_last_error"] == ("const char *", []) and FUNCS["lm_merge_matches"] == ("size_t", ["lm_match *m", "size_t n"])
    assert len(FUNCS["lm_mesh_pose_errors"][1]) == 18 and FUNCS["lm_detector_get_response_table"][1][1] == "uint8_t r[5]"


def test_every_function_of_the_header_is_declared_once_with_its_types():
    wrong = []
    for name, (ret, params) in FUNCS.items():
        if name not in lm_abi.PROTOTYPES:
            wrong.append("%s: not in the table" % name)
            continue
        restype, argtypes = lm_abi.PROTOTYPES[name]
        if len(argtypes) != len(params):
            wrong.append("%s: %d argtypes for %d parameters" % (name, len(argtypes), len(params)))
            continue
        if not _return_ok(ret, restype):
            wrong.append("%s: restype %r for %r" % (name, restype, ret))
        wrong += ["%s: argtypes[%d] %r for %r" % (name, i, t, p) for i, (p, t) in enumerate(zip(params, argtypes)) if not _param_ok(p, t)]
    assert not wrong, "\n".join(wrong)
    assert sorted(set(lm_abi.PROTOTYPES) - set(FUNCS)) == []            # reverse coverage: no entry without a prototype in the header


def test_structures_follow_the_header():
    assert ctypes.sizeof(lm_abi._CMatch) == lm_abi.MATCH_DTYPE.itemsize == 20
    assert [n for n, _ in lm_abi._CMatch._fields_] == list(lm_abi.MATCH_DTYPE.names)
    assert [lm_abi.MATCH_DTYPE.fields[n][1] for n in lm_abi.MATCH_DTYPE.names] == [getattr(lm_abi._CMatch, n).offset for n in lm_abi.MATCH_DTYPE.names]
    mirrors = {}
    for name, members in HEADER_STRUCTS.items():                        # in the header's order: a nested struct is defined before its user
        def ctype(c, n):
            base = SCALARS[c] if c in SCALARS else mirrors[c]
            return base * n if n else base
        mirrors[name] = type(name, (ctypes.Structure,), {"_fields_": [(m, ctype(c, n)) for c, m, n in members]})
        ours = STRUCTS[name]
        assert len(ours._fields_) == len(members), name
        assert [f[0] for f in ours._fields_] == [m for _, m, _ in members], name
        assert ctypes.sizeof(ours) == ctypes.sizeof(mirrors[name]), name
        assert [getattr(ours, m).offset for _, m, _ in members] == [getattr(mirrors[name], m).offset for _, m, _ in members], name


def test_the_library_exports_exactly_the_table():
    path = lm_abi.library_path()
    if not os.path.exists(path):
        pytest.skip("libamdlinemod.so is not built")
    lib = lm_abi.load_library()
    for name, (restype, argtypes) in lm_abi.PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("lm_")}
        assert exported - set(NOT_PUBLIC) == set(lm_abi.PROTOTYPES), (sorted(exported ^ set(lm_abi.PROTOTYPES)))
        assert set(NOT_PUBLIC) <= exported
