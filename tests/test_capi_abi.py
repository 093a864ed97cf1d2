"""CPU (-m "not gpu"): the Python side of the C ABI against include/ftcf.h, whole.  Signatures: every declaration of the header
is parsed and compared, parameter by parameter, with capi.PROTOTYPES.  Layouts: for every mirror in capi.STRUCTS one C program
compiled against the header prints the struct's size and each field's offset and size, and ctypes must agree on all of them.
The per-feature host tests call check_mirror() for the structs their feature touched."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from fastertransformer4codefuse_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = shutil.which("gcc") or shutil.which("cc")

# what a parameter of the header must be bound with
SCALARS = {"int": C.c_int, "ftcf_dtype": C.c_int, "ftcf_act": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "long": C.c_long,
           "unsigned long long": C.c_ulonglong}
HANDLES = ("ftcf_gptneox_t", "ftcf_batcher_t", "ftcf_comm_t")
CALLBACKS = {"ftcf_host_allgather_fn": capi.HOST_ALLGATHER, "ftcf_token_callback_fn": capi.BATCHER_TOKEN_CALLBACK}
RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
POINTEES = {**{cls: name for name, cls in capi.STRUCTS.items()}, C.c_int: "int", C.c_long: "long"}


def header():
    """include/ftcf.h without its comments"""
    with open(os.path.join(ROOT, "include", "ftcf.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def declarations():
    """{name: (return type, [parameter, ...])} of every function the header declares"""
    found = re.findall(r"^(const char\*|int|size_t)\s+(ftcf_\w+)\(([^)]*)\);", header(), flags=re.M)
    return {name: (ret, [] if args.strip() == "void" else [" ".join(a.split()) for a in args.split(",")]) for ret, name, args in found}


def expected(param):
    """the ctypes type a C parameter is bound with; "pointer" for every pointer, array and handle"""
    if "*" in param or "[" in param:
        return "pointer"
    ctype = re.sub(r"^const ", "", param).rsplit(" ", 1)[0]  # (without the parameter's name)
    if ctype in HANDLES:
        return "pointer"
    if ctype in CALLBACKS:
        return CALLBACKS[ctype]
    assert ctype in SCALARS, f"a kind of parameter this test does not know: {param!r}"
    return SCALARS[ctype]


def bound(argtype, param):
    """the same for an entry of the table; a typed pointer must point at what the header names"""
    if isinstance(argtype, type) and issubclass(argtype, C._Pointer):
        assert re.search(r"\b" + POINTEES[argtype._type_] + r"\s*\*", param), (argtype, param)
        return "pointer"
    return "pointer" if argtype is C.c_void_p else argtype


def test_every_declaration_of_the_header_has_its_prototype():
    decl = declarations()
    assert sorted(decl) == sorted(capi.EXPORTED), "the header and EXPORTED name the same functions"
    assert sorted(capi.PROTOTYPES) == sorted(capi.EXPORTED), "one entry per exported name"
    for name, (ret, params) in decl.items():
        restype, argtypes = capi.PROTOTYPES[name]
        assert restype is RETURNS[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (argtype, param) in enumerate(zip(argtypes, params)):
            assert bound(argtype, param) == expected(param), (name, i, param, argtype)


def test_the_loaded_library_carries_the_table():
    L = capi.lib()
    for name, (restype, argtypes) in capi.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def header_fields(struct):
    """the field names of a struct of the header, in its order"""
    body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", header()).group(1)
    return [re.findall(r"\w+", piece)[-1] for decl in body.split(";") if decl.strip() for piece in decl.split(",")]


@functools.lru_cache(maxsize=None)
def compiled_layouts():
    """{struct: [sizeof, offsetof and sizeof of every field of its mirror, ...]} as the host C compiler lays the header out"""
    assert CC is not None, "no C compiler (the caller skips)"
    body = ""
    for struct, cls in capi.STRUCTS.items():
        body += f'  printf("%zu", sizeof({struct}));\n'
        for n, _ in cls._fields_:
            body += f'  printf(" %zu %zu", offsetof({struct}, {n}), sizeof((({struct}*)0)->{n}));\n'
        body += '  printf("\\n");\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "ftcf.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
        out = subprocess.run([CC, "-I" + os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(lines) == len(capi.STRUCTS)
    return {struct: [int(v) for v in line.split()] for struct, line in zip(capi.STRUCTS, lines)}


def check_mirror(struct):
    """capi.STRUCTS[struct] has the header's fields, in its order, each at its offset and of its size, and the struct's size"""
    cls = capi.STRUCTS[struct]
    names = [n for n, _ in cls._fields_]
    assert names == header_fields(struct), struct
    want = [C.sizeof(cls)]
    for n in names:
        want += [getattr(cls, n).offset, getattr(cls, n).size]
    assert want == compiled_layouts()[struct], struct


STRUCT_NAMES = ["ftcf_smallm_problem", "ftcf_gemm_plan", "ftcf_ln_gemv_args", "ftcf_residual_gemv_args", "ftcf_dynamic_decode_args",
                "ftcf_beam_search_args", "ftcf_logit_process_args", "ftcf_gptneox_config", "ftcf_gptneox_weights", "ftcf_forward_args",
                "ftcf_forward_stats", "ftcf_batcher_options", "ftcf_logit_options", "ftcf_beam_options"]


def test_every_struct_of_the_header_has_a_mirror():
    assert sorted(capi.STRUCTS) == sorted(STRUCT_NAMES) == sorted(re.findall(r"typedef struct \{[^}]*\} (ftcf_\w+);", header()))


@pytest.mark.skipif(CC is None, reason="no C compiler")
@pytest.mark.parametrize("struct", STRUCT_NAMES)
def test_mirror_matches_the_compiled_header(struct):
    check_mirror(struct)
