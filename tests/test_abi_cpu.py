"""The Python side's copy of the C ABI against include/orienmask_hip.h: every prototype's return and argument classes against
lib.SIGNATURES, every struct's field names, offsets and sizes against its ctypes / numpy mirror, every OM_* constant against its
#define.  The header is plain C with one prototype per ';', so regular expressions are enough; nothing is loaded or built."""
import ctypes
import os
import re

import numpy as np

from conftest import REPO
from orienmask_amd import augment, lib as omlib, optim

HEADER = os.path.join(REPO, "include", "orienmask_hip.h")

MIRRORS = {"om_layer_info": omlib.LayerInfo, "om_post_cfg": omlib.PostCfg, "om_rle_image": omlib.RleImage,
           "om_vis_image": omlib.VisImage, "om_loss_cfg": omlib.LossCfg, "om_sgd_tensor": optim.TENSOR_ROW,
           "om_aug_sample": augment.AUG_SAMPLE_DTYPE}
# a typedef struct of the header without a Python mirror, and why it needs none
UNMIRRORED = {"om_sgd_chunk": "two int32: optim.plan_chunks builds the work list as an int32 [n, 2] array, no record type"}

C_SCALARS = {"int": "int", "int32_t": "int", "long long": "longlong", "int64_t": "longlong", "size_t": "size_t", "float": "float",
             "double": "double"}
C_SIZES = {"char": 1, "uint8_t": 1, "int": 4, "int32_t": 4, "uint32_t": 4, "float": 4, "int64_t": 8, "uint64_t": 8, "double": 8,
           "size_t": 8}
POINTER_SIZE = 8


# ------------------------------------------------------------------------------------------------------------ the header
def parse_header(text):
    """(defines {name: int}, structs {name: [(field, offset, size)] + [(None, total size, alignment)]}, prototypes
    {name: (return class, [argument classes])})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    assert "\\\n" not in text, "a continued line: this parser reads one directive per line"
    defines = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*?)[ \t]*$", text, flags=re.M):
        assert re.fullmatch(r"[\w\s()+\-*|&<]+", expr), "cannot evaluate #define %s %s" % (name, expr)
        defines[name] = eval(expr, {"__builtins__": {}}, dict(defines))       # noqa: S307: integers and earlier defines only
        assert isinstance(defines[name], int), name
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text = text.replace('extern "C" {', " ")
    structs = {}
    for tag, body, name in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        assert tag == name, (tag, name)
        structs[name] = struct_layout(body, defines)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{[^{}]*\}\s*\w+\s*;", " ", text)
    text = re.sub(r"typedef\s[^;{}]*;", " ", text)                # the opaque om_model and om_stream
    statements = [s.strip() for s in text.split(";")]
    assert statements[-1] == "}", "what follows the last prototype is not the end of extern \"C\": %r" % statements[-1][:80]
    protos = {}
    for s in statements[:-1]:
        m = re.fullmatch(r"(.+?)\b(\w+)\s*\(([^()]*)\)", s, flags=re.S)
        assert m, "not a prototype: %r" % s[:120]
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        assert name not in protos, name
        protos[name] = (c_class(ret, named=False), [] if params == "void" else [c_class(p) for p in params.split(",")])
    return defines, structs, protos


def c_class(decl, named=True):
    """pointer / int / longlong / size_t / float / double / void of a parameter declaration (or, named=False, a return type);
    an unknown type raises."""
    decl = " ".join(decl.split())
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split(" ") if w != "const"]
    for ctype in ([" ".join(words[:-1])] if named and len(words) > 1 else []) + [" ".join(words)]:
        if ctype == "om_stream":
            return "pointer"
        if ctype == "void" and not named:
            return "void"
        if ctype in C_SCALARS:
            return C_SCALARS[ctype]
    raise AssertionError("unknown C type in %r" % decl)


def struct_layout(body, defines):
    """[(field, offset, size), ..., (None, sizeof, alignment)] with natural alignment."""
    fields, off, align = [], 0, 1
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        pieces = [p.strip() for p in decl.split(",")]
        m = re.fullmatch(r"(.*?)([*\s])(\w+(?:\s*\[\w+\])*)", pieces[0])
        assert m, "not a field declaration: %r" % decl
        ctype = " ".join(w for w in (m.group(1) + m.group(2)).split() if w != "const")
        for d in [m.group(3)] + pieces[1:]:
            pointer = "*" in ctype or d.startswith("*")
            name = re.match(r"\*?\s*(\w+)", d).group(1)
            if pointer:
                elem = POINTER_SIZE
            else:
                assert ctype in C_SIZES, "unknown C type %r in %r" % (ctype, decl)
                elem = C_SIZES[ctype]
            count = 1
            for dim in re.findall(r"\[(\w+)\]", d):
                count *= int(dim) if dim.isdigit() else defines[dim]
            off = (off + elem - 1) // elem * elem
            fields.append((name, off, elem * count))
            off += elem * count
            align = max(align, elem)
    return fields + [(None, (off + align - 1) // align * align, align)]


# ------------------------------------------------------------------------------------------------------------ the Python side
def ctypes_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    if t is ctypes.c_size_t:
        return "size_t"
    if t in (ctypes.c_int, ctypes.c_int32):
        return "int"
    if t in (ctypes.c_longlong, ctypes.c_int64):
        return "longlong"
    if t is ctypes.c_float:
        return "float"
    if t is ctypes.c_double:
        return "double"
    raise AssertionError("unknown ctypes type %r" % (t,))


def mirror_layout(mirror):
    """[(field, offset, size), ..., (None, size of the whole, None)] of a ctypes.Structure or a numpy record dtype."""
    if isinstance(mirror, np.dtype):
        return [(n, mirror.fields[n][1], mirror.fields[n][0].itemsize) for n in mirror.names] + [(None, mirror.itemsize, None)]
    return [(n, getattr(mirror, n).offset, getattr(mirror, n).size) for n, *_ in mirror._fields_] + [(None, ctypes.sizeof(mirror), None)]


def prototype_mismatches(protos, signatures):
    out = []
    for name in sorted(set(protos) | set(signatures)):
        if name not in protos or name not in signatures:
            out.append("%s: only in %s" % (name, "the header" if name in protos else "SIGNATURES"))
            continue
        (ret, args), (res, argtypes) = protos[name], signatures[name]
        if ctypes_class(res) != ret:
            out.append("%s: returns %s, restype is %s" % (name, ret, ctypes_class(res)))
        if len(args) != len(argtypes):
            out.append("%s: %d parameters, %d argtypes" % (name, len(args), len(argtypes)))
            continue
        for i, (c, t) in enumerate(zip(args, argtypes)):
            if ctypes_class(t) != c:
                out.append("%s: parameter %d is %s, argtype is %s" % (name, i, c, ctypes_class(t)))
    return out


def struct_mismatches(name, c_layout, py_layout):
    out = []
    if [f[0] for f in c_layout] != [f[0] for f in py_layout]:
        return ["%s: fields %s in the header, %s in Python" % (name, [f[0] for f in c_layout[:-1]], [f[0] for f in py_layout[:-1]])]
    for (field, off, size), (_, poff, psize) in zip(c_layout[:-1], py_layout[:-1]):
        if (off, size) != (poff, psize):
            out.append("%s.%s: offset, size %s in the header, %s in Python" % (name, field, (off, size), (poff, psize)))
    if c_layout[-1][1] != py_layout[-1][1]:
        out.append("%s: sizeof %d in the header, %d in Python" % (name, c_layout[-1][1], py_layout[-1][1]))
    return out


def _parsed():
    with open(HEADER) as f:
        return parse_header(f.read())


DEFINES, STRUCTS, PROTOS = _parsed()


# ------------------------------------------------------------------------------------------------------------ the checks
def test_every_prototype_matches_its_signature():
    assert len(PROTOS) == len(omlib.SIGNATURES) and len(PROTOS) > 100
    assert all(name.startswith("om_") for name in PROTOS)
    assert prototype_mismatches(PROTOS, omlib.SIGNATURES) == []
    # the _bf16 aliases share their float32 entry's argtypes list in Python: each has a prototype of its own in the header
    bf16 = [n for n in omlib.SIGNATURES if n.endswith("_bf16")]
    assert len(bf16) == 8 and all(n in PROTOS and PROTOS[n] == PROTOS[n[:-len("_bf16")]] for n in bf16)


def test_every_struct_matches_its_mirror():
    assert set(STRUCTS) == set(MIRRORS) | set(UNMIRRORED), "a typedef struct of the header is neither mirrored nor listed as unmirrored"
    assert not set(MIRRORS) & set(UNMIRRORED) and all(UNMIRRORED.values())
    for name, mirror in MIRRORS.items():
        assert struct_mismatches(name, STRUCTS[name], mirror_layout(mirror)) == [], name
    assert STRUCTS["om_sgd_chunk"] == [("tensor", 0, 4), ("chunk", 4, 4), (None, 8, 4)]      # what plan_chunks' rows are
    # the parser against layouts known by hand: padding in front of an 8-byte field, a multi-declarator line, OM_* array bounds
    assert STRUCTS["om_rle_image"][:3] == [("mask", 0, 8), ("K", 8, 4), ("H", 12, 4)] and STRUCTS["om_rle_image"][-1] == (None, 56, 8)
    assert ("anchor_mask", 4 + 24 + 8 + 4 + 72, 36) in STRUCTS["om_post_cfg"]
    assert STRUCTS["om_sgd_tensor"][-1][1] == 64 and STRUCTS["om_aug_sample"][-1][1] == 160


def test_every_constant_matches_its_define():
    seen = 0
    for module in (omlib, optim):
        for name, value in vars(module).items():
            if name.startswith("OM_") and isinstance(value, int) and not isinstance(value, bool):
                assert name in DEFINES, "%s.%s has no #define" % (module.__name__, name)
                assert DEFINES[name] == value, (module.__name__, name, value, DEFINES[name])
                seen += 1
    assert seen >= 23 + 7
    assert DEFINES["OM_LOSS_RESULT_FLOATS"] == 3 * (7 + 2 * 8) + 1 and DEFINES["OM_COUNTER_BLOCK_DOUBLES"] == 4 * 65 + 2


def test_the_comparison_can_fail():
    """A perturbed copy of one SIGNATURES entry and of one struct layout, in memory only: each is reported."""
    sigs = {k: (r, list(a)) for k, (r, a) in omlib.SIGNATURES.items()}
    res, args = sigs["om_conv2d_split_k"]
    assert args[6] is ctypes.c_void_p
    args[6] = ctypes.c_int                                    # a pointer declared as int: the address would be truncated
    assert prototype_mismatches(PROTOS, sigs) == ["om_conv2d_split_k: parameter 6 is pointer, argtype is int"]
    sigs["om_conv2d_split_k"] = (res, omlib.SIGNATURES["om_conv2d_split_k"][1][:-1])         # a dropped argument
    assert prototype_mismatches(PROTOS, sigs) == ["om_conv2d_split_k: 24 parameters, 23 argtypes"]
    sigs["om_conv2d_split_k"] = (ctypes.c_size_t, omlib.SIGNATURES["om_conv2d_split_k"][1])
    assert prototype_mismatches(PROTOS, sigs) == ["om_conv2d_split_k: returns int, restype is size_t"]
    del sigs["om_conv2d_split_k"]
    assert prototype_mismatches(PROTOS, sigs) == ["om_conv2d_split_k: only in the header"]
    sz = list(omlib.SIGNATURES["om_bn_act_forward"][1])
    sz[19] = ctypes.c_int                                     # size_t ws_bytes as int
    assert prototype_mismatches({"om_bn_act_forward": PROTOS["om_bn_act_forward"]}, {"om_bn_act_forward": (ctypes.c_int, sz)}) \
        == ["om_bn_act_forward: parameter 19 is size_t, argtype is int"]

    class Narrow(ctypes.Structure):                           # om_rle_image with K as int64: K and everything behind it moves
        _fields_ = [(n, ctypes.c_int64 if n == "K" else t) for n, t in omlib.RleImage._fields_]
    bad = struct_mismatches("om_rle_image", STRUCTS["om_rle_image"], mirror_layout(Narrow))
    assert bad[0] == "om_rle_image.K: offset, size (8, 4) in the header, (8, 8) in Python"
    assert len(bad) == 11                                     # K and the ten fields behind it; the tail padding hides it from sizeof

    class Renamed(ctypes.Structure):
        _fields_ = [("k" if n == "K" else n, t) for n, t in omlib.RleImage._fields_]
    assert len(struct_mismatches("om_rle_image", STRUCTS["om_rle_image"], mirror_layout(Renamed))) == 1
    row = np.dtype([(n, "<u4" if n == "n" else optim.TENSOR_ROW.fields[n][0]) for n in optim.TENSOR_ROW.names])
    assert any(m.startswith("om_sgd_tensor.n:") for m in struct_mismatches("om_sgd_tensor", STRUCTS["om_sgd_tensor"], mirror_layout(row)))
    try:
        c_class("unsigned count")
    except AssertionError as e:
        assert "unknown C type" in str(e)
    else:
        raise AssertionError("an unknown C type was classified")
