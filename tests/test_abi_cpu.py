"""``smoltts_amd/abi.py`` held to ``include/smoltts_hip.h``: every prototype against the signature table, every mirrored struct
against the host compiler's layout, every mirrored constant against the header's value.  No GPU, no library call beyond dlopen."""
import ctypes as C
import itertools
import re
import subprocess

from smoltts_amd import abi, build
from test_host_cpu import ROOT, _declared_functions

HEADER = ROOT / "include" / "smoltts_hip.h"
SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "size_t": "size", "uint64_t": "u64", "uint32_t": "u32",
           "float": "f32", "double": "f64"}
LETTERS = {"p": ("ptr", C.c_void_p), "i": ("i32", C.c_int32), "q": ("i64", C.c_int64), "z": ("size", C.c_size_t),
           "Q": ("u64", C.c_uint64), "f": ("f32", C.c_float), "d": ("f64", C.c_double)}  # the table's spelling of the scalar kinds


def _header_text() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _c_kind(decl: str) -> str:
    """Kind of one C parameter / return declaration: ``ptr`` for anything with a ``*``, else its scalar type."""
    if "*" in decl:
        return "ptr"
    words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w not in ("const", "struct")]
    assert words and words[0] in SCALARS, f"unreadable C type in {decl!r}"
    return SCALARS[words[0]]


def _prototypes():
    """{name: (return declaration, [parameter declarations])} of every function the header declares."""
    out = {}
    text = re.sub(r"^[ \t]*#.*$", "", _header_text(), flags=re.M)  # (one-line preprocessor directives only)
    for ret, name, params in re.findall(r"(?:\A|(?<=[;{}]))\s*((?:const\s+)?\w+[\s*]+)(smoltts_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        out[name] = (ret.strip(), [] if params == ["void"] else params)
    return out


def _spelled_kind(kind: str) -> str:
    """Kind of one argument as the table spells it (abi.SIGNATURES): the letter, not the ctypes class it resolves to."""
    return "ptr" if kind.endswith("*") else LETTERS[kind][0]


def test_every_prototype_matches_the_table():
    protos = _prototypes()
    assert len(protos) == len(_declared_functions()), \
        f"could not read the prototype of {sorted(set(_declared_functions()) - set(protos))}"
    for name, (ret, params) in protos.items():
        assert name in abi.SIGNATURES, f"{name} is declared in the header but has no entry in abi.SIGNATURES"
        restype, kinds = abi.SIGNATURES[name]
        want = [_c_kind(p) for p in params]
        got = [_spelled_kind(k) for k in kinds.split()]
        assert len(got) == len(want), f"{name}: the table has {len(got)} arguments, the header {len(want)}"
        for i, (g, w, p) in enumerate(zip(got, want, params)):
            assert g == w, f"{name}: argument {i} ({p}) is {w} in the header, {g} in the table"
        if ret == "void":
            assert restype is None, f"{name} returns void"
        elif "*" in ret:
            assert ret.replace(" ", "") == "constchar*" and restype is C.c_char_p, f"{name} returns {ret}"
        elif _c_kind(ret) == "size":
            assert restype is C.c_size_t, f"{name} returns size_t"
        else:
            assert _c_kind(ret) == "i32" and restype in (C.c_int, C.c_int32) and C.sizeof(restype) == 4, f"{name} returns {ret}"
    for name in abi.SIGNATURES:
        assert name in protos, f"{name} is in abi.SIGNATURES but not declared in the header"
    assert set(abi.DEBUG_HOOKS) == {"smoltts_profile_begin", "smoltts_profile_end"} and not set(abi.DEBUG_HOOKS) & set(protos)


def test_the_table_resolves_to_the_ctypes_it_spells():
    """What ``load_library`` applies: each letter is the ctypes class of its kind, each ``X*`` a POINTER."""
    assert abi._KINDS == {k: t for k, (_, t) in LETTERS.items()} and C.sizeof(C.c_int) == 4
    for table in (abi.SIGNATURES, abi.DEBUG_HOOKS):
        for name, (_, kinds) in table.items():
            for k in kinds.split():
                assert issubclass(abi._argtype(k), C._Pointer) if k.endswith("*") else abi._argtype(k) is LETTERS[k][1], f"{name}: {k}"


def _struct_bodies():
    """{header struct name: [field names in order]} of every ``typedef struct Name { ... } Name;``."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", _header_text(), flags=re.S):
        fields = []
        for stmt in body.split(";"):
            if not stmt.strip():
                continue
            head, *rest = stmt.split(",")  # "int32_t M, N, K" / "uint64_t in_proj[2]" / "const float* x_dev"
            for piece in [head] + rest:
                ident = re.findall(r"[A-Za-z_]\w*", re.sub(r"\[[^\]]*\]", "", piece))
                assert ident, f"unreadable field in {name}: {stmt!r}"
                fields.append(ident[-1])
        out[name] = fields
    return out


def test_struct_layouts_match_the_host_compiler(tmp_path):
    bodies = _struct_bodies()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "smoltts_hip.h"', "int main(void) {"]
    for s in abi.STRUCTS:
        c_name = "Smoltts" + s.__name__
        assert c_name in bodies, f"abi.{s.__name__} mirrors no struct of the header"
        names = [f[0] for f in s._fields_]
        for i, (mine, theirs) in enumerate(itertools.zip_longest(names, bodies[c_name])):
            assert mine == theirs, f"{s.__name__}: field {i} is {mine!r} in abi.py, {theirs!r} in the header"
        lines.append(f'  printf("{s.__name__} sizeof %zu\\n", sizeof({c_name}));')
        for n in names:
            lines.append(f'  printf("{s.__name__} {n} %zu %zu\\n", offsetof({c_name}, {n}), sizeof((({c_name}*)0)->{n}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc = build._hipcc()  # (raises when there is no compiler: nothing here works without it)
    r = subprocess.run([cc, "-x", "c", "-std=c11", f"-I{HEADER.parent}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, f"host compile failed:\n{r.stdout}\n{r.stderr}"
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        struct, field, *nums = line.split()
        got[struct, field] = tuple(int(n) for n in nums)
    for s in abi.STRUCTS:
        assert got[s.__name__, "sizeof"] == (C.sizeof(s),), f"{s.__name__}: sizeof {C.sizeof(s)} in abi.py, {got[s.__name__, 'sizeof'][0]} in C"
        for n, _ in s._fields_:
            f = getattr(s, n)
            assert got[s.__name__, n] == (f.offset, f.size), \
                f"{s.__name__}.{n}: (offset, size) {(f.offset, f.size)} in abi.py, {got[s.__name__, n]} in C"
    assert {"Smoltts" + s.__name__ for s in abi.STRUCTS} == set(bodies), "a struct of the header has no mirror in abi.STRUCTS"


def _header_constants():
    """{NAME: value} of every ``NAME = literal`` inside an enum and every ``#define NAME literal`` (int and float literals)."""
    text, out = _header_text(), {}
    literal = r"(-?(?:0[xX][0-9a-fA-F]+|\d+\.\d*|\d+))([uUfF]?)\b"
    pairs = [m for body in re.findall(r"enum\s*\{(.*?)\}", text, flags=re.S) for m in re.findall(r"(SMOLTTS_\w+)\s*=\s*" + literal, body)]
    pairs += re.findall(r"^[ \t]*#define[ \t]+(SMOLTTS_\w+)[ \t]+" + literal + r"[ \t]*$", text, flags=re.M)
    for name, value, _ in pairs:
        out[name] = float(value) if "." in value else int(value, 0)
    return out


def test_constants_match_the_header():
    consts = _header_constants()
    assert consts["SMOLTTS_ABI_VERSION"] == abi.ABI_VERSION
    families = ("E_", "KV_", "W_", "OPT_", "MIMI_OPT_", "PRO_", "EPI_", "RESAMPLE_", "SEAM_", "FLAC_", "FILTER_MAX_", "PREFIX_", "MAX_", "MIMI_MAX_")
    for name, value in consts.items():
        short = name[len("SMOLTTS_"):]
        assert hasattr(abi, short) or not short.startswith(families), f"{name} has no mirror in abi.py"
        if hasattr(abi, short):
            assert getattr(abi, short) == value, f"abi.{short} is {getattr(abi, short)!r}, the header's {name} is {value!r}"
    # every UPPER_CASE number of abi.py is a header constant: nothing there is a second, unchecked literal
    for short, v in vars(abi).items():
        if short.isupper() and isinstance(v, (int, float)) and not isinstance(v, bool):
            assert "SMOLTTS_" + short in consts, f"abi.{short} mirrors no enum member or #define of the header"
    assert abi.KV_FORMATS == {"fp32": consts["SMOLTTS_KV_F32"], "bf16": consts["SMOLTTS_KV_BF16"]}
