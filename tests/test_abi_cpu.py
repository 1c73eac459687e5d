"""CPU-only: the C-ABI library builds, loads, and exports every symbol include/dclip_hip.h declares."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(REPO, "include", "dclip_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dclip_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    from dclip_amd import _lib
    assert declared_symbols() == sorted(_lib.SIGNATURES), "include/dclip_hip.h and dclip_amd/_lib.py differ"


def declared_signatures():
    """{name: (return type, [parameter type, ...])} as the header declares them, each type reduced to one of
    'ptr' (any pointer or array, the stream included), 'int*' (a pointer or array of int), 'char*', 'int', 'float',
    'size_t', 'int64_t', 'void'."""
    src = open(os.path.join(REPO, "include", "dclip_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)

    def kind(text: str, is_param: bool) -> str:
        text = text.strip()
        pointer = "*" in text or "[" in text
        words = [w for w in re.sub(r"\[[^\]]*\]|\*", " ", text).split() if w not in ("const", "restrict", "__restrict__")]
        if is_param and len(words) > 1:
            words = words[:-1]                     # the parameter's name
        base = " ".join(words)
        if pointer:                                # whatever it points to (float, uint16_t, int32_t, ...): an address
            return {"int": "int*", "char": "char*"}.get(base, "ptr")
        assert base in ("int", "float", "size_t", "int64_t", "void"), f"unknown type in {text!r}"
        return base

    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dclip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        ret = ret.replace('extern "C"', "").strip()
        params = params.strip()
        plist = [] if params in ("", "void") else [kind(t, True) for t in params.split(",")]
        assert name not in out, f"{name} is declared twice"
        out[name] = (kind(ret, False), plist)
    return out


def test_header_and_binding_agree_on_every_type():
    """_lib.SIGNATURES is a hand copy of the header: every return type and every parameter, position by position.  Pointers,
    arrays and the stream are c_void_p; a binding may name a typed pointer for an int array (dclip_gemm_f32_plan's out[4])."""
    from dclip_amd import _lib
    C = ctypes
    scalar = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "int64_t": C.c_int64}
    decl = declared_signatures()
    assert sorted(decl) == declared_symbols(), "the declaration parser missed a symbol"
    typed_int_pointers = []
    bad = []
    for name, (ret, params) in sorted(decl.items()):
        res, args = _lib.SIGNATURES[name]
        want_res = C.c_char_p if ret == "char*" else scalar.get(ret)
        if want_res is None or res is not want_res:
            bad.append(f"{name}: returns {ret}, bound as {res}")
        if len(args) != len(params):
            bad.append(f"{name}: {len(params)} parameters declared, {len(args)} bound")
            continue
        for i, (k, a) in enumerate(zip(params, args)):
            if k in scalar:
                ok = a is scalar[k]
            elif k == "int*" and a is not C.c_void_p:
                ok = a is C.POINTER(C.c_int)
                typed_int_pointers.append((name, i))
            else:
                ok = k in ("ptr", "int*") and a is C.c_void_p
            if not ok:
                bad.append(f"{name}: parameter {i} is {k}, bound as {a}")
    assert not bad, "include/dclip_hip.h and dclip_amd/_lib.py differ:\n" + "\n".join(bad)
    assert typed_int_pointers == [("dclip_gemm_f32_plan", 5)], typed_int_pointers


def test_library_exports_every_declared_symbol():
    from dclip_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.load().dclip_abi_version() == 1


def test_argument_errors_do_not_need_a_gpu():
    from dclip_amd import _lib
    lib = _lib.load()
    rc = lib.dclip_gemm_f32(None, None, None, None, None, None, 4, 4, 4, 4, 4, 4, 3, 0, 1.0, 0, None, 0, None)
    assert rc == -1
    assert b"null operand" in lib.dclip_last_error()
    with pytest.raises(_lib.DclipError):
        _lib.check(rc, "gemm")


def test_text_embed_bwd_refuses_the_shapes_its_forward_refuses():
    from dclip_amd import _lib
    lib = _lib.load()
    ptr = 4096                                   # never dereferenced: every case below is refused before a launch
    for B, T, D, vocab in [(0, 8, 64, 100), (2, 0, 64, 100), (2, 8, 0, 100), (2, 8, 6, 100), (2, 8, 64, 0), (-1, 8, 64, 100)]:
        assert lib.dclip_text_embed_bwd(ptr, ptr, ptr, B, T, D, vocab, None) == -1, (B, T, D, vocab)
        assert b"text_embed_bwd: bad shape" in lib.dclip_last_error()
        if D != 0:
            assert lib.dclip_text_embed_fwd(ptr, ptr, ptr, ptr, B, T, D, vocab, None) == -1, (B, T, D, vocab)
    assert lib.dclip_text_embed_bwd(None, ptr, ptr, 2, 8, 64, 100, None) == -1 and b"null pointer" in lib.dclip_last_error()


def test_product_path_does_not_import_oracle():
    bad = []
    for root, _, files in os.walk(os.path.join(REPO, "dclip_amd")):
        for f in files:
            if f.endswith(".py"):
                s = open(os.path.join(root, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", s, flags=re.M):
                    bad.append(f)
    assert not bad, f"product modules import the oracle: {bad}"
