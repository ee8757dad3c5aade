"""CPU-only: the C-ABI library loads and exports exactly what include/ppbo_hip.h declares."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", txt)))


def test_header_lists_entry_points():
    syms = header_symbols()
    assert "ppbo_gram" in syms and "ppbo_predict" in syms and "ppbo_fit_fmap" in syms
    assert len(syms) >= 19


def test_library_exports_every_declared_symbol():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    for s in header_symbols():
        assert hasattr(lib, s), f"libppbo_hip.so does not export {s}"
        assert s in _lib.SIGNATURES, f"ctypes binding lacks {s}"
    assert set(_lib.SIGNATURES) == set(header_symbols()) and len(header_symbols()) == 84
    assert lib.ppbo_abi_version() == _lib.ABI_VERSION == 9


def test_library_exports_nothing_but_the_c_abi():
    """-fvisibility=hidden + the version script: the dynamic symbol table is the header's entry points and the HIP
    toolchain's per-TU registration ids (__hip_cuid_*) -- no mangled internals, no device stubs, no libstdc++ weak symbols."""
    import shutil
    import subprocess
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    exported = sorted(n for n in names if not n.startswith("__hip_"))
    assert exported == header_symbols(), sorted(set(exported) ^ set(header_symbols()))
    assert all(n.startswith("__hip_cuid_") for n in names if n.startswith("__hip_"))


def test_no_edge_twins_anywhere():
    """The operator's form is ppbo_model.form / the form argument, a model's coordinate map is ppbo_model.coords / a
    ppbo_coords argument, and its variance projection is ppbo_model.proj: never a function name."""
    import shutil
    import subprocess
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert len(exported) > 50
    for names in (header_symbols(), list(_lib.SIGNATURES), exported):
        assert not [n for n in names if n.endswith(("_edge", "_scaled", "_camphor", "_p"))]


def test_model_struct_matches_the_header(tmp_path):
    """_lib.Model is ppbo_model: `coords` (a ppbo_coords) and `proj` (a ppbo_var_projection) are its last members behind
    `form`, and the sizes and every field offset -- those of the members of coords and of proj included -- are what the C
    compiler gives the header's structs."""
    import ctypes as C
    import shutil
    import subprocess
    from ppbo_amd import _lib
    names = [f[0] for f in _lib.Model._fields_]
    assert names[-3:] == ["form", "coords", "proj"] and _lib.Model.form.size == C.sizeof(C.c_int)
    assert _lib.Model().form == 0          # a zero-initialised model is a node-form model ...
    assert _lib.Model().coords.kind == 0 and not _lib.Model().coords.h_coef and not _lib.Model().coords.d_Xc   # ... in the caller's coordinates
    assert _lib.Model().proj.rows == 0 and not _lib.Model().proj.d_T          # ... without a projection
    cnames = [f[0] for f in _lib.Coords._fields_]
    assert cnames == ["kind", "h_coef", "d_Xc"]
    pnames = [f[0] for f in _lib.VarProjection._fields_]
    assert pnames == ["d_T", "rows", "rows_padded", "ld", "bound", "tol"]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to lay out ppbo_model with"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppbo_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(ppbo_model));\n'
                   + "".join(f'  printf(" %zu", offsetof(ppbo_model, {n}));\n' for n in names)
                   + '  printf(" %zu", sizeof(ppbo_coords));\n'
                   + "".join(f'  printf(" %zu", offsetof(ppbo_model, coords.{n}));\n' for n in cnames)
                   + '  printf(" %zu", sizeof(ppbo_var_projection));\n'
                   + "".join(f'  printf(" %zu", offsetof(ppbo_model, proj.{n}));\n' for n in pnames)
                   + '  printf(" %d %d %d", PPBO_COORDS_MODEL, PPBO_COORDS_SCALED, PPBO_COORDS_CAMPHOR);\n'
                   + '  printf(" %d %d", PPBO_FORM_NODE, PPBO_FORM_EDGE); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.Model)
    nm = len(names)
    assert out[1:1 + nm] == [getattr(_lib.Model, n).offset for n in names]
    assert out[1 + nm] == C.sizeof(_lib.Coords) == _lib.Model.coords.size
    assert out[2 + nm:5 + nm] == [_lib.Model.coords.offset + getattr(_lib.Coords, n).offset for n in cnames]
    assert out[5 + nm] == C.sizeof(_lib.VarProjection) == _lib.Model.proj.size
    assert out[6 + nm:12 + nm] == [_lib.Model.proj.offset + getattr(_lib.VarProjection, n).offset for n in pnames]
    assert _lib.Model.proj.offset + C.sizeof(_lib.VarProjection) == C.sizeof(_lib.Model)      # nothing behind proj
    assert out[12 + nm:15 + nm] == [_lib.COORDS_MODEL, _lib.COORDS_SCALED, _lib.COORDS_CAMPHOR] == [0, 1, 2]
    assert out[-2:] == [0, 1] and len(out) == 17 + nm


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ppbo_amd.engine import Engine
    with pytest.raises(RuntimeError, match="no CPU path"):
        Engine(0)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "ppbo_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S).replace("# the oracle", ""), \
                    f"{f} mentions the oracle: the product path must not depend on it"


def test_ctx_create_without_gpu_returns_an_error_code():
    """No GPU in the build container: the C entry point must report it as a status code, not crash."""
    import ctypes as C
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ppbo_amd import _lib
    lib = _lib.load()
    ctx = C.c_void_p()
    rc = lib.ppbo_ctx_create(0, C.byref(ctx))
    assert rc != 0 and not ctx.value
    assert lib.ppbo_ctx_destroy(None) == 0
    buf = C.create_string_buffer(16)
    assert lib.ppbo_last_error(None, buf, 16) != 0
