"""CPU-only checks of the C-ABI shared library: it loads, exports every symbol ``include/gridpf.h`` declares, and
fails loudly (no CPU fallback) when no GPU is present."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _declared_functions():
    txt = open(os.path.join(ROOT, "include", "gridpf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gpf_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    import __graft_entry__ as entry
    entry.build()
    from grid2op_amd import _capi
    L = _capi.lib()
    declared = _declared_functions()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gridpf.h but not exported by libgridpf.so"
    assert sorted(_capi.EXPORTED_SYMBOLS) == declared
    assert L.gpf_version() >= 100


def test_no_silent_cpu_fallback(load_model):
    """Without a GPU the product path must raise (a CPU fallback would void every parity claim)."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    from grid2op_amd.engine import PowerFlowEngine, GridPFError
    m = load_model("rte_case5_example")
    with pytest.raises(GridPFError):
        PowerFlowEngine(m, n_lanes=2)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "grid2op_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "pf_oracle" not in txt or f == "_capi.py" and "oracle/" in txt, f


# ---- the whole binding against include/gridpf.h: structures, prototypes, constants -------------------------------------------------
_C_SCALARS = {"int": C.c_int, "int8_t": C.c_int8, "int16_t": C.c_int16, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8,
              "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float,
              "double": C.c_double}


def _header():
    txt = open(os.path.join(ROOT, "include", "gridpf.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _struct_class(c_name):
    """gpf_step_opts -> _capi.GpfStepOpts"""
    from grid2op_amd import _capi
    return getattr(_capi, "".join(w.capitalize() for w in c_name.split("_")))


def _ctype(base, stars, dims, param):
    """The ctypes type of the C declaration ``base stars name dims`` as a structure field or (``param``) a function parameter."""
    if base == "gpf_handle":
        t = C.c_void_p
    elif base == "void":
        assert stars, "a void object"
        t, stars = C.c_void_p, stars - 1
    elif base == "char":
        assert stars, "a plain char is not part of the ABI"
        t, stars = C.c_char_p, stars - 1
    elif base in _C_SCALARS:
        t = _C_SCALARS[base]
    else:
        t = _struct_class(base)
    for _ in range(stars):
        t = C.POINTER(t)
    if dims is not None:
        t = C.POINTER(t) if param else t * int(dims)
    return t


def _declaration(text, param):
    """(name, ctypes type) of every declarator of ``[const] T[*] a[, [*]b ...]`` / ``T a[k]``."""
    m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(.*?)\s*", text, flags=re.S)
    assert m, text
    out = []
    for d in m.group(2).split(","):
        dm = re.fullmatch(r"\s*(\**)\s*(?:const\s+)?(\w+)\s*(?:\[\s*(\d*)\s*\])?\s*", d)
        assert dm, text
        out.append((dm.group(2), _ctype(m.group(1), len(dm.group(1)), dm.group(3), param)))
    return out


def _header_structs():
    return {m.group(1): [f for decl in m.group(2).split(";") if decl.strip() for f in _declaration(decl, param=False)]
            for m in re.finditer(r"typedef\s+struct\s+(gpf_\w+)\s*\{(.*?)\}\s*\1\s*;", _header(), flags=re.S)}


def _header_prototypes():
    out = {}
    for m in re.finditer(r"(?:^|[;}])\s*(const\s+char\s*\*|int|void)\s*(gpf_\w+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M):
        ret, name, args = m.groups()
        args = [] if args.strip() == "void" else [_declaration(a, param=True)[0][1] for a in args.split(",")]
        out[name] = (args, C.c_char_p if "char" in ret else None if ret == "void" else C.c_int)
    return out


def test_every_structure_matches_header():
    """Every ``typedef struct gpf_*`` of the header has a ctypes Structure with the same field names, in the same order, of the
    corresponding types (the field names of GpfLayout and GpfGridDesc among them)."""
    structs = _header_structs()
    assert {"gpf_grid_desc", "gpf_layout", "gpf_step_opts", "gpf_opponent_desc", "gpf_alert_desc", "gpf_reward_slot", "gpf_episode_desc",
            "gpf_combined_desc", "gpf_cursor_desc"} <= set(structs)
    for c_name, fields in structs.items():
        cls = _struct_class(c_name)
        assert issubclass(cls, C.Structure)
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields], c_name
        for (name, got), (_, want) in zip(cls._fields_, fields):
            assert got is want, f"{c_name}.{name}: {got} in the binding, {want} in include/gridpf.h"


def test_every_prototype_matches_signature_table():
    """Every ``gpf_*`` prototype of the header has a row in `_capi.SIGNATURES` with as many ``argtypes``, each of the corresponding
    ctypes type, and the corresponding ``restype`` -- and the loaded library carries exactly the table's rows."""
    from grid2op_amd import _capi
    protos = _header_prototypes()
    assert sorted(protos) == _declared_functions() == sorted(_capi.SIGNATURES)
    for name, (want_args, want_res) in protos.items():
        got_args, got_res = _capi.SIGNATURES[name]
        assert len(got_args) == len(want_args), f"{name}: {len(got_args)} argtypes, {len(want_args)} parameters in include/gridpf.h"
        for k, (got, want) in enumerate(zip(got_args, want_args)):
            assert got is want, f"{name} argument {k}: {got} in the binding, {want} in include/gridpf.h"
        assert got_res is want_res, f"{name}: restype {got_res}, header {want_res}"
    assert list(_capi.EXPORTED_SYMBOLS) == list(_capi.SIGNATURES)
    import __graft_entry__ as entry
    entry.build()
    L = _capi.lib()
    for name, (args, res) in _capi.SIGNATURES.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == list(args) and fn.restype is res, name


def test_every_mirrored_constant_matches_header():
    """Every ``#define GPF_<NAME> <integer>`` of the header that `_capi` or `engine` mirrors as ``<NAME>`` has the header's value there."""
    from grid2op_amd import _capi, engine
    defines = {}
    for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+GPF_(\w+)[ \t]+([-+* \t0-9a-fA-FxX()]*[0-9a-fA-F)])[ \t]*$", _header(), flags=re.M):
        defines[name] = int(eval(val, {"__builtins__": {}}))           # an integer literal or a parenthesised integer expression
    matched = set()
    for name, val in defines.items():
        for mod in (_capi, engine):
            if hasattr(mod, name):
                assert getattr(mod, name) == val, f"{mod.__name__}.{name} = {getattr(mod, name)}, GPF_{name} = {val}"
                matched.add(name)
    must = {"ABI_VERSION", "N_DEVICE_POINTERS", "N_ALERT_POINTERS", "N_REWARD_POINTERS", "N_EPISODE_POINTERS", "N_CURSOR_POINTERS",
            "N_COMBINED_POINTERS", "OPP_STATE_INTS", "OPP_AREA_STATE_INTS", "OPP_MAX_AREAS", "OPP_TIME_NONE", "CURSOR_STATE_INTS",
            "REWARD_MAX_SLOTS", "RW_REDISP", "RW_L2RPN", "RW_LINES_CAPACITY", "RW_ECONOMIC", "RW_GAMEPLAY", "MASK_TOO_MANY_LINES",
            "MASK_TOO_MANY_SUBS", "MASK_LINE_COOLDOWN", "MASK_SUB_COOLDOWN", "MASK_AMBIGUOUS", "ALERT_MAX_LINES", "ALERT_MAX_WINDOW"}
    assert must <= matched, sorted(must - matched)


def test_busbar_limit_is_declared_and_validated_before_the_device_is_touched(load_model):
    """The reference takes any n_busbar_per_sub (pandaPowerBackend.py:562-577; grid2op/tests/test_issue_l2g_128.py:218 uses 6).  The
    engine takes up to GPF_MAX_BUSBAR busbars -- split substations run on the bus-level graph of their topology class, only the
    block-kernel fallback is limited to 3 -- and validates the count before it touches the device (no GPU here: a larger count must
    be refused with THAT reason, a legal one must get as far as the missing device)."""
    from grid2op_amd.engine import PowerFlowEngine, GridPFError
    m = load_model("rte_case5_example")
    hdr = open(os.path.join(ROOT, "include", "gridpf.h")).read()
    assert "#define GPF_MAX_BUSBAR 64" in hdr and "#define GPF_MAX_BUSBAR_BLOCKS 3" in hdr
    with pytest.raises(GridPFError, match="more than 64 busbars"):
        PowerFlowEngine(m, n_lanes=2, n_busbar=65)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    if not has_gpu:
        with pytest.raises(GridPFError, match="no HIP device"):
            PowerFlowEngine(m, n_lanes=2, n_busbar=6)


def test_bench_uses_the_oracle_only_as_checker_or_cpu_baseline():
    """bench.py may call the oracle in its cpu_baseline leg and in the spot checks that run AFTER a timed workload -- nowhere
    else (the measured path must be the HIP engine)."""
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    allowed = {"cpu_baseline", "oracle_spot_check", "oracle_dc_check", "workload_ptdf", "workload_ptdf_rows"}       # (the two PTDF records: checker legs after the timed loops)
    found = set()
    for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        for n in ast.walk(fn):
            if isinstance(n, (ast.Import, ast.ImportFrom)):
                names = [a.name for a in n.names] if isinstance(n, ast.Import) else [n.module or ""]
                if any(x == "oracle" or x.startswith("oracle.") for x in names):
                    found.add(fn.name)
    for n in tree.body:                                   # no module-level import either
        if isinstance(n, (ast.Import, ast.ImportFrom)):
            names = [a.name for a in n.names] if isinstance(n, ast.Import) else [n.module or ""]
            assert not any(x == "oracle" or x.startswith("oracle.") for x in names)
    assert found and found <= allowed, found
