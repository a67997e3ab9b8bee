"""CPU: the C-ABI library loads and exports every symbol include/tsg_hip.h declares,
and the ctypes prototype table covers exactly that set (no compute calls)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "tsg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(tsg_[a-z0-9_]+)\s*\(", src))


def test_library_exports_every_declared_symbol():
    from torchseg_amd import _lib, build
    build.build()
    names = _declared()
    assert len(names) >= 20
    h = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in names if not hasattr(h, n)]
    assert not missing, missing
    assert set(_lib._PROTOS) == names
    assert _lib.lib().tsg_version() >= 100


def test_argument_validation_without_gpu():
    from torchseg_amd import _lib
    lib = _lib.lib()
    assert lib.tsg_bn_num_partials(_lib.NCHW, 16, 64, 512 * 512) >= 1
    assert lib.tsg_bn_num_partials(_lib.NHWC, 0, 64, 4) < 0
    plan = _lib.OhemPlan()
    assert lib.tsg_ohem_make_plan(16, 19, 1024 * 1024, 0.7, ctypes.byref(plan)) == 0
    assert plan.P == 16 * 1024 * 1024 and plan.levels == 2 and plan.bins[0] == 1229 and plan.bins[1] == 4096
    assert plan.ws_bytes > 0
    assert lib.tsg_ohem_make_plan(0, 19, 4, 0.7, ctypes.byref(plan)) < 0
    # NULL pointers are rejected before any launch
    assert lib.tsg_bn_stats(None, 0, 0, 1, 1, 1, None, None, None) < 0
    assert lib.tsg_sgd_step(None, None, None, 4, 0.1, 0.9, 0.0, 1.0, 1, None) < 0
    # host-side helpers of the multi-tensor SGD and the stem convolution
    import numpy as np
    n = np.array([1, 4096, 4097, 10000], dtype=np.int64)
    nb = lib.tsg_sgd_multi_blockmap(n.ctypes.data, 4, None, 0)
    m = np.empty((nb, 2), np.int32)
    assert nb == 7 and lib.tsg_sgd_multi_blockmap(n.ctypes.data, 4, m.ctypes.data, nb) == 7
    assert m.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [3, 0], [3, 1], [3, 2]]
    assert lib.tsg_sgd_multi_blockmap(n.ctypes.data, 129, None, 0) < 0
    assert lib.tsg_stem_conv_supported(_lib.BF16, 3, 64, 7, 7, 2, 3, 1, 1, 1024, 1024) == 1
    assert lib.tsg_stem_conv_supported(_lib.F32, 3, 64, 7, 7, 2, 3, 1, 1, 1024, 1024) == 0
    assert lib.tsg_stem_conv_supported(_lib.BF16, 3, 64, 3, 3, 2, 1, 1, 1, 1024, 1024) == 0
    assert lib.tsg_stem_conv_ws_bytes() > 64 * 176 * 2
    assert lib.tsg_stem_conv_fwd(None, None, None, 1, 8, 8, None, 0, None) < 0


def test_product_path_refuses_cpu_tensors():
    import pytest
    import torch
    from torchseg_amd.losses import ProbOhemCrossEntropy2d
    from torchseg_amd.syncbn import SyncBatchNorm
    with pytest.raises(Exception):
        SyncBatchNorm(4)(torch.randn(2, 4, 3, 3))
    with pytest.raises(Exception):
        ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=1)(torch.randn(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))


def test_comm_entry_points_without_gpu():
    """tsg_comm_*: librccl resolves at run time, argument validation happens before any RCCL call, and RCCL failures
    come back in their own error range with RCCL's message (no GPU here: no communicator can exist)."""
    import torch  # noqa: F401  (puts the framework's librccl.so into the process, the copy the library must reuse)
    from torchseg_amd import _lib
    lib = _lib.lib()
    assert lib.tsg_comm_init_library(None) == 0
    assert lib.tsg_comm_unique_id_bytes() == 128
    assert lib.tsg_comm_xgmi_handle_bytes() == 64
    assert lib.tsg_comm_get_unique_id(None) == -5
    h = ctypes.c_void_p()
    assert lib.tsg_comm_create(None, 0, 0, 0, ctypes.byref(h)) == -3          # world < 1
    assert lib.tsg_comm_create(None, 2, 2, 0, ctypes.byref(h)) == -3          # rank >= world
    assert lib.tsg_comm_allreduce(None, None, 4, 0, None) == -5
    assert lib.tsg_comm_allgather(None, None, None, 4, 0, None) == -5
    assert lib.tsg_comm_broadcast(None, None, 4, 0, 0, None) == -5
    assert lib.tsg_xgmi_small_allreduce(None, None, 4, None) == -5
    assert b"librccl" in lib.tsg_comm_error_string(-7)
    if not torch.cuda.is_available():
        buf = ctypes.create_string_buffer(128)
        rc = lib.tsg_comm_get_unique_id(buf)        # RCCL builds differ: some hand out an id without a device
        assert rc == 0 or rc <= -100
        if rc:
            import pytest
            assert len(lib.tsg_comm_error_string(rc)) > 0
            with pytest.raises(_lib.TsgError, match="RCCL error"):
                _lib.check(rc, "tsg_comm_get_unique_id")
        else:
            assert any(buf.raw)


# ---- torchseg_amd/_lib.py against the header: the parser that derives _PROTOS, and the few mirrors still written by hand ----

def _header():
    src = open(os.path.join(ROOT, "include", "tsg_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_prototype_parser_on_hand_read_signatures():
    """expected (restype, argtypes) written down from the header by hand: together they cover int, int64_t, float, double
    and size_t by value, data / struct / handle / pointer-to-pointer parameters, and `const char*` both ways"""
    from torchseg_amd import _lib
    i, i64, f, d, sz, p, s = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
                              ctypes.c_void_p, ctypes.c_char_p)
    want = {
        "tsg_bn_finalize": (i, [p, i, i64, d, p, f, f, p, p, p, p, p, p, p, p, p]),
        "tsg_gap_fwd": (i, [p, p, i, i, i64, i64, i64, p, sz, p]),
        "tsg_bn_num_partials": (i, [i, i64, i64, i64]),
        "tsg_conv3x3_gen_filter_elems": (i64, [i, i]),
        "tsg_ohem_make_plan": (i, [i64, i, i64, f, p]),
        "tsg_comm_create": (i, [p, i, i, i, p]),
        "tsg_comm_error_string": (s, [i]),
        "tsg_comm_init_library": (i, [s]),
        "tsg_stem_conv_ws_bytes": (sz, []),
        "tsg_augment_crop": (i, [p, p, p, p, i, i, i, p, p, f, i, p, p, i, p]),
    }
    for name, proto in want.items():
        assert _lib._PROTOS[name] == proto, name


def test_prototype_arity_equals_the_header_for_every_entry_point():
    from torchseg_amd import _lib
    decls = re.findall(r"\b(tsg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header())
    assert len(decls) == len(_lib._PROTOS) >= 165
    for name, args in decls:
        n = 0 if args.strip() in ("", "void") else args.count(",") + 1
        assert len(_lib._PROTOS[name][1]) == n, name


def test_prototype_parser_refuses_what_it_does_not_know():
    import pytest
    from torchseg_amd import _lib
    parse = _lib._parse_protos
    assert parse("/* int tsg_a(int x); */\n#define TSG_Z (-1)\n// int tsg_b(int x);\nsize_t tsg_y(void);\nint tsg_w();") == {
        "tsg_y": (ctypes.c_size_t, []), "tsg_w": (ctypes.c_int, [])}
    assert parse("const char* tsg_s(const char *a, const void* const* b, long long* c, int64_t d);") == {
        "tsg_s": (ctypes.c_char_p, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64])}
    for bad in ("tsg_x(__int128 a);", "int tsg_x(__int128 a);", "int tsg_x(int a, unsigned b);", "int tsg_x(long a);",
                "unsigned tsg_x(int a);", "int tsg_x(void (*cb)(int));"):
        with pytest.raises(_lib.TsgError, match="tsg_x"):
            parse(bad)


def test_prototypes_need_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys; from torchseg_amd import _lib; "
            "assert len(_lib._PROTOS) >= 165 and _lib._lib is None and 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=60)


def test_ohem_plan_mirrors_the_header_struct():
    from torchseg_amd import _lib
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    body = re.search(r"typedef\s+struct\s+tsg_ohem_plan\s*\{(.*?)\}\s*tsg_ohem_plan\s*;", _header(), re.S).group(1)
    want = []
    for decl in filter(str.strip, body.split(";")):
        t, name, n = re.fullmatch(r"\s*(\w+)\s+(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", decl).groups()
        want.append((name, ctype[t], int(n) if n else None))
    got = [(name, t._type_, t._length_) if issubclass(t, ctypes.Array) else (name, t, None)
           for name, t in _lib.OhemPlan._fields_]
    assert len(want) == 8 and got == want


def test_error_codes_and_enums_mirror_the_header():
    import pytest
    from torchseg_amd import _lib
    src = _header()
    codes = {k: int(v) for k, v in re.findall(r"#define\s+TSG_E_(\w+)\s+\((-\d+)\)", src)}
    base = codes.pop("COMM_BASE")
    assert len(codes) >= 7 and set(_lib._ERR) == set(codes.values())
    for v in codes.values():
        with pytest.raises(_lib.TsgError, match=re.escape("invalid argument (%s)" % _lib._ERR[v])):
            _lib.check(v, "x")
    # check() hands a code to RCCL's message table from TSG_E_COMM_BASE downwards, and not before
    with pytest.raises(_lib.TsgError, match="RCCL error 0 "):
        _lib.check(base, "x")
    with pytest.raises(_lib.TsgError, match="RCCL error 3 "):
        _lib.check(base - 3, "x")
    with pytest.raises(_lib.TsgError, match="invalid argument"):
        _lib.check(base + 1, "x")
    enums = {k: int(v) for body in re.findall(r"enum\s*\{(.*?)\}", src, re.S) for k, v in re.findall(r"TSG_(\w+)\s*=\s*(\d+)", body)}
    assert enums == {"F32": _lib.F32, "BF16": _lib.BF16, "NCHW": _lib.NCHW, "NHWC": _lib.NHWC, "I64": _lib.I64, "U8": _lib.U8}


def test_call_raises_checks_error_named_after_the_entry_point():
    import pytest
    from torchseg_amd import _lib
    lib = _lib.lib()
    assert _lib.call(lib.tsg_comm_init_library, None) is None
    with pytest.raises(_lib.TsgError, match=re.escape("tsg_conv3x3_wrw_tr: invalid argument (null pointer)")):
        _lib.call(lib.tsg_conv3x3_wrw_tr, None, None, None, 1, 8, 8, None, 0, None)
    with pytest.raises(_lib.TsgError, match=re.escape("tsg_comm_create: invalid argument (bad shape)")):
        _lib.call(lib.tsg_comm_create, None, 0, 0, 0, ctypes.byref(ctypes.c_void_p()))
