"""ctypes binding of libtsg_hip.so (C-ABI in include/tsg_hip.h).

The header is the only place a signature is written: `_PROTOS` is parsed from it at import, so a new entry point needs
a declaration there and nothing here.  What is still mirrored by hand (`OhemPlan`, `_ERR`, the enum constants) is
pinned to the header by tests/test_abi.py.

There is deliberately NO fallback: if the shared library is missing or a call
returns non-zero, the caller gets an exception.  The product path never routes
around the HIP kernels.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtsg_hip.so")

F32, BF16 = 0, 1
NCHW, NHWC = 0, 1
I64, U8 = 0, 1

_ERR = {-1: "unsupported dtype", -2: "unsupported layout", -3: "bad shape",
        -4: "misaligned pointer", -5: "null pointer", -6: "workspace too small",
        -7: "librccl.so could not be loaded"}


class TsgError(RuntimeError):
    pass


class OhemPlan(C.Structure):
    _fields_ = [("P", C.c_int64), ("C", C.c_int), ("grid", C.c_int), ("levels", C.c_int),
                ("shift", C.c_int * 3), ("bins", C.c_int * 3), ("thresh_bits", C.c_uint32),
                ("ws_bytes", C.c_size_t)]


_HEADER = os.path.join(_HERE, "..", "include", "tsg_hip.h")

# The closed type map of the C-ABI.  By value: exactly these spellings.  Pointers, ONE rule: every pointer parameter is
# c_void_p (it takes None, an integer address, byref(...) and ctypes pointers alike), except `const char*`, which is
# c_char_p as a parameter and as a return type.  Anything else is an error, never a default.
_VALUES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_DECL = re.compile(r"(.+?)\b(tsg_\w+)\s*\(([^()]*)\)", re.S)


def _ctype(spelling, decl, named):
    """ctypes type of a return type (named = False) or of a parameter, whose last word is its name"""
    t = " ".join(spelling.replace("*", " * ").split())
    if "*" in t:
        if named:
            t = t.rsplit("*", 1)[0] + "*"
        return C.c_char_p if t == "const char *" else C.c_void_p
    if named and " " in t:
        t = t.rsplit(" ", 1)[0]
    if t not in _VALUES:
        raise TsgError(f"C-ABI header: no ctypes mapping for '{spelling.strip()}' in `{' '.join(decl.split())}`")
    return _VALUES[t]


def _parse_protos(text):
    """name -> (restype, argtypes) of every `RET tsg_name(ARGS);` declaration of a C header"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
    protos = {}
    for decl in text.split(";"):
        if "(" not in decl:
            continue            # enums, the fields of a struct, typedefs
        m = _DECL.fullmatch(decl.strip())
        if m is None:
            raise TsgError(f"C-ABI header: cannot read `{' '.join(decl.split())}`")
        ret, name, args = m.groups()
        args = [] if args.strip() in ("", "void") else args.split(",")
        protos[name] = (_ctype(ret, decl, False), [_ctype(a, decl, True) for a in args])
    return protos


with open(_HEADER) as _f:
    _PROTOS = _parse_protos(_f.read())

_lib = None


def lib():
    """Return the loaded CDLL; raise if libtsg_hip.so has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TsgError(
                f"{LIB_PATH} not found: build it with `python -m torchseg_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU/eager fallback.")
        # torch FIRST: its wheel bundles its own libamdhip64.so; libtsg_hip.so is linked against /opt/rocm's.  With torch's
        # runtime already in the process ours resolves to it (same SONAME) and kernels, streams and pointers belong to
        # ONE HIP runtime; loaded the other way round (`python __graft_entry__.py --smoke`: build() before torch) every
        # launch on a torch stream came back hipErrorNoDevice (round 5)
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(handle, name)  # AttributeError if the .so is stale
            fn.restype = res
            fn.argtypes = args
        if handle.tsg_version() < 100:
            raise TsgError("libtsg_hip.so is older than this package")
        _lib = handle
    return _lib


def check(rc, what):
    if rc == 0:
        return
    if rc <= -100:
        raise TsgError(f"{what}: RCCL error {-100 - rc} ({lib().tsg_comm_error_string(rc).decode()})")
    if rc < 0:
        raise TsgError(f"{what}: invalid argument ({_ERR.get(rc, rc)})")
    raise TsgError(f"{what}: hipError_t {rc}")


def call(fn, *args):
    """fn(*args) for an entry point whose int result is a status: non-zero raises, named after the entry point called"""
    rc = fn(*args)
    if rc:
        check(rc, fn.__name__)


def ptr(t):
    """Device (or host) address of a tensor, None -> NULL."""
    return None if t is None else t.data_ptr()


def dtype_code(t):
    import torch
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TsgError(f"unsupported activation dtype {t.dtype} (float32 / bfloat16 only)")


_raw_stream = None


def stream_ptr(t):
    """hipStream_t of torch's current stream on the tensor's device (also right under
    stream contexts and hipGraph capture).  Uses torch's raw-stream getter: this runs
    ~1200 times per training step."""
    global _raw_stream
    if not t.is_cuda:
        raise TsgError("torchseg_amd kernels need tensors on an AMD GPU (got a CPU tensor); "
                       "there is no CPU fallback in the product path")
    if _raw_stream is None:
        import torch
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (
            lambda idx: torch.cuda.current_stream(idx).cuda_stream)
    return _raw_stream(t.device.index)
