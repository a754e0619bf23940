"""ctypes binding of csrc/libcnrma_hip.so.  The binding IS the C-ABI's header: the signatures and the integer constants are read
from include/cnrma.h once, at import (_read_header); nothing here restates a prototype or a #define.
The product path has NO fallback: if the header or the library is missing or a symbol is absent this module raises.

Two libraries are built from the same sources: libcnrma_hip.so (the product: shipped kernels only, no cnrma_debug_* entry point,
no tuning state) and libcnrma_hip_exp.so (-DCNRMA_EXPERIMENTS: + the measured-and-rejected kernel forms behind
cnrma_debug_conv_tuning / cnrma_debug_dense_tuning).  Product code only ever sees the first; `experiments(True)` -- called by
sparse.conv_tuning(...) / rma.dense_tuning(...) with arguments, i.e. by scripts/ and by the bit-identity tests -- routes this
process's calls through the second until `experiments(False)`.
"""
import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libcnrma_hip.so")
EXP_LIB_PATH = os.path.join(_HERE, "csrc", "libcnrma_hip_exp.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cnrma.h")
# the data-preparation surface: a library and a header of their own (include/cnrma_prep.h), bound the same way
PREP_LIB_PATH = os.path.join(_HERE, "csrc", "libcnrma_prep_hip.so")
PREP_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cnrma_prep.h")
# the evaluation surface (indoor mAP of the detections): include/cnrma_eval.h and its own library, bound the same way
EVAL_LIB_PATH = os.path.join(_HERE, "csrc", "libcnrma_eval_hip.so")
EVAL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cnrma_eval.h")
# the reconstruction-head surface (TSDF regression, fill, loss, backward): include/cnrma_recon.h and its own library, bound the same way
RECON_LIB_PATH = os.path.join(_HERE, "csrc", "libcnrma_recon_hip.so")
RECON_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cnrma_recon.h")
# the 3D U-Net surface (dense 3x3x3 convolutions in f16x3): include/cnrma_unet.h and its own library, bound the same way
UNET_LIB_PATH = os.path.join(_HERE, "csrc", "libcnrma_unet_hip.so")
UNET_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cnrma_unet.h")
# the 3D U-Net decoder joints (up-sampling, 1x1x1 convolutions, conditional skip and mean in one pass): include/cnrma_unet_join.h and
# its own library, bound the same way
UNET_JOIN_LIB_PATH = os.path.join(_HERE, "csrc", "libcnrma_unetjoin_hip.so")
UNET_JOIN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cnrma_unet_join.h")
# the header's whole vocabulary: a parameter whose text holds a `*` is a pointer, the scalars by name.  A new one is a line here
_CTYPES = {"*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32}


class CnrmaError(RuntimeError):
    pass


def _read_header(text):
    """(prototypes, experiment_prototypes, constants) of include/cnrma.h's text: name -> (restype, [argtypes]) of every
    `int|size_t cnrma_<name>(...);` outside / inside the `#ifdef CNRMA_EXPERIMENTS ... #endif` blocks, name -> int of every
    `#define CNRMA_X <int>`.  What it does not know raises: there is no fallback type"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)       # comments quote prototypes and trail the defines
    text = text.replace("\\\n", " ")                                # a function-like macro's lines: one #define, not a constant
    bodies, tables, constants, in_exp = ([], []), ({}, {}), {}, False
    for line in text.split("\n"):
        directive = re.match(r"\s*#\s*(\w+)", line)
        if directive is None:
            bodies[in_exp].append(line)
        elif directive.group(1) in ("if", "ifdef", "ifndef", "elif", "else"):
            if in_exp:                                                # blocks are flat: their first #endif is their own
                raise CnrmaError(f"cnrma.h: a conditional nested in an #ifdef CNRMA_EXPERIMENTS block: {line.strip()!r}")
            in_exp = line.split() == ["#ifdef", "CNRMA_EXPERIMENTS"]
        elif directive.group(1) == "endif":
            in_exp = False
        elif m := re.fullmatch(r"\s*#\s*define\s+(CNRMA_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*", line):
            constants[m.group(1)] = int(m.group(2))
    for table, body in zip(tables, bodies):
        for ret, name, params in re.findall(r"(\w+)\s+(cnrma_\w+)\s*\(([^;()]*)\)\s*;", "\n".join(body)):
            if ret not in ("int", "size_t") or name in tables[0] or name in tables[1]:
                raise CnrmaError(f"cnrma.h: {name} is declared twice or returns {ret!r}, neither int nor size_t")
            table[name] = (_CTYPES[ret], [])
            for param in ([] if params.strip() in ("", "void") else params.split(",")):
                ctype = "*" if "*" in param else " ".join(w for w in param.split()[:-1] if w != "const")     # [:-1]: its name
                if ctype not in _CTYPES:
                    raise CnrmaError(f"cnrma.h: {name}: no ctypes type for the parameter {' '.join(param.split())!r}")
                table[name][1].append(_CTYPES[ctype])
    return tables[0], tables[1], constants


try:        # name -> (restype, argtypes) in header order: the product surface, and what libcnrma_hip_exp.so exports on top of it
    with open(HEADER_PATH) as _f:
        SIGNATURES, EXPERIMENT_SIGNATURES, CONSTANTS = _read_header(_f.read())
except OSError as e:
    raise CnrmaError(f"cannot read the C-ABI header {HEADER_PATH}: {e}") from e
ABI_VERSION, EINVAL = CONSTANTS["CNRMA_ABI_VERSION"], CONSTANTS["CNRMA_EINVAL"]
try:
    with open(PREP_HEADER_PATH) as _f:
        PREP_SIGNATURES, _prep_exp, PREP_CONSTANTS = _read_header(_f.read())
except OSError as e:
    raise CnrmaError(f"cannot read the C-ABI header {PREP_HEADER_PATH}: {e}") from e
if _prep_exp:
    raise CnrmaError(f"cnrma_prep.h declares experiment entry points ({sorted(_prep_exp)}): the preparation library has none")
PREP_ABI_VERSION = PREP_CONSTANTS["CNRMA_PREP_ABI_VERSION"]
try:
    with open(EVAL_HEADER_PATH) as _f:
        EVAL_SIGNATURES, _eval_exp, EVAL_CONSTANTS = _read_header(_f.read())
except OSError as e:
    raise CnrmaError(f"cannot read the C-ABI header {EVAL_HEADER_PATH}: {e}") from e
if _eval_exp:
    raise CnrmaError(f"cnrma_eval.h declares experiment entry points ({sorted(_eval_exp)}): the evaluation library has none")
EVAL_ABI_VERSION = EVAL_CONSTANTS["CNRMA_EVAL_ABI_VERSION"]
try:
    with open(RECON_HEADER_PATH) as _f:
        RECON_SIGNATURES, _recon_exp, RECON_CONSTANTS = _read_header(_f.read())
except OSError as e:
    raise CnrmaError(f"cannot read the C-ABI header {RECON_HEADER_PATH}: {e}") from e
if _recon_exp:
    raise CnrmaError(f"cnrma_recon.h declares experiment entry points ({sorted(_recon_exp)}): the reconstruction library has none")
RECON_ABI_VERSION = RECON_CONSTANTS["CNRMA_RECON_ABI_VERSION"]
try:
    with open(UNET_HEADER_PATH) as _f:
        UNET_SIGNATURES, _unet_exp, UNET_CONSTANTS = _read_header(_f.read())
except OSError as e:
    raise CnrmaError(f"cannot read the C-ABI header {UNET_HEADER_PATH}: {e}") from e
if _unet_exp:
    raise CnrmaError(f"cnrma_unet.h declares experiment entry points ({sorted(_unet_exp)}): the 3D U-Net library has none")
UNET_ABI_VERSION = UNET_CONSTANTS["CNRMA_UNET_ABI_VERSION"]
try:
    with open(UNET_JOIN_HEADER_PATH) as _f:
        UNET_JOIN_SIGNATURES, _unet_join_exp, UNET_JOIN_CONSTANTS = _read_header(_f.read())
except OSError as e:
    raise CnrmaError(f"cannot read the C-ABI header {UNET_JOIN_HEADER_PATH}: {e}") from e
if _unet_join_exp:
    raise CnrmaError(f"cnrma_unet_join.h declares experiment entry points ({sorted(_unet_join_exp)}): the joint library has none")
UNET_JOIN_ABI_VERSION = UNET_JOIN_CONSTANTS["CNRMA_UNET_JOIN_ABI_VERSION"]

_libs = {}            # False: product library, True: experiments library
_active = False       # which of the two load() / call() use
_exp_users = set()    # who asked for the experiments library ("conv", "dense", a test): product again when nobody is left


def load(experiments=None):
    """The library this process's calls go to, loaded once; raises loudly when it is not built (no CPU fallback exists).
    experiments: None = the active one (the product library unless experiments(True) was called), False / True = that one."""
    which = _active if experiments is None else bool(experiments)
    lib = _libs.get(which)
    if lib is not None:
        return lib
    path = EXP_LIB_PATH if which else LIB_PATH
    if not os.path.exists(path):
        raise CnrmaError(f"{path} not found: build it with `python __graft_entry__.py build` "
                         f"(or `make -C cn-rma_amd/csrc`). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(path)
    table = dict(SIGNATURES, **EXPERIMENT_SIGNATURES) if which else SIGNATURES
    for name, (res, args) in table.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.cnrma_abi_version() != ABI_VERSION:
        raise CnrmaError("ABI version mismatch")
    _libs[which] = lib
    return lib


_prep_lib = None


def load_prep():
    """libcnrma_prep_hip.so (include/cnrma_prep.h), loaded once; raises loudly when it is not built"""
    global _prep_lib
    if _prep_lib is not None:
        return _prep_lib
    if not os.path.exists(PREP_LIB_PATH):
        raise CnrmaError(f"{PREP_LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                         f"(or `make -C cn-rma_amd/csrc`). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(PREP_LIB_PATH)
    for name, (res, args) in PREP_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.cnrma_prep_abi_version() != PREP_ABI_VERSION:
        raise CnrmaError("ABI version mismatch (libcnrma_prep_hip.so)")
    _prep_lib = lib
    return lib


def call_prep(name, *args):
    rc = getattr(load_prep(), name)(*args)
    if rc != 0:
        raise CnrmaError(f"{name} failed with code {rc}" + (" (invalid argument)" if rc == PREP_CONSTANTS["CNRMA_PREP_EINVAL"]
                                                          else " (-hipError_t)"))
    return rc


_eval_lib = None


def load_eval():
    """libcnrma_eval_hip.so (include/cnrma_eval.h), loaded once; raises loudly when it is not built"""
    global _eval_lib
    if _eval_lib is not None:
        return _eval_lib
    if not os.path.exists(EVAL_LIB_PATH):
        raise CnrmaError(f"{EVAL_LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                         f"(or `make -C cn-rma_amd/csrc`). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(EVAL_LIB_PATH)
    for name, (res, args) in EVAL_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.cnrma_eval_abi_version() != EVAL_ABI_VERSION:
        raise CnrmaError("ABI version mismatch (libcnrma_eval_hip.so)")
    _eval_lib = lib
    return lib


def call_eval(name, *args):
    rc = getattr(load_eval(), name)(*args)
    if rc != 0:
        raise CnrmaError(f"{name} failed with code {rc}" + (" (invalid argument)" if rc == EVAL_CONSTANTS["CNRMA_EVAL_EINVAL"]
                                                          else " (-hipError_t)"))
    return rc


_recon_lib = None


def load_recon():
    """libcnrma_recon_hip.so (include/cnrma_recon.h), loaded once; raises loudly when it is not built"""
    global _recon_lib
    if _recon_lib is not None:
        return _recon_lib
    if not os.path.exists(RECON_LIB_PATH):
        raise CnrmaError(f"{RECON_LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                         f"(or `make -C cn-rma_amd/csrc`). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(RECON_LIB_PATH)
    for name, (res, args) in RECON_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.cnrma_recon_abi_version() != RECON_ABI_VERSION:
        raise CnrmaError("ABI version mismatch (libcnrma_recon_hip.so)")
    _recon_lib = lib
    return lib


def call_recon(name, *args):
    rc = getattr(load_recon(), name)(*args)
    if rc != 0:
        raise CnrmaError(f"{name} failed with code {rc}" + (" (invalid argument)" if rc == RECON_CONSTANTS["CNRMA_RECON_EINVAL"]
                                                          else " (-hipError_t)"))
    return rc


_unet_lib = None


def load_unet():
    """libcnrma_unet_hip.so (include/cnrma_unet.h), loaded once; raises loudly when it is not built"""
    global _unet_lib
    if _unet_lib is not None:
        return _unet_lib
    if not os.path.exists(UNET_LIB_PATH):
        raise CnrmaError(f"{UNET_LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                         f"(or `make -C cn-rma_amd/csrc`). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(UNET_LIB_PATH)
    for name, (res, args) in UNET_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.cnrma_unet_abi_version() != UNET_ABI_VERSION:
        raise CnrmaError("ABI version mismatch (libcnrma_unet_hip.so)")
    _unet_lib = lib
    return lib


def call_unet(name, *args):
    rc = getattr(load_unet(), name)(*args)
    if rc != 0:
        raise CnrmaError(f"{name} failed with code {rc}" + (" (invalid argument)" if rc == UNET_CONSTANTS["CNRMA_UNET_EINVAL"]
                                                          else " (-hipError_t)"))
    return rc


_unet_join_lib = None


def load_unet_join():
    """libcnrma_unetjoin_hip.so (include/cnrma_unet_join.h), loaded once; raises loudly when it is not built"""
    global _unet_join_lib
    if _unet_join_lib is not None:
        return _unet_join_lib
    if not os.path.exists(UNET_JOIN_LIB_PATH):
        raise CnrmaError(f"{UNET_JOIN_LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                         f"(or `make -C cn-rma_amd/csrc`). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(UNET_JOIN_LIB_PATH)
    for name, (res, args) in UNET_JOIN_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.cnrma_unet_join_abi_version() != UNET_JOIN_ABI_VERSION:
        raise CnrmaError("ABI version mismatch (libcnrma_unetjoin_hip.so)")
    _unet_join_lib = lib
    return lib


def call_unet_join(name, *args):
    rc = getattr(load_unet_join(), name)(*args)
    if rc != 0:
        raise CnrmaError(f"{name} failed with code {rc}" + (" (invalid argument)"
                                                          if rc == UNET_JOIN_CONSTANTS["CNRMA_UNET_JOIN_EINVAL"] else " (-hipError_t)"))
    return rc


def experiments(on=True, who="caller"):
    """route this process's C-ABI calls through libcnrma_hip_exp.so (True) or back through the product library (False, once
    every `who` that asked for it has let go).  The two libraries are the same sources; the experiments one adds kernels and the
    cnrma_debug_* switches.  Never called by product code."""
    global _active
    if on:
        load(True)
        _exp_users.add(who)
    else:
        _exp_users.discard(who)
    _active = bool(_exp_users)


def experiments_active():
    return _active


def ptr(t):
    """device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "C-ABI buffers must be contiguous"
    if not t.is_cuda:                    # a host pointer handed to a kernel is a GPU memory fault, not an exception
        raise CnrmaError(f"C-ABI buffers must live on the GPU (got a {t.device} tensor of shape {tuple(t.shape)}): "
                         "move the module / tensor with .to(device) first")
    return t.data_ptr()


def stream():
    """raw hipStream_t of torch's current stream on the current device (fast path: no Stream object is built)"""
    import torch
    try:
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    except AttributeError:
        return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise CnrmaError(f"{name} failed with code {rc}" + (" (invalid argument)" if rc == EINVAL else " (-hipError_t)"))
    return rc


def scratch(query_name, *args, device, dtype=None):
    """a fresh buffer of as many bytes as the library's `query_name(*args)` asks for (uint8; another dtype: that many bytes in
    whole elements).  Never cached: the allocator's stream ordering is what makes reuse of the block safe"""
    import torch
    nbytes = getattr(load(), query_name)(*args)
    if dtype is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    return torch.empty(nbytes // dtype.itemsize, dtype=dtype, device=device)


LRU_STREAMS = 12      # entries a stream-keyed table keeps by default: the streams of a process come and go (every scene slot / detector
                      # has its own), their raw handles are all such a table knows of them -- the least recently used entries are
                      # dropped (round 6: ~1 GB per detector ever built stayed allocated).  Dropping is safe: the caching allocator
                      # hands a freed block back to the stream it was allocated on, in stream order.
LRU_LOCK = threading.RLock()      # the tables are module-wide; several host threads (one per scene slot) reach them


def lru_get(table, key, make, limit=LRU_STREAMS):
    """table[key] (moved to the most-recent end), created by make() when absent; the oldest entries beyond `limit` are dropped"""
    with LRU_LOCK:
        buf = table.pop(key, None)
        if buf is None:
            buf = make()
        table[key] = buf
        while len(table) > limit:
            table.pop(next(iter(table)))
        return buf


_tls = threading.local()


def read_ints(t):
    """device int tensor -> list of host ints, as an asynchronous copy into this thread's pinned buffer followed by a
    wait on the CURRENT stream only.  (Tensor.item()/.tolist() issue a blocking hipMemcpy into pageable memory, during
    which other host threads' launches stall: with several scenes in flight that drained the whole GPU at every
    read-back.)"""
    import torch
    t = t.reshape(-1)
    n = t.numel()
    buf = getattr(_tls, "pinned", None)
    if buf is None or buf.numel() < n or buf.dtype != t.dtype:
        buf = torch.empty(max(64, n), dtype=t.dtype, pin_memory=True)
        _tls.pinned = buf
    buf[:n].copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return buf[:n].tolist()


_gpu_ok = False


def require_gpu():
    global _gpu_ok
    if _gpu_ok:
        return
    import torch
    if not torch.cuda.is_available():
        raise CnrmaError("cn-rma_amd needs a HIP device (MI355X); the product path has no CPU implementation")
    _gpu_ok = True
