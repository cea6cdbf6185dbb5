"""ctypes binding of libthinktwice_hip.so -- the ONLY compute backend.

There is deliberately no CPU or eager-PyTorch fallback: if the library is not
built, or a call fails, this raises.

The ABI is stated once, in include/thinktwice_hip.h.  `prototypes()` reads its
declarations and `lib()` sets argtypes / restype on every entry at load, so a
call passes plain Python numbers, device pointers as ints (`ptr()`) and host
arrays / byref(struct) for host pointers; a wrong argument count or kind raises
at the call.  The same table drives the plan thunks (build.py) and the plan
recorder (plan.py).
"""
import collections
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "thinktwice_hip.h")
LIB_PATH = os.path.join(_HERE, "libthinktwice_hip.so")
# experiments only (tools/): load an alternative build of the same ABI, e.g. one compiled with -DTT_GLDS_DEBUG=1
LIB_PATH = os.environ.get("TT_LIB_PATH", LIB_PATH)

TT_F32, TT_BF16, TT_F16 = 0, 1, 2
TT_IDA_MAX_SETS = 64     # parameter sets (samples x cameras) of one tt_preprocess_*_ida call
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_GELU, ACT_SOFTPLUS, ACT_SOFTPLUS_CLAMP = 0, 1, 2, 3, 4, 5

_lib = None


class TTError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong,
            "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double,
            "const char*": ctypes.c_char_p}

# one declaration of the header: C return type, [(C type, parameter name)], and their ctypes mirrors
Proto = collections.namedtuple("Proto", "ret params restype argtypes")


def _ctype(t, name):
    t = re.sub(r"\s*\*", "*", t)
    if t in _SCALARS:
        return _SCALARS[t]
    if t.endswith("*"):
        return ctypes.c_void_p
    raise TTError(f"thinktwice_hip.h: `{t}` in the declaration of {name} has no ctypes type")


def prototypes(path=HEADER):
    """{name: Proto} of every `ret tt_name(params);` declaration of the header, in header order."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\n\s*([A-Za-z_][\w ]*?\**)\s*(tt_\w+)\s*\(([^;{]*?)\)\s*;", src):
        params = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a in ("void", ""):
                continue
            m = re.match(r"(.*?)(\w+)$", a)
            params.append((m.group(1).strip(), m.group(2)))
        ret = ret.strip()
        out[name] = Proto(ret, params, None if ret == "void" else _ctype(ret, name), [_ctype(t, name) for t, _ in params])
    return out


def takes_stream(name, params):
    """An asynchronous entry a launch plan records and replays: last parameter `void* stream`, not the plan API itself."""
    return (bool(params) and params[-1] == ("void*", "stream") and not name.startswith("tt_plan")
            and name not in ("tt_encoder_fwd", "tt_decoder_fwd"))


def lib():
    """Load (once) and return the C-ABI library, every declared entry typed; raise loudly if it is missing or stale."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TTError(
                f"{LIB_PATH} is missing: run `python -m thinktwice_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no fallback path.")
        so = ctypes.CDLL(LIB_PATH)
        missing = []
        for name, p in prototypes().items():
            try:
                f = getattr(so, name)
            except AttributeError:
                missing.append(name)
                continue
            f.restype, f.argtypes = p.restype, p.argtypes
        if missing:
            raise TTError(f"{LIB_PATH} does not export {', '.join(missing)} declared in include/thinktwice_hip.h: "
                          "rebuild it (`python -m thinktwice_amd.build`)")
        _lib = so
    return _lib


def check(rc, what):
    if rc != 0:
        raise TTError(f"{what} failed (rc={rc}): {lib().tt_last_error().decode()}")


def ptr(t):
    """Device pointer of a torch tensor (None = NULL)."""
    return None if t is None else t.data_ptr()


def cur_stream(device=None):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise TTError("thinktwice_amd ops need device tensors (MI355X); got a CPU tensor. "
                          "There is no CPU path in the product -- see oracle/ for the checker.")


def device_faults():
    """Non-blocking read of the current device's host-mapped fault word (tt_device_faults): meaningful for work the caller
    has synchronised with."""
    return int(lib().tt_device_faults())


def clear_device_faults():
    check(lib().tt_clear_device_faults(), "tt_clear_device_faults")


def raise_on_device_fault(where):
    """The product's check: a barrier time-out of tt_mlp_chain_wide poisons its outputs with NaN and sets the fault word;
    whoever has just synchronised with the forward (or is about to start the next one) turns it into a TTError."""
    if device_faults() > 0:
        raise TTError(f"{where}: a tt_mlp_chain_wide barrier timed out on this device -- the decoder outputs since then are "
                      f"NaN / invalid (thinktwice_amd.ops.clear_device_faults() re-arms the device)")
