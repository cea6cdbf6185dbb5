"""ctypes binding of libthinktwice_hip.so -- the ONLY compute backend.

There is deliberately no CPU or eager-PyTorch fallback: if the library is not
built, or a call fails, this raises.

The ABI is stated once, in include/thinktwice_hip.h.  `prototypes()` reads its declarations and `lib()` sets argtypes /
restype on every entry at load, so a call passes plain Python numbers, device pointers as ints (`ptr()`) and host arrays /
byref(struct) for host pointers; a wrong argument count or kind raises at the call.  The same table drives the plan thunks
(build.py) and the plan recorder (plan.py).  The data types too: `constants()` is every `#define TT_X <integer>` and
enumerator, `structs()` a ctypes.Structure per `typedef struct`, and the package's names for them (ops._ConvDesc,
control.ACT_STEER, ...) are bound to those at import, from the header alone: none is written out in Python.
"""
import collections
import ctypes
import functools
import keyword
import operator
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "thinktwice_hip.h")
LIB_PATH = os.path.join(_HERE, "libthinktwice_hip.so")
# experiments only (tools/): load an alternative build of the same ABI, e.g. one compiled with -DTT_GLDS_DEBUG=1
LIB_PATH = os.environ.get("TT_LIB_PATH", LIB_PATH)

_lib = None


class TTError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong,
            "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double,
            "const char*": ctypes.c_char_p, "unsigned char": ctypes.c_ubyte}

# one declaration of the header: C return type, [(C type, parameter name)], and their ctypes mirrors
Proto = collections.namedtuple("Proto", "ret params restype argtypes")


def _ctype(t, name):
    t = re.sub(r"\s*\*", "*", t)
    if t in _SCALARS:
        return _SCALARS[t]
    if t.endswith("*"):
        return ctypes.c_void_p
    raise TTError(f"thinktwice_hip.h: `{t}` in the declaration of {name} has no ctypes type")


def _source(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def prototypes(path=HEADER):
    """{name: Proto} of every `ret tt_name(params);` declaration of the header, in header order."""
    src = _source(path)
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


def _int(expr, consts, where):
    try:
        return operator.index(eval(expr, {"__builtins__": {}}, dict(consts)))
    except Exception:
        raise TTError(f"thinktwice_hip.h: `{expr}` of {where} is not a constant integer expression") from None


@functools.lru_cache(maxsize=None)
def constants(path=HEADER):
    """{name: int} of every `#define TT_NAME <integer>` and every enumerator of the header."""
    src = _source(path)
    out = {n: int(v, 0) for n, v in re.findall(r"^\s*#\s*define\s+(TT_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*$", src, flags=re.M)}
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", src):
        nxt = 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, val = (p.strip() for p in item.partition("="))
            out[name] = nxt = _int(val, out, "enumerator " + name) if val else nxt
            nxt += 1
    return out


@functools.lru_cache(maxsize=None)
def structs(path=HEADER):
    """{name: ctypes.Structure subclass} of every `typedef struct name { ... } name;`, in header order.  Pointer members are
    c_void_p, dimensions are evaluated over `constants()`, a Python keyword gets an underscore (`in_`); else TTError."""
    consts, out = constants(path), {}
    for name, body, alias in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w*)\s*;", _source(path), flags=re.S):
        if alias != name:       # a nested struct / union ends the match at ITS `}`: alias is then that member's name
            raise TTError(f"thinktwice_hip.h: struct {name}: `}} {alias};` closes a nested struct / union: no ctypes mapping")
        fields = []
        for stmt in filter(None, (" ".join(s.split()) for s in body.split(";"))):
            # `type declarator, ...`: a declarator is `*`s, a name and dimensions -- a bit-field or a function pointer is none
            decls = [re.fullmatch(r"([\w\s*]*?)([A-Za-z_]\w*)((?:\s*\[[^\]]*\])*)", d.strip()) for d in stmt.split(",")]
            if None in decls:
                raise TTError(f"thinktwice_hip.h: struct {name}: member `{stmt}` has no ctypes mapping")
            base = re.sub(r"^const ", "", decls[0].group(1).replace("*", " ").strip())
            for stars, member, dims in (d.groups() for d in decls):
                ct = ctypes.c_void_p if "*" in stars else out.get(base) or _ctype(base, f"struct {name}, member {member}")
                for d in reversed(re.findall(r"\[([^\]]*)\]", dims)):
                    ct = ct * _int(d, consts, f"struct {name}, member {member}")
                fields.append((member + "_" if keyword.iskeyword(member) else member, ct))
        out[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    return out


# every constant under its header name (TT_F32, TT_IDA_MAX_SETS, ...), but the activation codes and the slots of
# tt_action_post's `out` without the prefix, as the package spells them (ACT_RELU, ACT_STEER, ..., ACTION_OUT)
globals().update({k[3:] if k.startswith("TT_ACT") else k: v for k, v in constants().items()})


def takes_stream(name, params):
    """An asynchronous entry a launch plan records and replays: last parameter `void* stream`, not the plan API itself."""
    return (bool(params) and params[-1] == ("void*", "stream") and not name.startswith("tt_plan")
            and name not in ("tt_encoder_fwd", "tt_decoder_fwd"))


def load(path):
    """A build of the C-ABI library at `path`, every declared entry typed; raise loudly if it is missing or stale.  The package
    uses lib(); a tool that sets two builds side by side (tools/file_encode_ab.py) loads the other one here."""
    if not os.path.exists(path):
        raise TTError(
            f"{path} is missing: run `python -m thinktwice_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no fallback path.")
    so = ctypes.CDLL(path)
    missing = []
    for name, p in prototypes().items():
        try:
            f = getattr(so, name)
        except AttributeError:
            missing.append(name)
            continue
        f.restype, f.argtypes = p.restype, p.argtypes
    if missing:
        raise TTError(f"{path} does not export {', '.join(missing)} declared in include/thinktwice_hip.h: "
                      "rebuild it (`python -m thinktwice_amd.build`)")
    return so


def lib():
    """Load (once) and return the C-ABI library, every declared entry typed."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
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
