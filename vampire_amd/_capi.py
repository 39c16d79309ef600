"""ctypes binding of include/vampire_hip.h (the C-ABI HIP library), built from the header at import.

The header is the source: its constants, structures and prototypes (read by _header.py) become this module's VAMP_*
names, Vamp* classes and SIGNATURES.  A new entry point is declared there and nowhere else; what the header cannot
say -- which `int` returns are values -- is in the short table above SIGNATURES (_INT_VALUES).

There is deliberately no fallback: if the shared library is missing or a symbol
does not resolve, importing the ops raises.  The product path never routes
through oracle/ or any CPU implementation.
"""
import ctypes as C
import os
import types
import typing

# torch must bring in ITS libamdhip64 first: a second HIP runtime (the system copy this
# library would otherwise pull in) sees no device inside a torch process.
import torch

from . import _header
from .build import lib_path

_H = _header.read()

# every VAMP_* constant of the header (#defines and enumerators) under its own name
globals().update(_H.constants)
ABI_VERSION = _H.constants["VAMP_ABI_VERSION"]     # load() holds the library's vamp_abi_version() against it: a stale .so


def _regions(prefix):
    """The workspace regions an enum of the header names, in layout order: VAMP_LIFTWS_FEAT_CL -> "feat_cl"."""
    names = [n for n in _H.constants if n.startswith(prefix) and n != prefix + "REGIONS"]
    assert [_H.constants[n] for n in names] == list(range(_H.constants[prefix + "REGIONS"])), prefix
    return tuple(n[len(prefix):].lower() for n in names)


RENDERWS_REGIONS = _regions("VAMP_RENDERWS_")      # ("grad" overlays "gcl" .. "beta_part")
LIFTWS_REGIONS = _regions("VAMP_LIFTWS_")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float,
            "double": C.c_double, "const char*": C.c_char_p}


def _field_type(ctype, dims):
    t = C.c_void_p if ctype.endswith("*") else globals()[ctype] if ctype in _H.structs else _SCALARS[ctype]
    for n in reversed(dims):
        t = t * n
    return t


# the Vamp* structures, fields in header order; a pointer field is a c_void_p
for _name, _fields in _H.structs.items():
    globals()[_name] = type(_name, (C.Structure,), {
        "_fields_": [(f, _field_type(t, dims)) for f, t, dims in _fields],
        "__doc__": f"{_name} of include/vampire_hip.h, where its fields are described."})


_Tensor, _void_p = torch.Tensor, C.c_void_p       # (module globals: from_param runs once per pointer argument of every call)


class TensorPtr(C.c_void_p):
    """`void*` parameter of the signature table: takes a torch tensor (its data_ptr()), None (NULL), an integer address
    or anything c_void_p itself takes (a c_void_p, a ctypes array or pointer).  Contiguity, device and shape are the
    caller's business (ops `_chk`): this type converts, it does not validate."""

    @classmethod
    def from_param(cls, obj):
        if isinstance(obj, _Tensor):
            # a c_void_p, never the bare integer: ctypes passes an int that from_param returns as a 32-bit C int
            return _void_p(obj.data_ptr())
        if obj is None:
            return None
        if isinstance(obj, int):
            return _void_p(obj)
        if isinstance(obj, (str, bytes)):         # (c_void_p would take the characters' address)
            raise TypeError(f"expected a tensor or a pointer, got {type(obj).__name__}")
        return _void_p.from_param(obj)


class _Ret(typing.NamedTuple):
    """What an entry point returns: its ctypes type, and whether that is a VampStatus code (VAMP_OK or negative), which
    the checked set turns into an exception, or a value handed to the caller as it is."""
    ctype: type
    is_status: bool


_STATUS = _Ret(C.c_int, True)
_INT, _SIZE, _STR = _Ret(C.c_int, False), _Ret(C.c_size_t, False), _Ret(C.c_char_p, False)

# ---- what the header cannot say ----------------------------------------------------------------------------------------
# `int` returns that are a value, not a VampStatus code (besides every `*_supported`, which answers 0 or 1)
_INT_VALUES = ("vamp_abi_version", "vamp_profile_slots")


def _argtype(function, ctype, name):
    """A scalar by its type; a `Vamp*` pointer as POINTER(structure), so that a bare instance goes by reference; a
    scalar pointer whose name ends in _host (the header's mark of host memory) as POINTER(scalar); every other pointer,
    array parameters included, as TensorPtr.  Every parameter of the header falls under these rules today; one that
    did not would get an entry in a (function, parameter) table consulted first here, with its reason."""
    if ctype in _SCALARS:
        return _SCALARS[ctype]
    if not ctype.endswith("*"):
        raise TypeError(f"{function}({name}): no ctypes type for {ctype!r}")
    pointee = ctype[:-1] if ctype[:-1] in _SCALARS else ctype[:-1].removeprefix("const ")
    if pointee in _H.structs:
        return C.POINTER(globals()[pointee])
    if name.endswith("_host") and pointee in _SCALARS:
        return C.POINTER(_SCALARS[pointee])
    return TensorPtr


def _ret(function, ctype):
    if ctype == "int":
        return _INT if function in _INT_VALUES or function.endswith("_supported") else _STATUS
    return {"size_t": _SIZE, "const char*": _STR}[ctype]


# name -> (return kind, argtypes) of every prototype of the header
SIGNATURES = {name: (_ret(name, ret), [_argtype(name, t, p) for t, p in params])
              for name, (ret, params) in _H.prototypes.items()}

_lib = None
_checked = None     # (the library it was made from, the checked set)


class VampireHipError(RuntimeError):
    pass


def load():
    """Load the library and bind every symbol; raises if anything is missing.  The functions of the returned library
    hand status codes back as integers (what the C-ABI tests assert on); `checked()` is the set that raises."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("VAMPIRE_HIP_LIB", lib_path())
    if not os.path.exists(path):
        raise VampireHipError(
            f"{path} not found: build it with `python -m vampire_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (ret, args) in SIGNATURES.items():
        fn = getattr(lib, name)           # AttributeError if the symbol is missing
        fn.restype = ret.ctype
        fn.argtypes = args
    got = lib.vamp_abi_version()
    if got != ABI_VERSION:
        raise VampireHipError(f"ABI version mismatch: library {got}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def _raise_on_status(last_error, name):
    def errcheck(code, func=None, args=None):
        if code != 0:
            raise VampireHipError(f"{name} failed with code {code}: {last_error().decode('utf-8', 'replace')}")
        return code
    return errcheck


def checked(through=None):
    """The entry points of `load()` once more, as attributes of one object, with every status return checked: a call
    that fails raises VampireHipError with the library's message; the value returns (`*_bytes`, `*_supported`, ...)
    come back as they are.  `through`: a stand-in for the library whose attributes the calls are to go through (the
    tests' call recorders); None or the library itself gives the set bound to the library's own symbols."""
    global _checked
    lib = load()
    if through is not None and through is not lib:
        def via(name):
            fn, check = getattr(through, name), _raise_on_status(lib.vamp_last_error, name)
            return lambda *a: check(fn(*a))
        return types.SimpleNamespace(**{name: via(name) if ret.is_status else getattr(through, name)
                                        for name, (ret, _) in SIGNATURES.items()})
    if _checked is None or _checked[0] is not lib:
        fns = {}
        for name, (ret, args) in SIGNATURES.items():
            fn = lib[name]                # (a function object of its own: lib.name is the unchecked one)
            fn.restype, fn.argtypes = ret.ctype, args
            if ret.is_status:
                fn.errcheck = _raise_on_status(lib.vamp_last_error, name)
            fns[name] = fn
        _checked = (lib, types.SimpleNamespace(**fns))
    return _checked[1]


def profile_enable(on: bool):
    checked().vamp_profile_enable(1 if on else 0)


def profile_select(name=None):
    """Restrict the event timer to one kernel slot (by name); None = all slots."""
    vamp = checked()
    slot = -1
    if name is not None:
        for i in range(vamp.vamp_profile_slots()):
            nm, n, ms = C.c_char_p(), C.c_int(), C.c_double()
            vamp.vamp_profile_read(i, nm, n, ms)
            if nm.value.decode() == name:
                slot = i
        if slot < 0:
            raise KeyError(name)
    vamp.vamp_profile_select(slot)


def profile_read():
    """{kernel name: (launches, total_ms)} since the last profile_enable(True)."""
    vamp = checked()
    out = {}
    for slot in range(vamp.vamp_profile_slots()):
        name, n, ms = C.c_char_p(), C.c_int(), C.c_double()
        vamp.vamp_profile_read(slot, name, n, ms)
        if n.value:
            out[name.value.decode()] = (n.value, ms.value)
    return out
