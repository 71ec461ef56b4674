"""ctypes binding of librald_hip.so, derived from its header include/rald_hip.h.

The header is the one declaration of the C ABI: its prototypes give every entry point's restype / argtypes and its
`typedef struct` bodies give the config structs (DitConfig, AeConfig, RadarDspConfig, RadarPointsConfig, LidarConfig).
Every pointer parameter binds as c_void_p, so a call passes `t.data_ptr()` for a tensor, None for NULL, a numpy array's
`.ctypes.data`, ctypes arrays or `byref(struct)`.

The library is the product: if it is missing or fails to load, every entry point raises -
there is no eager/PyTorch fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librald_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "rald_hip.h")
_lock = threading.Lock()
_lib = None

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float,
            "double": C.c_double}


def _scalar(type_name: str, where: str):
    try:
        return _SCALARS[type_name]
    except KeyError:
        raise RuntimeError(f"{HEADER}: unknown type {type_name!r} in `{where}`") from None


def _param(decl: str, where: str):
    """One parameter declaration ('const float* x', 'int64_t n') -> its ctypes type: c_void_p for every pointer."""
    if "*" in decl:
        return C.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if len(words) != 2:
        raise RuntimeError(f"{HEADER}: cannot read the parameter {decl!r} in `{where}`")
    return _scalar(words[0], where)


def _restype(ret: str, where: str):
    ret = " ".join(ret.replace("*", " * ").split())
    if ret == "void":
        return None
    if ret == "const char *":
        return C.c_char_p
    if "*" in ret:
        raise RuntimeError(f"{HEADER}: unknown return type {ret!r} in `{where}`")
    return _scalar(ret, where)


def _struct(body: str, where: str) -> list:
    """`int32_t a, b; double x[6];` -> [("a", c_int32), ("b", c_int32), ("x", c_double * 6)] in field order."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        type_name, names = decl.split(None, 1)
        t = _scalar(type_name, where)
        for name in (n.strip() for n in names.split(",")):
            m = re.fullmatch(r"(\w+)\s*(?:\[\s*(\d+)\s*\])?", name)
            if m is None:
                raise RuntimeError(f"{HEADER}: cannot read the field {name!r} in `{where}`")
            fields.append((m.group(1), t * int(m.group(2)) if m.group(2) else t))
    return fields


def _parse(path: str):
    """(name -> (restype, argtypes), struct typedef name -> _fields_) of every prototype and config struct in the header."""
    with open(path, "r", encoding="utf-8") as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)              # comments
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)                         # preprocessor lines
    text = " ".join(text.split())
    structs = {}
    for m in re.finditer(r"typedef struct \w*\s*\{([^}]*)\}\s*(\w+)\s*;", text):
        structs[m.group(2)] = _struct(m.group(1), m.group(0))
    signatures = {}
    for m in re.finditer(r"([A-Za-z_][\w ]*?\**)\s*\b(rald_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, name, params = m.groups()
        params = params.strip()
        argtypes = [] if params in ("", "void") else [_param(p, m.group(0)) for p in params.split(",")]
        signatures[name] = (_restype(ret, m.group(0)), argtypes)
    return signatures, structs


# name -> (restype, argtypes); everything include/rald_hip.h declares
SIGNATURES, _STRUCT_FIELDS = _parse(HEADER)


def _config_struct(typedef: str) -> type:
    """rald_radar_dsp_config -> class RadarDspConfig(ctypes.Structure) with the header's fields."""
    name = "".join(w.capitalize() for w in typedef[len("rald_"):].split("_"))
    return type(name, (C.Structure,), {"_fields_": _STRUCT_FIELDS[typedef]})


DitConfig = _config_struct("rald_dit_config")
AeConfig = _config_struct("rald_ae_config")
RadarDspConfig = _config_struct("rald_radar_dsp_config")
RadarPointsConfig = _config_struct("rald_radar_points_config")
LidarConfig = _config_struct("rald_lidar_config")


def build_library(verbose: bool = False) -> str:
    """Compile rald_amd/csrc/*.hip for gfx950 into rald_amd/librald_hip.so (hipcc cross-compiles
    without a GPU).  Returns the library path."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j", str(min(8, os.cpu_count() or 1))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-8000:])
    if r.returncode:
        raise RuntimeError("building librald_hip.so failed")
    return LIB_PATH


def lib():
    """The loaded library (cached).  Raises if it is absent - never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(or `make -C rald_amd/csrc`); rald_amd has no CPU/PyTorch fallback")
            L = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(L, name)          # AttributeError if the symbol is not exported
                fn.restype = res
                fn.argtypes = args
            _lib = L
        return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().rald_last_error()
        raise RuntimeError(f"librald_hip: {msg.decode() if msg else 'error'} (status {rc})")
