"""What yak_amd.walk, yak_amd.gfa and yak_amd.path share: the loading of a library that stands above others, its last error and its launch tally
(the exports yakamd_<prefix>_last_error and yakamd_<prefix>_tally_names / _read / _reset, which each of the three libraries has)."""
import ctypes as C
import os

P = C.POINTER


def common(prefix):
    """the signatures of the four exports every layer has"""
    return {f"yakamd_{prefix}_last_error": (C.c_char_p, []), f"yakamd_{prefix}_tally_names": (C.c_int, [P(P(C.c_char_p))]),
            f"yakamd_{prefix}_tally_read": (None, [P(C.c_uint64), C.c_int]), f"yakamd_{prefix}_tally_reset": (None, [])}


def load(path, below, signatures):
    """the library at `path` with {export: (restype, argtypes)} set, after below() has loaded what it stands on.  Raises if it has not been
    built: there is no fallback."""
    below()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make lib` (python __graft_entry__.py build)")
    L = C.CDLL(path)
    for name, (restype, argtypes) in signatures.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    return L


def last_error(L, prefix):
    return (getattr(L, f"yakamd_{prefix}_last_error")() or b"").decode()


def tally(L, prefix):
    """{kernel instantiation: launches since the last yakamd_<prefix>_tally_reset} of the library's own kernels"""
    names = P(C.c_char_p)()
    n = getattr(L, f"yakamd_{prefix}_tally_names")(C.byref(names))
    out = (C.c_uint64 * max(n, 1))()
    getattr(L, f"yakamd_{prefix}_tally_read")(out, n)
    return {names[i].decode(): int(out[i]) for i in range(n)}
