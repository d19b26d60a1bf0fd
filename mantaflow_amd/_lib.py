"""ctypes binding of the C ABI declared in include/manta_hip.h.

The product library is ``mantaflow_amd/csrc/libmanta_hip.so`` (HIP, gfx950).  There is no CPU fallback: if the
library is missing or cannot be loaded the import of any hot-path function raises.  ``use_library`` exists so that
the test-suite can drive the *same* host code with another implementation of the same ABI (the plain-C oracle
restatement, host pointers) -- nothing in this package ever loads anything from ``oracle/`` by itself.

Prototypes are parsed from the header itself, so the binding cannot drift from ``include/manta_hip.h``.

An *extension* is one row of ``EXTENSIONS``, ``MORE_EXTENSIONS`` or ``OPEN_EXTENSIONS`` below: an optional header
``include/manta_hip_<name>.h`` (first table), ``include/ext/manta_hip_<name>.h`` (second table) or ``include/open/manta_hip_<name>.h``
(third table) that is parsed the same way.
Its entries are bound when the loaded library exports them (``Library.<name>`` is then True, and ``mf_<name>_abi_version()`` must
equal the header's ``MF_<NAME>_ABI_VERSION``); a library without them still loads, and the plugins of that extension refuse it.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "manta_hip.h")
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libmanta_hip.so")


class Extension(object):
    """One optional extension of the ABI.  ``name`` is the attribute on Library / SolverLib and fixes the header, the version
    function and the version macro; ``what`` is the phrase the refusals use and ``verb`` the "does" / "do" it takes; ``subdir`` is
    the directory under include/ that holds the header (none: include/ itself)."""

    def __init__(self, name, what, verb, subdir=""):
        self.name, self.what, self.verb = name, what, verb
        self.header = os.path.join(os.path.dirname(_HERE), "include", subdir, "manta_hip_%s.h" % name)
        self.version_fn = "mf_%s_abi_version" % name
        self.version_macro = "MF_%s_ABI_VERSION" % name.upper()

    def not_implemented(self, who, backend):
        """the refusal of a library that lacks this extension (the CPU test backend lacks all of them)"""
        return "%s: the '%s' backend does not implement %s (manta_hip_%s.h)" % (who, backend, self.what, self.name)


EXTENSIONS = (
    Extension("obstacles", "the fill-fraction obstacle plugins", "do"),
    Extension("multigrid", "the multigrid preconditioners PcMGStatic / PcMGDynamic", "do"),
    Extension("resample", "particle resampling", "does"),
    Extension("idp", "implicit density projection", "does"),
    Extension("partls", "the smooth particle level sets", "do"),
    Extension("guiding", "fluid guiding", "does"),
    Extension("secparts", "the secondary particles", "do"),
)
MORE_EXTENSIONS = (
    Extension("turbulence", "the turbulence model", "does", "ext"),
)
"""The second table.  EXTENSIONS above is frozen: tests/test_extensions_api.py pins its seven names and the set of headers
include/manta_hip_*.h, so it cannot grow.  Every later extension is a row here, with its header under include/ext/; the two tables
are treated alike everywhere (binding, SolverLib, build()'s symbol check, the *_HEADER names, core._extension_lib)."""
OPEN_EXTENSIONS = (
    Extension("fields", "the fire, wave-equation and uv-grid plugins", "do", "open"),
    Extension("mesh", "surface meshes", "do", "open"),
    Extension("meshsdf", "mesh level sets", "do", "open"),
    Extension("reinit", "level-set reinitialisation by fast marching", "does", "open"),
    Extension("grid4d", "the 4-D grid and particle-data kernels", "do", "open"),
    Extension("vortex", "vortex particles", "do", "open"),
    Extension("mlflip", "the array bridge and the MLFLIP plugins", "do", "open"),
    Extension("datagen", "the smoke data-generation plugins", "do", "open"),
    Extension("movingobs", "moving obstacles and obstacle coupling", "do", "open"),
    Extension("gridops", "the grid-operation plugins", "do", "open"),
    Extension("meshops", "mesh connectivity, smoothing and component removal", "do", "open"),
    Extension("surfturb", "surface turbulence", "does", "open"),
    Extension("vsheet", "vortex sheets", "do", "open"),
    Extension("mg2d", "the multigrid preconditioners PcMGStatic / PcMGDynamic on 2-D solvers", "do", "open"),
    Extension("mgslab", "the multigrid preconditioners PcMGStatic / PcMGDynamic on z-slabs", "do", "open"),
)
"""The third table, and the last one.  MORE_EXTENSIONS is frozen as well: tests/test_turbulence_api.py pins its one name and the set of
headers include/ext/manta_hip_*.h.  This table is open: the next extension appends a row here, puts its header under include/open/
and brings its own test file.  No test may pin the tuple of names or its length -- a test may only ask that the headers under
include/open/ are exactly the rows' headers and that its own row is found -- so nothing has to move again."""


def all_extensions():
    """the three tables, in order: every place that walks the extensions walks this"""
    return EXTENSIONS + MORE_EXTENSIONS + OPEN_EXTENSIONS


for _ext in all_extensions():    # OBSTACLES_HEADER ... SECPARTS_HEADER, TURBULENCE_HEADER, FIELDS_HEADER, MESH_HEADER, MESHSDF_HEADER, REINIT_HEADER, GRID4D_HEADER, VORTEX_HEADER, MLFLIP_HEADER, DATAGEN_HEADER, MOVINGOBS_HEADER, GRIDOPS_HEADER, MESHOPS_HEADER, SURFTURB_HEADER, VSHEET_HEADER, MG2D_HEADER, MGSLAB_HEADER
    globals()[_ext.name.upper() + "_HEADER"] = _ext.header


def extension(name):
    """the row of the three tables with that attribute name"""
    return next(e for e in all_extensions() if e.name == name)


_CTYPES = {
    "int": ctypes.c_int,
    "int32_t": ctypes.c_int32,
    "int64_t": ctypes.c_int64,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
}


def parse_header(path=HEADER):
    """Return {name: (restype, [argtypes], [argnames])} for every function the header declares."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = {}
    for m in re.finditer(r"(const\s+char\s*\*|int)\s+(mf_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        restype = ctypes.c_char_p if "char" in ret else ctypes.c_int
        argtypes, argnames = [], []
        args = args.strip()
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                pm = re.match(r"(.*?)(\w+)$", a)
                typ, an = pm.group(1).strip(), pm.group(2)
                if "*" in typ:
                    argtypes.append(ctypes.c_char_p if "char" in typ else ctypes.c_void_p)
                else:
                    argtypes.append(_CTYPES[typ.replace("const", "").strip()])
                argnames.append(an)
        protos[name] = (restype, argtypes, argnames)
    return protos


class Library:
    """A loaded implementation of the ABI; ``device`` is the torch device its pointers must live on."""

    def __init__(self, path, device):
        if not os.path.exists(path):
            raise RuntimeError(
                "mantaflow_amd: native library %s not found -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)" % path)
        self.path = path
        self.device = device
        self.cdll = ctypes.CDLL(path)
        self.protos = parse_header()
        missing = []
        for name, (restype, argtypes, _) in self.protos.items():
            try:
                fn = getattr(self.cdll, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.restype = restype
            fn.argtypes = argtypes
        if missing:
            raise RuntimeError("mantaflow_amd: %s lacks ABI symbols: %s" % (path, ", ".join(missing)))
        self.backend = self.cdll.mf_backend().decode()
        want = int(re.search(r"#define\s+MF_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
        got = int(self.cdll.mf_abi_version())
        if got != want:
            raise RuntimeError("mantaflow_amd: %s implements ABI revision %d, include/manta_hip.h declares %d -- rebuild the library"
                               % (path, got, want))
        for ext in all_extensions():
            setattr(self, ext.name, self._bind_extension(path, ext.header, ext.version_fn, ext.version_macro))
        # the z-slab window is thread-local state of the shared object (which stays loaded across Library instances): start
        # from "the grid is the whole domain"; solvers carry their own window and set it per call (core.SolverLib)
        self.cdll.mf_set_slab_window(0, 0)
        self.cdll.mf_set_slab_window_source(0, 0)

    def _bind_extension(self, path, header, version_fn, version_macro):
        """bind the entries of an optional extension header; False when the library has none of it"""
        protos = parse_header(header)
        have = [n for n in protos if hasattr(self.cdll, n)]
        if not have:
            return False
        missing = [n for n in protos if n not in have]
        if missing:
            raise RuntimeError("mantaflow_amd: %s implements part of %s, lacks: %s" % (path, os.path.basename(header), ", ".join(missing)))
        for name in have:
            restype, argtypes, _ = protos[name]
            fn = getattr(self.cdll, name)
            fn.restype = restype
            fn.argtypes = argtypes
        want = int(re.search(r"#define\s+%s\s+(\d+)" % version_macro, open(header).read()).group(1))
        got = int(getattr(self.cdll, version_fn)())
        if got != want:
            raise RuntimeError("mantaflow_amd: %s implements %s revision %d, the header declares %d -- rebuild the library"
                               % (path, os.path.basename(header), got, want))
        return True

    def call(self, name, *args):
        fn = getattr(self.cdll, name)
        rc = fn(*args)
        if rc != 0:
            msg = self.cdll.mf_last_error().decode(errors="replace")
            raise RuntimeError(msg)
        return rc


_current = None


def get():
    """The active library (loads the HIP product library on first use; fails loudly if absent)."""
    global _current
    if _current is None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("mantaflow_amd: no GPU visible (torch.cuda.is_available() is False); the hot path "
                               "has no CPU fallback")
        _current = Library(DEFAULT_LIB, "cuda")
    return _current


def use_library(path, device):
    """Test hook: route the host layer through another implementation of the same ABI (e.g. the oracle)."""
    global _current
    _current = Library(path, device)
    return _current


def reset():
    global _current
    _current = None
