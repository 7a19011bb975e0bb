"""The C ABI checks of the shared libraries (include/lidar4d_*.h, lidar4d_amd/_*lib.py), written once and run for every row of
LIBRARIES, one row per library: each exports exactly what its header declares, its ctypes signatures are the header's prototypes, a
C99 compiler consumes the header, and the libraries beside liblidar4d_hip.so are mapped on first use only; no two libraries export
a common name; and the table itself is checked against the package, include/ and csrc/Makefile.  No compute calls, no GPU."""
import ctypes
import importlib
import itertools
import os
import re
import shutil
import subprocess
import sys
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# One row per library.  name: liblidar4d_<name>.so behind include/lidar4d_<name>.h, consumed from C by tests/c_abi/<name>_abi_check.c;
# binding: its module under lidar4d_amd (whose Binding has the prefix of its entry points).  Where a library pins them: abi (the ABI
# version), names (the exact SIGNATURES keys), min_bound (at least so many bound entry points), stream_last (every entry point but
# *_workspace takes `void* stream` last), may_skip (skip, not fail, when the library has not been built).
# first_use: what a process may import and construct before the library is mapped (None: mapped with the package).
class Library(namedtuple("Library", "name binding abi names min_bound stream_last may_skip first_use",
                         defaults=(None, None, 0, False, False, None))):
    header = property(lambda self: f"lidar4d_{self.name}.h")
    link = property(lambda self: f"lidar4d_{self.name}")
    c_file = property(lambda self: f"{self.name}_abi_check.c")
    prefix = property(lambda self: _binding(self)._binding.prefix)


LIBRARIES = [
    Library("hip", "_lib", min_bound=36, may_skip=True),
    Library("prep", "_prep_lib",
            first_use="import lidar4d_amd, lidar4d_amd.trainer, sys\n"
                      "assert 'lidar4d_amd.pointprep' not in sys.modules and 'lidar4d_amd._prep_lib' not in sys.modules\n"
                      "from lidar4d_amd import pointprep, _prep_lib as binding\n"
                      "assert 'pointprep' not in lidar4d_amd.__all__\n"),
    Library("eval", "_eval_lib", abi=1,
            first_use="import lidar4d_amd, lidar4d_amd.trainer, lidar4d_amd.metrics\n"
                      "from lidar4d_amd import _eval_lib as binding\n"
                      "from lidar4d_amd.metrics import DepthMeter, IntensityMeter\n"
                      "DepthMeter(1.0), IntensityMeter(1.0)\n"
                      "assert hasattr(lidar4d_amd.trainer.Trainer, 'evaluate')\n"),
    Library("loss", "_loss_lib", abi=1, names={"l4dl_los_workspace", "l4dl_los_fwd", "l4dl_los_bwd"}, stream_last=True,
            first_use="import lidar4d_amd, lidar4d_amd.trainer\n"
                      "from lidar4d_amd import _loss_lib as binding\n"
                      "assert callable(lidar4d_amd.trainer.line_of_sight_loss)\n"),
    Library("patch", "_patch_lib", abi=1, names={"l4dg_patch_workspace", "l4dg_patch_fwd", "l4dg_patch_bwd"}, stream_last=True,
            first_use="import lidar4d_amd, lidar4d_amd.trainer\n"
                      "from lidar4d_amd import _patch_lib as binding\n"
                      "assert callable(lidar4d_amd.trainer.patch_depth_grad_loss)\n"),
    Library("step", "_step_lib", abi=1, names={"l4ds_ray_batch", "l4ds_primary_losses_workspace", "l4ds_primary_losses"},
            stream_last=True,
            first_use="import lidar4d_amd, lidar4d_amd.trainer, lidar4d_amd.kitti360, lidar4d_amd.ops\n"
                      "from lidar4d_amd import _step_lib as binding\n"
                      "assert callable(lidar4d_amd.ops.primary_losses_any) and callable(lidar4d_amd.ops.ray_batch_patches)\n"),
    Library("mlp", "_mlp_lib", abi=1, names={"l4dm_mlp_fwd", "l4dm_mlp_bwd"}, stream_last=True,
            first_use="import lidar4d_amd, lidar4d_amd.trainer, lidar4d_amd.ops, lidar4d_amd.tcnn, sys\n"
                      "assert 'lidar4d_amd._mlp_lib' not in sys.modules\n"
                      "from oracle.make_golden import SMALL_MODEL\n"
                      "lidar4d_amd.LiDAR4D(**SMALL_MODEL)\n"  # a model of the default widths does not touch it,
                      "lidar4d_amd.LiDAR4D(**dict(SMALL_MODEL, hidden_dim_sigma=32, hidden_dim_lidar=128, hidden_dim_flow=16))\n"
                      "assert 'lidar4d_amd._mlp_lib' not in sys.modules\n"  # and constructing one of other widths does not either
                      "from lidar4d_amd import _mlp_lib as binding\n"),
    Library("planes", "_planes_lib", abi=1,
            names={"l4dh_planes_fwd", "l4dh_planes_bwd", "l4dh_density_planes_fwd", "l4dh_density_planes_bwd"}, stream_last=True,
            first_use="import lidar4d_amd, lidar4d_amd.trainer, lidar4d_amd.ops, lidar4d_amd.planes_field, sys\n"
                      "assert 'lidar4d_amd._planes_lib' not in sys.modules\n"
                      "from oracle.make_golden import SMALL_MODEL\n"
                      "lidar4d_amd.LiDAR4D(**SMALL_MODEL)\n"  # a model of the default width does not touch it,
                      "lidar4d_amd.LiDAR4D(**dict(SMALL_MODEL, n_features_per_level_plane=16))\n"
                      "assert 'lidar4d_amd._planes_lib' not in sys.modules\n"  # and constructing one of another width does not either
                      "from lidar4d_amd import _planes_lib as binding\n"),
    Library("march", "_march_lib", abi=1,
            names={"l4dr_march_init", "l4dr_slab_rows", "l4dr_slab_update_workspace", "l4dr_slab_update"}, stream_last=True,
            first_use="import lidar4d_amd, lidar4d_amd.trainer, lidar4d_amd.simulator, lidar4d_amd.ops, lidar4d_amd.early_stop, sys\n"
                      "assert 'lidar4d_amd._march_lib' not in sys.modules\n"
                      "from oracle.make_golden import SMALL_MODEL\n"
                      "lidar4d_amd.LiDAR4D(**SMALL_MODEL)\n"  # neither the package, the march's host side nor a model maps it
                      "assert 'lidar4d_amd._march_lib' not in sys.modules\n"
                      "from lidar4d_amd import _march_lib as binding\n"),
]
ROW = {row.name: row for row in LIBRARIES}
every_library = pytest.mark.parametrize("row", LIBRARIES, ids=lambda row: row.name)


def _binding(row):
    return importlib.import_module("lidar4d_amd." + row.binding)


def _header(row):
    """The public header without its /* */ comments (they name entry points in prose)."""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", row.header)).read(), flags=re.S)


def _exported(path):
    assert shutil.which("nm"), "needs binutils nm"
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def _kind(arg):
    arg = arg.strip()
    if "*" in arg:
        return "ptr"
    for name, k in (("int64_t", "i64"), ("int32_t", "i32"), ("double", "f64"), ("float", "f32"), ("int ", "i32")):
        if arg.startswith(name):
            return k
    raise AssertionError(f"unparsed argument {arg!r}")


def _require_built(row, b):
    if os.path.exists(b.LIB_PATH):
        return
    if row.may_skip:
        pytest.skip(f"lib{row.link}.so not built (run __graft_entry__.build())")
    raise AssertionError(f"lib{row.link}.so not built (run __graft_entry__.build())")


@every_library
def test_exports_declared_abi(row):
    """Header, binding and dynamic symbol table name the same entry points -- and the library nothing else: the helpers its
    translation units share (error text, launch profiling), kernel stubs and handles stay inside (csrc/exports*.map)."""
    b = _binding(row)
    version, last_error = row.prefix + "version", row.prefix + "last_error"
    declared = set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % row.prefix, _header(row)))
    assert {version, last_error} <= declared
    bound = set(b.SIGNATURES) | {version, last_error}
    assert declared == bound, (declared - bound, bound - declared)
    if row.names is not None:
        assert set(b.SIGNATURES) == row.names
    _require_built(row, b)
    lib = ctypes.CDLL(b.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/{row.header} but not exported"
    assert b.version() == b.ABI_VERSION
    if row.abi is not None:
        assert b.ABI_VERSION == row.abi
    exported = _exported(b.LIB_PATH)
    assert exported == declared, (sorted(exported - declared)[:8], declared - exported)


def test_no_library_exports_a_name_of_another():
    exported = {}
    for row in LIBRARIES:
        _require_built(row, _binding(row))
        exported[row.link] = _exported(_binding(row).LIB_PATH)
        assert exported[row.link]
    pairs = list(itertools.combinations(exported, 2))
    assert len(pairs) == len(LIBRARIES) * (len(LIBRARIES) - 1) // 2
    for a, b in pairs:
        assert not exported[a] & exported[b], (a, b, sorted(exported[a] & exported[b])[:8])


def test_the_table_names_every_library():
    """Everything that lists the libraries lists the same ones: the rows here, the package's BINDINGS (what build() checks), the
    binding modules and public headers on disk, and the Makefile's SATELLITES.  A library added in one place only fails here."""
    import glob
    from lidar4d_amd import _lib
    names = [row.name for row in LIBRARIES]
    assert len(set(names)) == len(names)
    assert tuple(row.binding for row in LIBRARIES) == _lib.BINDINGS
    on_disk = lambda pattern: {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, pattern))}
    assert on_disk("lidar4d_amd/_*lib.py") == {b + ".py" for b in _lib.BINDINGS}
    assert on_disk("include/lidar4d_*.h") == {row.header for row in LIBRARIES}
    assert on_disk("tests/c_abi/*_abi_check.c") == {row.c_file for row in LIBRARIES}
    satellites = re.search(r"^SATELLITES\s*:=(.*)$", open(os.path.join(ROOT, "lidar4d_amd", "csrc", "Makefile")).read(), flags=re.M)
    assert satellites.group(1).split() == names[1:] and names[0] == "hip"


@every_library
def test_ctypes_signatures_match_header_prototypes(row):
    """Every prototype of the header against the binding's SIGNATURES: same number of arguments and the same kind (pointer /
    int32 / int64 / float / double) in every position -- a drifted binding would pass garbage silently."""
    from lidar4d_amd import _lib
    b = _binding(row)
    protos = dict(re.findall(r"\b(?:int|int64_t|void\s*\*)\s*(%s[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;" % row.prefix, _header(row), flags=re.S))
    ckind = {_lib.P: "ptr", _lib.I32: "i32", _lib.I64: "i64", _lib.F32: "f32", _lib.F64: "f64", _lib.GD: "ptr", _lib.FD: "ptr",
             _lib.FG: "ptr", _lib.PI32: "ptr", _lib.PI64: "ptr", _lib.PP: "ptr"}
    checked = 0
    for name, argtypes in b.SIGNATURES.items():
        assert name in protos, f"{name} bound but no prototype found"
        args = [a for a in protos[name].split(",") if a.strip() and a.strip() != "void"]
        want, got = [_kind(a) for a in args], [ckind[t] for t in argtypes]
        assert want == got, (name, want, got)
        if row.stream_last and not name.endswith("_workspace"):
            assert re.match(r"void\s*\*\s*stream$", args[-1].strip()), name
        checked += 1
    assert checked == len(b.SIGNATURES) >= row.min_bound
    assert set(protos) == set(b.SIGNATURES) | {row.prefix + "version"}  # (<prefix>last_error returns const char*)


@every_library
def test_c_abi_from_plain_c(row, tmp_path):
    """tests/c_abi/*.c: the header consumed by a C99 compiler (-Wall -Wextra -Werror), every declared entry point linked against
    the shared library, version / error calls executed -- no Python, no torch in the boundary."""
    b = _binding(row)
    _require_built(row, b)
    assert shutil.which("gcc"), "needs gcc"
    exe = str(tmp_path / row.c_file[:-2])
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", row.c_file), "-L", libdir, "-l" + row.link, f"-Wl,-rpath,{libdir}",
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith(f"{len(b.SIGNATURES) + 2} entry points, ABI v{b.ABI_VERSION}")


@pytest.mark.parametrize("row", [r for r in LIBRARIES if r.first_use], ids=lambda row: row.name)
def test_loaded_on_first_use_only(row):
    code = (row.first_use +
            f"assert 'lib{row.link}' not in open('/proc/self/maps').read()\n"
            "binding.lib()\n"
            f"assert 'lib{row.link}' in open('/proc/self/maps').read()\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
