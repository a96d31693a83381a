"""The drop-in boundary on a machine WITHOUT a GPU: libfusionpic.so loads and exports
every symbol include/fusionpic.h declares; spec validation speaks the reference's
".prop <- ..." language; and the product fails loudly, with no CPU fallback, when no
gfx950 device is present.  No compute call is made here."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT, load_json, make_spec

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")
ADDON = os.path.join(ROOT, "fusion-sim_amd", "lib", "fusionpic_napi.node")


SOR_HEADER = os.path.join(ROOT, "include", "fusionsor.h")


def declared_symbols(header=HEADER, prefix="fpic_"):
    text = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_header_symbols_are_all_exported(fp):
    lib = ctypes.CDLL(LIB)
    syms = declared_symbols()
    assert len(syms) >= 28
    for s in syms:
        assert hasattr(lib, s), "libfusionpic.so does not export " + s
    assert sorted(fp.ABI_FUNCTIONS) == syms
    lib.fpic_build_arch.restype = ctypes.c_char_p
    assert lib.fpic_build_arch() == b"gfx950"
    assert lib.fpic_abi_version() == 2


def test_solver_header_symbols_are_all_exported(fp):
    """include/fusionsor.h (the dense iterative solver)."""
    from fusionpic import sor
    lib = ctypes.CDLL(LIB)
    syms = declared_symbols(SOR_HEADER, "fsor_")
    assert len(syms) >= 19
    for s in syms:
        assert hasattr(lib, s), "libfusionpic.so does not export " + s
    assert sorted(sor.ABI_FUNCTIONS) == syms
    assert lib.fsor_abi_version() == 1
    text = open(SOR_HEADER).read()
    for cite in ("matrix_webgl.js:35-711", "matrix_webgl.js:36-40", ":566-697", ":456-475", ":389-424"):
        assert cite in text


def test_solver_validation_and_no_cpu_fallback(fp):
    from fusionpic import sor
    with pytest.raises(fp.FusionPicError) as e:
        sor.makeSORIterative({})
    assert str(e.value) == ".n_power <- Non-optional property is undefined!"
    with pytest.raises(fp.FusionPicError) as e:
        sor.makeSORIterative({"n_power": "3"})
    assert str(e.value) == ".n_power <- Property does not match any given possible types!"
    with pytest.raises(fp.FusionPicError) as e:
        sor.makeSORIterative({"n_power": 0})      # the reference throws while linking programResult
    assert "u_Vsum" in str(e.value)
    if not has_gpu():
        with pytest.raises(fp.FusionPicError) as e:
            sor.makeSORIterative({"n_power": 2})
        assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def test_header_cites_reference_lines():
    text = open(HEADER).read()
    for cite in ("empic.js:30-1529", "empic.js:1157-1350", "empic.js:1413-1434", "empic.js:1436-1469",
                 "empic.js:1471-1495", "utilities.js:118-127", "utilities.js:701-711"):
        assert cite in text


def test_library_does_not_link_the_oracle():
    out = subprocess.check_output(["ldd", LIB]).decode()
    assert "pic_oracle" not in out
    syms = subprocess.check_output(["nm", "-D", LIB]).decode()
    assert "orc_" not in syms


def test_spec_validation_messages_match_reference(fp):
    v = load_json("validation.json")
    good = make_spec(4, 4, 2)
    bad = dict(good); del bad["radius"]
    with pytest.raises(fp.FusionPicError) as e:
        fp.makeCylindricalParticlePusher(bad)
    assert str(e.value) == v["missing_radius"]
    with pytest.raises(fp.FusionPicError) as e:
        fp.makeCylindricalParticlePusher(dict(good, nr="4"))
    assert str(e.value) == v["string_nr"]
    bad = dict(good); del bad["particle_charge"]
    with pytest.raises(fp.FusionPicError) as e:
        fp.makeCylindricalParticlePusher(bad)
    assert str(e.value) == v["missing_charge"]


def test_c_level_validation_precedes_device_probe(fp):
    lib = fp.load_library()
    s = fp.Spec()
    s.radius, s.height, s.nr, s.nz, s.dt, s.nparticles = -1.0, 1.0, 4, 4, 1e-9, 2
    s.particle_mass, s.particle_charge = 1.0, 1.0
    h = ctypes.c_void_p()
    assert lib.fpic_create(ctypes.byref(s), ctypes.byref(h)) == -1
    assert lib.fpic_last_error(None).decode().startswith(".radius <- ")
    s.radius, s.nr = 1.0, 0
    assert lib.fpic_create(ctypes.byref(s), ctypes.byref(h)) == -1
    assert lib.fpic_last_error(None).decode().startswith(".nr <- ")
    assert lib.fpic_create(None, ctypes.byref(h)) == -1


def test_box_refuses_an_axis_of_one_node(fp):
    """the periodic box needs two nodes or more per axis (its tile windows and the rocFFT plan are not made for one); the
    spec check says so before any device is probed"""
    box = dict(radius=1.0, length_y=1.0, height=1.0, nr=8, ny=8, nz=8, dt=1e-10, nparticles=0, count=10, particle_mass=1.0,
               particle_charge=1.0, geometry="cart3d", solver="poisson_fft")
    for key in ("nr", "ny", "nz"):
        with pytest.raises(fp.FusionPicError) as e:
            fp.makeCylindricalParticlePusher(dict(box, **{key: 1}))
        assert str(e.value) == ".%s <- an axis of the periodic box needs at least 2 nodes (got 1)" % key


@pytest.mark.skipif(has_gpu(), reason="a GPU is present")
def test_no_cpu_fallback_without_a_device(fp):
    with pytest.raises(fp.FusionPicError) as e:
        fp.makeCylindricalParticlePusher(make_spec(4, 4, 2))
    assert e.value.code == -2
    assert "no CPU fallback" in str(e.value)


def test_product_sources_never_touch_the_oracle():
    pkg = os.path.join(ROOT, "fusion-sim_amd")
    for dirpath, _, files in os.walk(pkg):
        if os.sep + "build" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".js", ".c", ".cpp", ".hpp", ".hip", ".h")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "pic_oracle" not in text and "orc_f32" not in text and "libpic_oracle" not in text, f


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node is not installed")
def test_node_addon_loads_and_mirrors_reference_surface():
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "fusion-sim_amd"), "napi"])
    script = r"""
const e = require(process.argv[1]);
const out = {arch: e.buildArch(), errors: []};
const good = {radius:1,height:2,nr:4,nz:4,dt:1e-9,nparticles:2,particle_mass:1,particle_charge:1};
for (const bad of [Object.assign({}, good, {radius: undefined}), Object.assign({}, good, {nr: '4'})]) {
  try { e.makeCylindricalParticlePusher(bad); out.errors.push(null); } catch (x) { out.errors.push(x.message); }
}
try { const s = e.makeCylindricalParticlePusher(good); out.methods = Object.keys(s).sort(); s.destroy(); }
catch (x) { out.create_error = x.message; }
console.log(JSON.stringify(out));
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    import json
    out = json.loads(subprocess.check_output([node, "-e", script, shim]))
    v = load_json("validation.json")
    assert out["arch"] == "gfx950"
    assert out["errors"] == [v["missing_radius"], v["string_nr"]]
    if has_gpu():
        ref_api = set(load_json("draw_order.json")["api"]) - {"canvas"}
        assert ref_api <= set(out["methods"])
    else:
        assert "no CPU fallback" in out["create_error"]


@pytest.mark.skipif(node is None, reason="node is not installed")
def test_node_solver_shim_mirrors_reference_surface():
    """matrix_native.js: the factory validates like the reference (utilities.js:118-127), n_power = 0
    throws as the reference does, and without a device the factory throws instead of falling back."""
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "fusion-sim_amd"), "napi"])
    script = r"""
const m = require(process.argv[1]);
const out = {errors: []};
for (const bad of [{}, {n_power: '3'}, {n_power: 0}, {n_power: 2, relaxation: 'x'}]) {
  try { m.makeSORIterative(bad); out.errors.push(null); } catch (x) { out.errors.push(x.message); }
}
try { const eq = m.makeSORIterative({n_power: 1}); out.members = Object.keys(eq).sort(); out.vec_length = eq.vec_length; eq.destroy(); }
catch (x) { out.create_error = x.message; }
console.log(JSON.stringify(out));
"""
    import json
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "matrix_native.js")
    out = json.loads(subprocess.check_output([node, "-e", script, shim]))
    assert out["errors"][0] == ".n_power <- Non-optional property is undefined!"
    assert out["errors"][1] == ".n_power <- Property does not match any given possible types!"
    assert "u_Vsum" in out["errors"][2]
    assert out["errors"][3] == ".relaxation <- Property does not match any given possible types!"
    if has_gpu():
        # members of the object the reference returns (matrix_webgl.js:50-51, :456-704)
        assert {"vec_length", "vec_height", "set_matrix", "set_b", "init_vector", "mv_product", "solve", "x_result_tex"} <= set(out["members"])
        assert out["vec_length"] == 16
    else:
        assert "no CPU fallback" in out["create_error"]


def test_upload_buffers_host_and_device(fp):
    """fusionpic._device_or_host: numpy arrays (converted like JavaScript numbers) and device tensors (anything with
    data_ptr(): passed on as they are, float32 / float64, contiguous)."""
    import numpy as np
    b = fp._device_or_host(np.arange(6, dtype=np.int64).reshape(2, 3))
    assert b.shape == (2, 3) and b.code == fp.F64 and b.ptr == b.keep.ctypes.data
    b = fp._device_or_host(np.zeros((4, 3), dtype=np.float32)[::2])          # not contiguous: copied
    assert b.shape == (2, 3) and b.code == fp.F32 and b.keep.flags["C_CONTIGUOUS"]

    class FakeTensor:
        def __init__(self, dtype, contiguous=True):
            self.dtype, self.shape, self._c = dtype, (5, 3), contiguous
        def data_ptr(self):
            return 0xDEAD0000
        def is_contiguous(self):
            return self._c
    b = fp._device_or_host(FakeTensor("torch.float32"))
    assert b.ptr == 0xDEAD0000 and b.code == fp.F32 and b.shape == (5, 3)
    assert fp._device_or_host(FakeTensor("torch.float64")).code == fp.F64
    for bad in (FakeTensor("torch.float16"), FakeTensor("torch.float32", contiguous=False)):
        with pytest.raises(fp.FusionPicError):
            fp._device_or_host(bad)


def test_rccl_library_override_is_reported(fp, monkeypatch):
    """FPIC_RCCL_LIBRARY names the RCCL build to bind: a path that does not exist is an error with that path in it, not
    a silent fall back to another library (and nothing here needs a GPU)."""
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r); import fusionpic as fp\n"
            "try:\n    fp.commUniqueId()\n    print('bound')\nexcept fp.FusionPicError as e:\n    print('ERR', e)\n") % os.path.join(ROOT, "fusion-sim_amd")
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, FPIC_RCCL_LIBRARY="/nonexistent/librccl.so")).decode()
    assert out.startswith("ERR") and "/nonexistent/librccl.so" in out
