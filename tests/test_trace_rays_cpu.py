"""aic_trace_rays, the parts that need no GPU: the header declares the call and its two flag bits, the bits collide with no
AIC_FRAME_* flag, abi.py binds the symbol with its nine arguments, and the host module exposes trace_rays."""
import os
import re

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = open(os.path.join(ROOT, "include", "aic_hip.h")).read()


def defines(prefix):
    return {m.group(1): int(m.group(2)) for m in re.finditer(rf"#define ({prefix}[A-Z_]+) (\d+)u?\b", HEADER)}


def test_header_declares_the_call_and_its_flags():
    m = re.search(r"\bint aic_trace_rays\(([^;]*)\);", HEADER)
    assert m, "include/aic_hip.h does not declare aic_trace_rays"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == 9, args
    assert args[0] == "aic_ctx *ctx" and args[1] == "int layer" and args[2] == "uint32_t n" and args[3] == "const double *rays"
    assert args[4] == "uint32_t flags" and args[5] == "float exposure" and args[6] == "void *out"
    assert args[7] == "aic_pixel_aux *aux" and args[8] == "aic_frame_info *info"
    rays = defines("AIC_RAYS_")
    assert set(rays) == {"AIC_RAYS_NO_SKY", "AIC_RAYS_DEVICE"}, rays
    assert defines("AIC_ABI_")["AIC_ABI_VERSION"] == 3  # additive


def test_the_two_bits_collide_with_no_frame_flag():
    rays, frame = defines("AIC_RAYS_"), defines("AIC_FRAME_")
    assert len(frame) >= 7, frame
    values = list(rays.values()) + list(frame.values())
    for v in values:
        assert v > 0 and v & (v - 1) == 0, f"{v} is not a single bit"
    assert len(set(values)) == len(values), (rays, frame)


def test_abi_py_binds_the_symbol_with_nine_arguments():
    from all_is_cubes_amd import abi

    assert "aic_trace_rays" in abi.ABI_SYMBOLS
    rays = defines("AIC_RAYS_")
    assert abi.RAYS_NO_SKY == rays["AIC_RAYS_NO_SKY"] and abi.RAYS_DEVICE == rays["AIC_RAYS_DEVICE"]
    assert callable(abi.Context.trace_rays) and callable(abi.Context.trace_rays_device)
    if abi.LIB_PATH.exists():  # (a built tree: the library exports it and the binding's argument list is the header's)
        lib = abi.load()
        assert hasattr(lib, "aic_trace_rays")
        assert len(lib.aic_trace_rays.argtypes) == 9
    else:
        src = open(os.path.join(ROOT, "all_is_cubes_amd", "abi.py")).read()
        m = re.search(r"lib\.aic_trace_rays\.argtypes = \[(.*)\]", src)
        assert m and len(m.group(1).split(",")) == 9


def test_rust_shim_declares_it():
    ffi = open(os.path.join(ROOT, "rust", "all-is-cubes-hip", "src", "ffi.rs")).read()
    assert re.search(r"pub fn aic_trace_rays\(ctx: \*mut aic_ctx, layer: c_int, n: u32, rays: \*const f64, flags: u32, exposure: f32, out: \*mut c_void, "
                     r"aux: \*mut aic_pixel_aux, info: \*mut aic_frame_info\) -> c_int;", ffi)
    for name, value in defines("AIC_RAYS_").items():
        assert re.search(rf"pub const {name}: u32 = {value};", ffi), name
    lib = open(os.path.join(ROOT, "rust", "all-is-cubes-hip", "src", "lib.rs")).read()
    assert "pub fn trace_rays(" in lib


def test_host_module_exposes_trace_rays():
    hpp = open(os.path.join(ROOT, "all_is_cubes_amd", "host", "aic_host.hpp")).read()
    assert re.search(r"RayResults trace_rays\(int layer, const std::vector<Ray> &rays, bool include_sky", hpp)
    import importlib.util

    if importlib.util.find_spec("all_is_cubes_amd._host") is not None:  # (a built tree)
        from all_is_cubes_amd import _host as H

        assert callable(H.HipRtRenderer.trace_rays)
    else:
        mod = open(os.path.join(ROOT, "all_is_cubes_amd", "host", "py_module.cpp")).read()
        assert '.def("trace_rays"' in mod
