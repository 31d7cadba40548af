// py_module.cpp -- pybind11 exposure of the C++ host mirror (aic_host.hpp) so that the Python
// tests and bench.py can drive the same classes a C++ (or, via the C ABI, Rust) caller uses.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "aic_host.hpp"

namespace py = pybind11;
using namespace aic::host;

static Vec3 v3(const std::array<double, 3> &a) { return Vec3{a[0], a[1], a[2]}; }
static std::array<double, 3> a3(const Vec3 &v) { return {v.x, v.y, v.z}; }
static py::array_t<double> mat(const Mat4 &m) {
    py::array_t<double> out({4, 4});
    std::memcpy(out.mutable_data(), m.m, sizeof(m.m));
    return out;
}

PYBIND11_MODULE(_host, m) {
    m.doc() = "C++ host mirror of the all-is-cubes raytracer interface above the MI355X C ABI";

    py::register_exception<RenderError>(m, "RenderError");

    py::enum_<FogOption>(m, "FogOption").value("None_", FogOption::None).value("Abrupt", FogOption::Abrupt)
        .value("Compromise", FogOption::Compromise).value("Physical", FogOption::Physical);
    py::enum_<ToneMappingOperator>(m, "ToneMappingOperator").value("Clamp", ToneMappingOperator::Clamp).value("Reinhard", ToneMappingOperator::Reinhard);
    py::enum_<AntialiasingOption>(m, "AntialiasingOption").value("None_", AntialiasingOption::None).value("IfCheap", AntialiasingOption::IfCheap)
        .value("Always", AntialiasingOption::Always);
    py::enum_<TransparencyOption::Kind>(m, "TransparencyKind").value("Surface", TransparencyOption::Surface)
        .value("Volumetric", TransparencyOption::Volumetric).value("Threshold", TransparencyOption::Threshold);
    py::enum_<LightingOption::Kind>(m, "LightingKind").value("None_", LightingOption::None).value("Flat", LightingOption::Flat)
        .value("Coarse", LightingOption::Coarse).value("Linear", LightingOption::Linear).value("Smoothstep", LightingOption::Smoothstep)
        .value("Bounce", LightingOption::Bounce);

    py::class_<TransparencyOption>(m, "TransparencyOption").def(py::init<>())
        .def(py::init([](TransparencyOption::Kind k, float t) { TransparencyOption o; o.kind = k; o.threshold = t; return o; }), py::arg("kind"), py::arg("threshold") = 0.5f)
        .def_readwrite("kind", &TransparencyOption::kind).def_readwrite("threshold", &TransparencyOption::threshold);
    py::class_<LightingOption>(m, "LightingOption").def(py::init<>())
        .def(py::init([](LightingOption::Kind k, int s) { LightingOption o; o.kind = k; o.samples = (uint8_t)s; return o; }), py::arg("kind"), py::arg("samples") = 0)
        .def_readwrite("kind", &LightingOption::kind).def_readwrite("samples", &LightingOption::samples);
    py::class_<ExposureOption>(m, "ExposureOption").def(py::init<>())
        .def_readwrite("automatic", &ExposureOption::automatic).def_readwrite("fixed", &ExposureOption::fixed);

    py::class_<GraphicsOptions>(m, "GraphicsOptions")
        .def(py::init<>())
        .def_static("unaltered_colors", &GraphicsOptions::unaltered_colors)
        .def("repair", &GraphicsOptions::repair)
        .def_readwrite("fog", &GraphicsOptions::fog).def_readwrite("fov_y", &GraphicsOptions::fov_y)
        .def_readwrite("tone_mapping", &GraphicsOptions::tone_mapping).def_readwrite("maximum_intensity", &GraphicsOptions::maximum_intensity)
        .def_readwrite("exposure", &GraphicsOptions::exposure).def_readwrite("bloom_intensity", &GraphicsOptions::bloom_intensity)
        .def_readwrite("view_distance", &GraphicsOptions::view_distance).def_readwrite("lighting_display", &GraphicsOptions::lighting_display)
        .def_readwrite("transparency", &GraphicsOptions::transparency).def_readwrite("show_ui", &GraphicsOptions::show_ui)
        .def_readwrite("antialiasing", &GraphicsOptions::antialiasing).def_readwrite("debug_info_text", &GraphicsOptions::debug_info_text)
        .def_readwrite("debug_pixel_cost", &GraphicsOptions::debug_pixel_cost)
        .def_readwrite("debug_light_rays_at_cursor", &GraphicsOptions::debug_light_rays_at_cursor);

    py::class_<Viewport>(m, "Viewport")
        .def(py::init<>())
        .def_static("with_scale", &Viewport::with_scale)
        .def_readwrite("nominal_width", &Viewport::nominal_width).def_readwrite("nominal_height", &Viewport::nominal_height)
        .def_readwrite("framebuffer_width", &Viewport::framebuffer_width).def_readwrite("framebuffer_height", &Viewport::framebuffer_height)
        .def("nominal_aspect_ratio", &Viewport::nominal_aspect_ratio)
        .def("normalize_fb_x", &Viewport::normalize_fb_x).def("normalize_fb_y", &Viewport::normalize_fb_y)
        .def("normalize_fb_x_edge", &Viewport::normalize_fb_x_edge).def("normalize_fb_y_edge", &Viewport::normalize_fb_y_edge)
        .def("is_empty", &Viewport::is_empty).def("pixel_count", &Viewport::pixel_count);

    py::class_<ViewTransform>(m, "ViewTransform")
        .def(py::init<>())
        .def_static("identity", &ViewTransform::identity)
        .def_property("rotation", [](const ViewTransform &t) { return std::array<double, 4>{t.rotation.i, t.rotation.j, t.rotation.k, t.rotation.r}; },
                      [](ViewTransform &t, const std::array<double, 4> &q) { t.rotation = Quat{q[0], q[1], q[2], q[3]}; })
        .def_property("translation", [](const ViewTransform &t) { return a3(t.translation); },
                      [](ViewTransform &t, const std::array<double, 3> &v) { t.translation = v3(v); });
    m.def("look_at_y_up", [](const std::array<double, 3> &eye, const std::array<double, 3> &target) { return look_at_y_up(v3(eye), v3(target)); });
    m.def("eye_for_look_at", [](const std::array<int32_t, 3> &lo, const std::array<int32_t, 3> &hi, const std::array<double, 3> &dir) {
        GridAab b;
        for (int a = 0; a < 3; a++) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
        return a3(eye_for_look_at(b, v3(dir)));
    });
    m.def("draw_info_text", [](py::array_t<uint8_t, py::array::c_style> image, const std::string &text, const std::array<uint8_t, 4> &outline,
                               const std::array<uint8_t, 4> &foreground) {
        if (image.ndim() != 3 || image.shape(2) != 4) throw std::invalid_argument("draw_info_text: image must be [h][w][4] uint8");
        draw_info_text(image.mutable_data(), (uint32_t)image.shape(1), (uint32_t)image.shape(0), outline.data(), foreground.data(), text);
    }, py::arg("image"), py::arg("text"), py::arg("outline") = std::array<uint8_t, 4>{0, 0, 0, 255}, py::arg("foreground") = std::array<uint8_t, 4>{255, 255, 255, 255});
    m.def("info_text_font_atlas", [] {
        const std::vector<uint8_t> a = info_text_font_atlas();
        py::array_t<uint8_t> out({(py::ssize_t)(16 * kInfoTextCell[1]), (py::ssize_t)(16 * kInfoTextCell[0]), (py::ssize_t)4});
        std::memcpy(out.mutable_data(), a.data(), a.size());
        return out;
    });
    m.attr("INFO_TEXT_CELL") = py::make_tuple(kInfoTextCell[0], kInfoTextCell[1], kInfoTextCell[2]);
    m.def("logged_image_size_policy", [](const std::array<uint32_t, 2> &size) {
        const std::array<uint32_t, 2> out = logged_image_size_policy(size[0], size[1]);
        return py::make_tuple(out[0], out[1]);
    }, py::arg("size"));
    m.def("rotation_around_y", [](double radians) { Quat q = rotation_around_y(radians); return std::array<double, 4>{q.i, q.j, q.k, q.r}; });

    py::class_<Camera>(m, "Camera")
        .def(py::init<const GraphicsOptions &, const Viewport &>())
        .def("set_options", &Camera::set_options).def("options", &Camera::options)
        .def("set_viewport", &Camera::set_viewport).def("viewport", &Camera::viewport)
        .def("set_view_transform", &Camera::set_view_transform).def("view_transform", &Camera::view_transform)
        .def("look_at_y_up", [](Camera &c, const std::array<double, 3> &eye, const std::array<double, 3> &target) { c.look_at_y_up(v3(eye), v3(target)); })
        .def("set_measured_exposure", &Camera::set_measured_exposure).def("exposure", &Camera::exposure)
        .def("fov_y", &Camera::fov_y).def("view_distance", &Camera::view_distance).def("near_plane_distance", &Camera::near_plane_distance)
        .def("projection_matrix", [](const Camera &c) { return mat(c.projection_matrix()); })
        .def("depth_transform_zw", &Camera::depth_transform_zw)
        .def("view_matrix", [](const Camera &c) { return mat(c.view_matrix()); })
        .def("inverse_projection_view", [](const Camera &c) { return mat(c.inverse_projection_view()); })
        .def_static("reprojection_matrix", &Camera::reprojection_matrix, py::arg("traced_with"), py::arg("current"))
        .def("inverse_projection_zw", &Camera::inverse_projection_zw)
        .def("pinhole", [](const Camera &c) {  // -> (image_from_camera [9] f32 column-major, resolution (w, h) f32, ViewTransform)
            const Pinhole p = c.pinhole();
            py::array_t<float> m(9);
            std::memcpy(m.mutable_data(), p.image_from_camera.data(), sizeof(float) * 9);
            py::array_t<float> res(2);
            std::memcpy(res.mutable_data(), p.resolution.data(), sizeof(float) * 2);
            return py::make_tuple(m, res, p.transform);
        })
        .def("view_position", [](const Camera &c) { return a3(c.view_position()); })
        .def("project_ndc_into_world", [](const Camera &c, double x, double y) { Ray r = c.project_ndc_into_world(x, y); return py::make_tuple(a3(r.origin), a3(r.direction)); })
        .def("project_ndc3_into_world", [](const Camera &c, const std::array<double, 3> &p) { return a3(c.project_ndc3_into_world(v3(p))); })
        .def("post_process_color", &Camera::post_process_color);

    py::class_<PackedLight>(m, "PackedLight")
        .def(py::init<>())
        .def_static("some", &PackedLight::some).def_static("scalar_in", &PackedLight::scalar_in).def_static("one", &PackedLight::one)
        .def(py::init([](int r, int g, int b, int s) { return PackedLight{(uint8_t)r, (uint8_t)g, (uint8_t)b, (uint8_t)s}; }))
        .def("as_texel", [](const PackedLight &p) { return std::array<int, 4>{p.r, p.g, p.b, p.status}; });

    py::class_<Sky>(m, "Sky")
        .def(py::init<>())
        .def_readwrite("kind", &Sky::kind)
        .def("set_uniform", [](Sky &s, const std::array<float, 3> &c) { s.kind = 0; std::memset(s.colors, 0, sizeof(s.colors)); for (int i = 0; i < 3; i++) s.colors[0][i] = c[i]; })
        .def("set_octants", [](Sky &s, py::array_t<float, py::array::c_style | py::array::forcecast> c) {
            if (c.size() != 24) throw std::invalid_argument("octants needs 8x3 floats");
            s.kind = 1;
            std::memcpy(s.colors, c.data(), sizeof(s.colors));
        })
        .def("for_blocks", [](const Sky &s) {
            uint8_t out[7][4];
            s.for_blocks(out);
            py::array_t<uint8_t> a({7, 4});
            std::memcpy(a.mutable_data(), out, sizeof(out));
            return a;
        });

    py::class_<Evoxels>(m, "Evoxels")
        // voxel_selectable: Evoxel::selectable; None: what the ABI's default rule says of the voxel (selectable iff not invisible), so that a block made
        // without it is uploaded as it always was
        .def_static("from_one", [](const std::array<float, 4> &rgba, const std::array<float, 3> &em, std::optional<bool> voxel_selectable) {
            Evoxel v;
            for (int i = 0; i < 4; i++) v.color[i] = rgba[i];
            for (int i = 0; i < 3; i++) v.emission[i] = em[i];
            v.selectable = voxel_selectable ? *voxel_selectable : !(rgba[3] == 0.f && em[0] == 0.f && em[1] == 0.f && em[2] == 0.f);
            return Evoxels::from_one(v);
        }, py::arg("rgba"), py::arg("emission") = std::array<float, 3>{0, 0, 0}, py::arg("voxel_selectable") = py::none())
        .def_static("air", &Evoxels::air)
        .def_static("paletted", [](int resolution, const std::array<int32_t, 3> &vlo, py::array_t<uint16_t, py::array::c_style | py::array::forcecast> idx,
                                   py::array_t<float, py::array::c_style | py::array::forcecast> pal, std::optional<std::vector<bool>> voxel_selectable) {
            if (idx.ndim() != 3) throw std::invalid_argument("indices must be 3-D");
            if (pal.ndim() != 2 || pal.shape(1) != 8) throw std::invalid_argument("palette must be [n][8]");
            if (voxel_selectable && voxel_selectable->size() != (size_t)pal.shape(0)) throw std::invalid_argument("voxel_selectable needs one entry per palette entry");
            Evoxels e;
            e.resolution = resolution;
            e.is_one = false;
            for (int a = 0; a < 3; a++) { e.vlo[a] = vlo[a]; e.vsize[a] = (int32_t)idx.shape(a); }
            e.indices.assign(idx.data(), idx.data() + idx.size());
            e.palette.resize((size_t)pal.shape(0));
            for (size_t i = 0; i < e.palette.size(); i++) {
                const float *p = pal.data() + 8 * i;
                std::memcpy(e.palette[i].color, p, 16);
                std::memcpy(e.palette[i].emission, p + 4, 12);
                e.palette[i].selectable = voxel_selectable ? (bool)(*voxel_selectable)[i] : !(p[3] == 0.f && p[4] == 0.f && p[5] == 0.f && p[6] == 0.f);
            }
            return e;
        }, py::arg("resolution"), py::arg("vlo"), py::arg("indices"), py::arg("palette"), py::arg("voxel_selectable") = py::none())
        .def_readwrite("selectable", &Evoxels::selectable).def("abi_flags", &Evoxels::abi_flags)
        .def("palette_floats", [](const Evoxels &e) {
            std::vector<float> v;
            e.palette_floats(&v);
            py::array_t<float> a({(py::ssize_t)(v.size() / 8), (py::ssize_t)8});
            if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * 4);
            return a;
        })
        .def_readwrite("resolution", &Evoxels::resolution).def_readwrite("is_air", &Evoxels::is_air).def_readwrite("is_one", &Evoxels::is_one)
        .def_readwrite("display_name", &Evoxels::display_name);

    py::class_<Space, std::shared_ptr<Space>>(m, "Space")
        .def(py::init([](const std::array<int32_t, 3> &lo, const std::array<int32_t, 3> &size) {
            return std::make_shared<Space>(GridAab::from_lower_size(lo.data(), size.data()));
        }))
        .def_readwrite("sky", &Space::sky)
        .def("add_block", &Space::add_block).def("set_block_data", &Space::set_block_data).def("n_blocks", &Space::n_blocks)
        .def("set", &Space::set).def("set_light", &Space::set_light).def("fill_all", &Space::fill_all)
        .def("get_block_index", &Space::get_block_index)
        .def("load_contents", [](Space &s, py::array_t<uint16_t, py::array::c_style | py::array::forcecast> bi, py::object light) {
            if ((size_t)bi.size() != s.contents().size()) throw std::invalid_argument("block_index size mismatch");
            const uint8_t *lp = nullptr;
            py::array_t<uint8_t, py::array::c_style | py::array::forcecast> la;
            if (!light.is_none()) {
                la = light.cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
                if ((size_t)la.size() != s.contents().size() * 4) throw std::invalid_argument("light size mismatch");
                lp = la.data();
            }
            s.load_contents(bi.data(), lp);
        }, py::arg("block_index"), py::arg("light") = py::none())
        .def("load_light", [](Space &s, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> la) {
            if ((size_t)la.size() != s.contents().size() * 4) throw std::invalid_argument("light size mismatch");
            s.load_light(la.data());
        }, py::arg("light"))
        .def("bounds", [](const Space &s) { const GridAab &b = s.bounds(); return py::make_tuple(std::array<int32_t, 3>{b.lo[0], b.lo[1], b.lo[2]}, std::array<int32_t, 3>{b.hi[0], b.hi[1], b.hi[2]}); });

    py::class_<UiViewState>(m, "UiViewState")
        .def(py::init<>())
        .def_readwrite("space", &UiViewState::space).def_readwrite("view_transform", &UiViewState::view_transform)
        .def_readwrite("graphics_options", &UiViewState::graphics_options)
        .def_property("backdrop", [](const UiViewState &u) { return std::array<float, 4>{u.backdrop[0], u.backdrop[1], u.backdrop[2], u.backdrop[3]}; },
                      [](UiViewState &u, const std::array<float, 4> &b) { for (int i = 0; i < 4; i++) u.backdrop[i] = b[i]; });
    py::class_<StandardCameras, std::shared_ptr<StandardCameras>>(m, "StandardCameras")
        .def(py::init([]() { return std::make_shared<StandardCameras>(); }))
        .def_readwrite("graphics_options", &StandardCameras::graphics_options).def_readwrite("viewport", &StandardCameras::viewport)
        .def_readwrite("world_space", &StandardCameras::world_space).def_readwrite("world_view_transform", &StandardCameras::world_view_transform)
        .def_readwrite("measured_exposure", &StandardCameras::measured_exposure).def_readwrite("ui", &StandardCameras::ui);

    py::class_<ImageInfo>(m, "ImageInfo")
        .def_readonly("cubes_traced", &ImageInfo::cubes_traced).def_readonly("n_outer", &ImageInfo::n_outer).def_readonly("n_inner", &ImageInfo::n_inner)
        .def_readonly("n_hits", &ImageInfo::n_hits).def_readonly("n_light", &ImageInfo::n_light).def_readonly("kernel_ms", &ImageInfo::kernel_ms)
        .def_readonly("total_ms", &ImageInfo::total_ms).def_readonly("width", &ImageInfo::width).def_readonly("height", &ImageInfo::height)
        .def_readonly("rows_rendered", &ImageInfo::rows_rendered).def("status_text", &ImageInfo::status_text);
    py::enum_<TerminalColorMode>(m, "TerminalColorMode").value("None_", TerminalColorMode::None).value("TwoFiftySix", TerminalColorMode::TwoFiftySix)
        .value("Rgb", TerminalColorMode::Rgb);
    py::enum_<TerminalCharacterMode>(m, "TerminalCharacterMode").value("Names", TerminalCharacterMode::Names).value("Shades", TerminalCharacterMode::Shades)
        .value("Split", TerminalCharacterMode::Split).value("Shapes", TerminalCharacterMode::Shapes).value("Braille", TerminalCharacterMode::Braille);
    py::class_<TerminalOptions>(m, "TerminalOptions")
        .def(py::init<>())
        .def_readwrite("colors", &TerminalOptions::colors).def_readwrite("characters", &TerminalOptions::characters)
        .def("cycle_colors", [](TerminalOptions &o) { o.colors = TerminalOptions::cycle(o.colors); })
        .def("cycle_characters", [](TerminalOptions &o) { o.characters = TerminalOptions::cycle(o.characters); })
        .def("viewport_from_terminal_size", &TerminalOptions::viewport_from_terminal_size, py::arg("cols"), py::arg("rows"));
    py::class_<CellsRendering>(m, "CellsRendering")
        .def_readonly("cols", &CellsRendering::cols).def_readonly("rows", &CellsRendering::rows).def_readonly("info", &CellsRendering::info)
        .def_property_readonly("cells", [](const CellsRendering &r) {  // [rows, cols, 3] u32: glyph, fg, bg -- view it as abi.CELL_DTYPE
            py::array_t<uint32_t> a({(py::ssize_t)r.rows, (py::ssize_t)r.cols, (py::ssize_t)3});
            if (!r.cells.empty()) std::memcpy(a.mutable_data(), r.cells.data(), r.cells.size() * sizeof(aic_cell));
            return a;
        })
        .def_property_readonly("counters", [](const CellsRendering &r) {
            py::array_t<uint32_t> a((py::ssize_t)16);  // n_cells, then the fifteen branch counters in aic_cells_info's order
            std::memcpy(a.mutable_data(), &r.cells_info, 16 * 4);
            return a;
        })
        .def_property_readonly("kernel_ms", [](const CellsRendering &r) { return r.cells_info.kernel_ms; });
    py::class_<Rendering>(m, "Rendering")
        .def_readonly("width", &Rendering::width).def_readonly("height", &Rendering::height).def_readonly("flaws", &Rendering::flaws)
        .def_readonly("info", &Rendering::info)
        .def_property_readonly("data", [](const Rendering &r) {
            py::array_t<uint8_t> a({(py::ssize_t)r.height, (py::ssize_t)r.width, (py::ssize_t)4});
            if (!r.data.empty()) std::memcpy(a.mutable_data(), r.data.data(), r.data.size());
            return a;
        });

    py::class_<SplitRendering>(m, "SplitRendering")
        .def_readonly("width", &SplitRendering::width).def_readonly("height", &SplitRendering::height).def_readonly("flaws", &SplitRendering::flaws)
        .def_readonly("info", &SplitRendering::info)
        .def_property_readonly("color_f16_bits", [](const SplitRendering &r) {  // [h, w, 4] uint16: view it as numpy float16
            py::array_t<uint16_t> a({(py::ssize_t)r.height, (py::ssize_t)r.width, (py::ssize_t)4});
            if (!r.color.empty()) std::memcpy(a.mutable_data(), r.color.data(), r.color.size() * 2);
            return a;
        })
        .def_property_readonly("depth", [](const SplitRendering &r) {
            py::array_t<float> a({(py::ssize_t)r.height, (py::ssize_t)r.width});
            if (!r.depth.empty()) std::memcpy(a.mutable_data(), r.depth.data(), r.depth.size() * 4);
            return a;
        });

    auto flaws = m.def_submodule("Flaws");
    flaws.attr("OTHER") = Flaws::OTHER; flaws.attr("UNSUPPORTED") = Flaws::UNSUPPORTED; flaws.attr("NO_BLOOM") = Flaws::NO_BLOOM;
    flaws.attr("NO_CURSOR") = Flaws::NO_CURSOR; flaws.attr("OUT_OF_MEMORY") = Flaws::OUT_OF_MEMORY;

    py::class_<Cursor>(m, "Cursor")
        .def(py::init<>())
        .def_property("cube", [](const Cursor &c) { return std::array<int32_t, 3>{c.cube[0], c.cube[1], c.cube[2]}; },
                      [](Cursor &c, std::array<int32_t, 3> v) { std::copy(v.begin(), v.end(), c.cube); })
        .def_readwrite("face_entered", &Cursor::face_entered)
        .def_readwrite("face_selected", &Cursor::face_selected)
        .def_property("point_entered", [](const Cursor &c) { return std::array<double, 3>{c.point_entered[0], c.point_entered[1], c.point_entered[2]}; },
                      [](Cursor &c, std::array<double, 3> v) { std::copy(v.begin(), v.end(), c.point_entered); })
        .def_readwrite("distance_to_point", &Cursor::distance_to_point)
        .def_property("voxel_lo", [](const Cursor &c) { return std::array<int32_t, 3>{c.voxel_lo[0], c.voxel_lo[1], c.voxel_lo[2]}; },
                      [](Cursor &c, std::array<int32_t, 3> v) { std::copy(v.begin(), v.end(), c.voxel_lo); })
        .def_property("voxel_size", [](const Cursor &c) { return std::array<int32_t, 3>{c.voxel_size[0], c.voxel_size[1], c.voxel_size[2]}; },
                      [](Cursor &c, std::array<int32_t, 3> v) { std::copy(v.begin(), v.end(), c.voxel_size); })
        .def_readwrite("resolution", &Cursor::resolution)
        .def_readwrite("block_index", &Cursor::block_index)
        .def_readwrite("layer", &Cursor::layer)
        .def("preceding_cube_or_cube", &Cursor::preceding_cube_or_cube)
        .def_property("voxel", [](const Cursor &c) { return std::array<int32_t, 3>{c.voxel[0], c.voxel[1], c.voxel[2]}; },
                      [](Cursor &c, std::array<int32_t, 3> v) { std::copy(v.begin(), v.end(), c.voxel); })
        .def_property("light", [](const Cursor &c) { return std::array<uint8_t, 4>{c.light.r, c.light.g, c.light.b, c.light.status}; },
                      [](Cursor &c, std::array<uint8_t, 4> v) { c.light = PackedLight{v[0], v[1], v[2], v[3]}; })
        .def_readwrite("preceding_cube", &Cursor::preceding_cube)
        .def_property("preceding_light", [](const Cursor &c) -> std::optional<std::array<uint8_t, 4>> {
                          if (!c.preceding_light) return std::nullopt;
                          return std::array<uint8_t, 4>{c.preceding_light->r, c.preceding_light->g, c.preceding_light->b, c.preceding_light->status};
                      },
                      [](Cursor &c, std::optional<std::array<uint8_t, 4>> v) {
                          if (v) c.preceding_light = PackedLight{(*v)[0], (*v)[1], (*v)[2], (*v)[3]}; else c.preceding_light.reset();
                      })
        .def("wireframe", [](const Cursor &c) {  // [2 n, 7] f32: position, linear RGBA
            const std::vector<aic_line_vertex> v = c.wireframe();
            py::array_t<float> a({(py::ssize_t)v.size(), (py::ssize_t)7});
            if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(aic_line_vertex));
            return a;
        });

    py::class_<PixelPicker>(m, "PixelPicker")
        .def(py::init<uint32_t, uint32_t>(), py::arg("width"), py::arg("height"))
        .def("take", [](PixelPicker &p, size_t n) {
            const std::vector<uint32_t> v = p.take(n);
            py::array_t<uint32_t> a((py::ssize_t)v.size());
            if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * 4);
            return a;
        }, py::arg("n"))
        .def("resize", &PixelPicker::resize, py::arg("width"), py::arg("height"))
        .def("cycle_length", &PixelPicker::cycle_length)
        .def_property_readonly("central", &PixelPicker::central);

    py::class_<HipRtRenderer>(m, "HipRtRenderer")
        .def(py::init([](std::shared_ptr<StandardCameras> cams, py::object policy, int device_id) {
            HipRtRenderer::SizePolicy sp = nullptr;
            if (!policy.is_none()) sp = policy.cast<HipRtRenderer::SizePolicy>();
            return std::make_unique<HipRtRenderer>(std::move(cams), sp, device_id);
        }), py::arg("cameras"), py::arg("size_policy") = py::none(), py::arg("device_id") = -1)
        .def("update", [](HipRtRenderer &r, py::object cursor) {
            if (cursor.is_none()) return r.update_scene(nullptr);
            const Cursor c = cursor.cast<Cursor>();
            return r.update_scene(&c);
        }, py::arg("cursor") = py::none())
        .def("draw", [](HipRtRenderer &r, const std::string &t) { py::gil_scoped_release rel; return r.draw(t); }, py::arg("info_text") = "")
        .def("draw_text", [](HipRtRenderer &r, const std::string &le) { py::gil_scoped_release rel; return r.draw_text(le); }, py::arg("line_ending") = "\n")
        .def("draw_cells", [](HipRtRenderer &r, const TerminalOptions &o) { py::gil_scoped_release rel; return r.draw_cells(o); }, py::arg("options"))
        .def("draw_terminal", [](HipRtRenderer &r, const TerminalOptions &o, bool in_rect, std::array<uint16_t, 2> origin) {
            std::string s;
            { py::gil_scoped_release rel; s = r.draw_terminal(o, in_rect, origin[0], origin[1]); }
            return py::bytes(s);
        }, py::arg("options"), py::arg("in_rect") = false, py::arg("origin") = std::array<uint16_t, 2>{0, 0})
        .def("cells_to_ansi", [](HipRtRenderer &r, const CellsRendering &frame, bool in_rect, std::array<uint16_t, 2> origin) {
            return py::bytes(r.cells_to_ansi(frame, in_rect, origin[0], origin[1]));
        }, py::arg("frame"), py::arg("in_rect") = false, py::arg("origin") = std::array<uint16_t, 2>{0, 0})
        .def("terminal_names", [](HipRtRenderer &r) {  // ((world names, ui names), (world widths, ui widths)): what abi.cells_ansi takes
            const HipRtRenderer::TerminalNames t = r.terminal_names();
            py::list names, widths;
            for (int layer = 0; layer < 2; layer++) {
                py::list n, w;
                for (const std::string &s : t.names[layer]) n.append(py::str(s));
                for (uint8_t v : t.widths[layer]) w.append((int)v);
                names.append(n);
                widths.append(w);
            }
            return py::make_tuple(names, widths);
        })
        .def("present_split_cells", [](HipRtRenderer &r, uintptr_t src_ptr, uintptr_t scratch_ptr, uint32_t cols, uint32_t rows, const TerminalOptions &o) {
            py::gil_scoped_release rel;
            return r.present_split_cells(reinterpret_cast<const void *>(src_ptr), reinterpret_cast<void *>(scratch_ptr), cols, rows, o);
        }, py::arg("src_ptr"), py::arg("scratch_ptr"), py::arg("cols"), py::arg("rows"), py::arg("options"))
        .def("trace_rays", [](HipRtRenderer &r, int layer, py::array_t<double, py::array::c_style | py::array::forcecast> rays, bool include_sky) {
            // rays [n, 6] = origin xyz, direction xyz -> dict(colorbuf [n, 4] f32, hits [n, sizeof(aic_pixel_aux)] u8 -- view it as abi.PIXEL_AUX_DTYPE --, info)
            if (rays.size() % 6 != 0) throw std::invalid_argument("rays: [n, 6] doubles");
            std::vector<Ray> v((size_t)rays.size() / 6);
            if (!v.empty()) std::memcpy(&v[0], rays.data(), v.size() * sizeof(Ray));
            HipRtRenderer::RayResults res;
            { py::gil_scoped_release rel; res = r.trace_rays(layer, v, include_sky); }
            py::array_t<float> colors({(py::ssize_t)v.size(), (py::ssize_t)4});
            py::array_t<uint8_t> hits({(py::ssize_t)v.size(), (py::ssize_t)sizeof(aic_pixel_aux)});
            if (!v.empty()) {
                std::memcpy(colors.mutable_data(), res.colors.data(), v.size() * 16);
                std::memcpy(hits.mutable_data(), res.hits.data(), v.size() * sizeof(aic_pixel_aux));
            }
            py::dict d;
            d["colorbuf"] = colors; d["hits"] = hits; d["info"] = res.info;
            return d;
        }, py::arg("layer"), py::arg("rays"), py::arg("include_sky") = true)
        .def("cursor_raycast", [](HipRtRenderer &r, int layer, py::array_t<double, py::array::c_style | py::array::forcecast> rays, double maximum_distance) -> py::object {
            // rays [6] -> a Cursor or None; rays [n, 6] -> a list of them (one launch)
            if (!((rays.ndim() == 1 && rays.shape(0) == 6) || (rays.ndim() == 2 && rays.shape(1) == 6))) throw std::invalid_argument("rays must be [6] or [n][6]: origin xyz, direction xyz");
            std::vector<Ray> v((size_t)(rays.size() / 6));
            if (!v.empty()) std::memcpy((void *)v.data(), rays.data(), v.size() * sizeof(Ray));
            std::vector<std::optional<Cursor>> res;
            { py::gil_scoped_release rel; res = r.cursor_raycast(layer, v, maximum_distance); }
            if (rays.ndim() == 1) return py::cast(res[0]);
            return py::cast(res);
        }, py::arg("layer"), py::arg("rays"), py::arg("maximum_distance"))
        .def("light_rays", [](HipRtRenderer &r, int layer, py::array_t<int32_t, py::array::c_style | py::array::forcecast> cubes, int maximum_distance) {
            // cubes [n, 3] -> a list of (info bytes [32] u8 -- view it as abi.LIGHT_CUBE_INFO_DTYPE --, rays [n_rays, 40] u8 -- abi.LIGHT_RAY_DTYPE --, lines [2 n_lines, 7] f32)
            if (cubes.size() % 3 != 0) throw std::invalid_argument("cubes: [n, 3] ints");
            std::vector<std::array<int32_t, 3>> v((size_t)cubes.size() / 3);
            if (!v.empty()) std::memcpy(v.data(), cubes.data(), v.size() * 12);
            std::vector<HipRtRenderer::LightCubeInfo> res;
            { py::gil_scoped_release rel; res = r.light_rays(layer, v, maximum_distance); }
            py::list out;
            for (const auto &c : res) {
                py::array_t<uint8_t> info((py::ssize_t)sizeof(aic_light_cube_info));
                std::memcpy(info.mutable_data(), &c.info, sizeof(aic_light_cube_info));
                py::array_t<uint8_t> rays({(py::ssize_t)c.rays.size(), (py::ssize_t)sizeof(aic_light_ray)});
                if (!c.rays.empty()) std::memcpy(rays.mutable_data(), c.rays.data(), c.rays.size() * sizeof(aic_light_ray));
                const std::vector<aic_line_vertex> w = c.wireframe();
                py::array_t<float> lines({(py::ssize_t)w.size(), (py::ssize_t)7});
                std::memcpy(lines.mutable_data(), w.data(), w.size() * sizeof(aic_line_vertex));
                out.append(py::make_tuple(info, rays, lines));
            }
            return out;
        }, py::arg("layer"), py::arg("cubes"), py::arg("maximum_distance"))
        .def_readwrite("light_rays_maximum_distance", &HipRtRenderer::light_rays_maximum_distance)
        .def("project_cursor", [](HipRtRenderer &r, double ndc_x, double ndc_y) {
            std::optional<Cursor> c;
            { py::gil_scoped_release rel; c = r.project_cursor(ndc_x, ndc_y); }
            return c;
        }, py::arg("ndc_x"), py::arg("ndc_y"))
        .def("sample_luminance", [](HipRtRenderer &r, int layer, py::array_t<double, py::array::c_style | py::array::forcecast> rays, uint32_t max_steps) {
            // rays [n, 6] = origin xyz, direction xyz -> [n] f32
            if (rays.size() % 6 != 0) throw std::invalid_argument("rays: [n, 6] doubles");
            std::vector<Ray> v((size_t)rays.size() / 6);
            if (!v.empty()) std::memcpy(&v[0].origin.x, rays.data(), v.size() * sizeof(Ray));
            std::vector<float> res;
            { py::gil_scoped_release rel; res = r.sample_luminance(layer, v, max_steps); }
            py::array_t<float> out((py::ssize_t)res.size());
            if (!res.empty()) std::memcpy(out.mutable_data(), res.data(), res.size() * sizeof(float));
            return out;
        }, py::arg("layer"), py::arg("rays"), py::arg("max_steps"))
        .def("trace_pixels", [](HipRtRenderer &r, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> pixels) {
            // pixels [n] = y * width + x -> dict(color_f16_bits [n, 4] u16 -- view it as numpy float16 --, depth [n] f32, hits [n, sizeof(aic_pixel_aux)] u8, info)
            std::vector<uint32_t> v((size_t)pixels.size());
            if (!v.empty()) std::memcpy(v.data(), pixels.data(), v.size() * 4);
            HipRtRenderer::PixelResults res;
            { py::gil_scoped_release rel; res = r.trace_pixels(v); }
            py::array_t<uint16_t> color({(py::ssize_t)v.size(), (py::ssize_t)4});
            py::array_t<float> depth((py::ssize_t)v.size());
            py::array_t<uint8_t> hits({(py::ssize_t)v.size(), (py::ssize_t)sizeof(aic_pixel_aux)});
            if (!v.empty()) {
                std::memcpy(color.mutable_data(), res.color.data(), v.size() * 8);
                std::memcpy(depth.mutable_data(), res.depth.data(), v.size() * 4);
                std::memcpy(hits.mutable_data(), res.hits.data(), v.size() * sizeof(aic_pixel_aux));
            }
            py::dict d;
            d["color_f16_bits"] = color; d["depth"] = depth; d["hits"] = hits; d["info"] = res.info;
            return d;
        }, py::arg("pixels"))
        .def("trace_pixels_into", [](HipRtRenderer &r, uintptr_t frame_ptr, uintptr_t pixels_ptr, uint32_t n) {
            py::gil_scoped_release rel;
            return r.trace_pixels_into(reinterpret_cast<void *>(frame_ptr), reinterpret_cast<const uint32_t *>(pixels_ptr), n);
        }, py::arg("device_ptr"), py::arg("pixels_ptr"), py::arg("n"))
        .def("reproject_split", [](HipRtRenderer &r, uintptr_t src_ptr, uintptr_t dst_ptr, const Camera &traced_with, uint32_t flags) {
            // -> dict(n_splats, n_dropped, n_gaps, n_unfilled, kernel_ms, levels, t0)
            aic_reproject_info i;
            { py::gil_scoped_release rel; i = r.reproject_split(reinterpret_cast<const void *>(src_ptr), reinterpret_cast<void *>(dst_ptr), traced_with, flags); }
            py::dict d;
            d["n_splats"] = i.n_splats; d["n_dropped"] = i.n_dropped; d["n_gaps"] = i.n_gaps; d["n_unfilled"] = i.n_unfilled;
            d["kernel_ms"] = i.kernel_ms; d["levels"] = i.levels; d["t0"] = py::make_tuple(i.t0[0], i.t0[1]);
            return d;
        }, py::arg("src_ptr"), py::arg("dst_ptr"), py::arg("traced_with"), py::arg("flags") = 0u)
        .def("pick_pixels", [](HipRtRenderer &r, uintptr_t order_ptr, uintptr_t out_ptr, uint32_t n, uint32_t max_unknown) {
            // -> dict(n_unknown, next_cursor, n_from_unknown, n_from_order, kernel_ms)
            aic_pick_info i;
            { py::gil_scoped_release rel; i = r.pick_pixels(reinterpret_cast<const uint32_t *>(order_ptr), reinterpret_cast<uint32_t *>(out_ptr), n, max_unknown); }
            py::dict d;
            d["n_unknown"] = i.n_unknown; d["next_cursor"] = i.next_cursor; d["n_from_unknown"] = i.n_from_unknown; d["n_from_order"] = i.n_from_order;
            d["kernel_ms"] = i.kernel_ms;
            return d;
        }, py::arg("order_ptr"), py::arg("out_ptr"), py::arg("n"), py::arg("max_unknown") = 0u)
        .def("stale_rects", [](const HipRtRenderer &r, const std::vector<std::array<int32_t, 6>> &boxes, int32_t expand) {
            // -> [(x0, y0, x1, y1, dmin, 0)]: the records of abi.STALE_RECT_DTYPE
            py::list out;
            for (const aic_stale_rect &q : r.stale_rects(boxes, expand)) out.append(py::make_tuple(q.x0, q.y0, q.x1, q.y1, q.dmin, q.reserved));
            return out;
        }, py::arg("boxes"), py::arg("expand") = 1)
        .def("changed_boxes", [](const HipRtRenderer &r) { return r.changed_boxes(); })
        .def("pick_stale", [](HipRtRenderer &r, const std::vector<std::tuple<uint16_t, uint16_t, uint16_t, uint16_t, float, uint32_t>> &rects, uintptr_t frame_ptr,
                              uintptr_t order_ptr, uintptr_t out_ptr, uint32_t n, uint32_t max_stale, uint32_t flags) {
            // -> dict(n_stale, next_cursor, n_from_stale, n_from_order, kernel_ms)
            std::vector<aic_stale_rect> v;
            for (const auto &t : rects) v.push_back(aic_stale_rect{std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t), std::get<4>(t), std::get<5>(t)});
            aic_stale_info i;
            {
                py::gil_scoped_release rel;
                i = r.pick_stale(v, reinterpret_cast<const void *>(frame_ptr), reinterpret_cast<const uint32_t *>(order_ptr), reinterpret_cast<uint32_t *>(out_ptr), n,
                                 max_stale, flags);
            }
            py::dict d;
            d["n_stale"] = i.n_stale; d["next_cursor"] = i.next_cursor; d["n_from_stale"] = i.n_from_stale; d["n_from_order"] = i.n_from_order;
            d["kernel_ms"] = i.kernel_ms;
            return d;
        }, py::arg("rects"), py::arg("frame_ptr"), py::arg("order_ptr"), py::arg("out_ptr"), py::arg("n"), py::arg("max_stale"), py::arg("flags") = 0u)
        .def("restart_stale", &HipRtRenderer::restart_stale)
        .def("changed_light_cubes", [](const HipRtRenderer &r) { return r.changed_light_cubes(); })
        .def("clear_changed_light_cubes", &HipRtRenderer::clear_changed_light_cubes)
        .def_readwrite("track_light_changes", &HipRtRenderer::track_light_changes)
        .def("pick_stale_cubes", [](HipRtRenderer &r, uintptr_t frame_ptr, uintptr_t order_ptr, uintptr_t out_ptr, uint32_t n, uint32_t max_stale, uint32_t flags, int32_t expand) {
            // -> dict(n_stale, next_cursor, n_from_stale, n_from_order, kernel_ms, n_rects, whole_frame)
            aic_stale_cubes_info i;
            {
                py::gil_scoped_release release;
                i = r.pick_stale_cubes(reinterpret_cast<const void *>(frame_ptr), reinterpret_cast<const uint32_t *>(order_ptr), reinterpret_cast<uint32_t *>(out_ptr), n, max_stale, flags,
                                       expand);
            }
            py::dict d;
            d["n_stale"] = i.n_stale; d["next_cursor"] = i.next_cursor; d["n_from_stale"] = i.n_from_stale; d["n_from_order"] = i.n_from_order;
            d["kernel_ms"] = i.kernel_ms; d["n_rects"] = i.n_rects; d["whole_frame"] = i.whole_frame;
            return d;
        }, py::arg("frame_ptr"), py::arg("order_ptr"), py::arg("out_ptr"), py::arg("n"), py::arg("max_stale"), py::arg("flags") = 0u, py::arg("expand") = 1)
        .def("changed_blocks", [](const HipRtRenderer &r) { return r.changed_blocks(); })
        .def("changed_cube_boxes", [](const HipRtRenderer &r) { return r.changed_cube_boxes(); })
        .def("find_block_cubes", [](HipRtRenderer &r, const std::vector<uint32_t> &indices, uint32_t capacity) {
            // -> (list of boxes, dict(n_cubes, n_runs, bounds, n_written, merged, kernel_ms))
            std::pair<std::vector<std::array<int32_t, 6>>, aic_block_cubes_info> res;
            {
                py::gil_scoped_release release;
                res = r.find_block_cubes(indices, capacity);
            }
            const aic_block_cubes_info &i = res.second;
            py::dict d;
            d["n_cubes"] = i.n_cubes; d["n_runs"] = i.n_runs; d["bounds"] = std::vector<int32_t>(i.bounds, i.bounds + 6);
            d["n_written"] = i.n_written; d["merged"] = i.merged; d["kernel_ms"] = i.kernel_ms;
            return py::make_tuple(res.first, d);
        }, py::arg("indices"), py::arg("capacity"))
        .def("replace_cube_grid_device", [](HipRtRenderer &r, int layer, uintptr_t ptr, uintptr_t light_ptr, uint32_t max_runs) {
            // -> dict(n_cubes, n_runs, bounds, n_written, merged, kernel_ms); the boxes are changed_boxes()
            aic_block_cubes_info i;
            {
                py::gil_scoped_release release;
                i = r.replace_cube_grid_device(layer, reinterpret_cast<const uint16_t *>(ptr), reinterpret_cast<const uint8_t *>(light_ptr), max_runs);
            }
            py::dict d;
            d["n_cubes"] = i.n_cubes; d["n_runs"] = i.n_runs; d["bounds"] = std::vector<int32_t>(i.bounds, i.bounds + 6);
            d["n_written"] = i.n_written; d["merged"] = i.merged; d["kernel_ms"] = i.kernel_ms;
            return d;
        }, py::arg("layer"), py::arg("ptr"), py::arg("light_ptr") = (uintptr_t)0, py::arg("max_runs") = 4096u)
        .def("pick_stale_blocks", [](HipRtRenderer &r, uintptr_t frame_ptr, uintptr_t order_ptr, uintptr_t out_ptr, uint32_t n, uint32_t max_stale, uint32_t flags, int32_t expand,
                                     uint32_t max_runs) {
            // -> dict(pick = pick_stale_cubes' dict, found = find_block_cubes' dict)
            aic_stale_blocks_info i;
            {
                py::gil_scoped_release release;
                i = r.pick_stale_blocks(reinterpret_cast<const void *>(frame_ptr), reinterpret_cast<const uint32_t *>(order_ptr), reinterpret_cast<uint32_t *>(out_ptr), n, max_stale,
                                        flags, expand, max_runs);
            }
            py::dict p, f, d;
            p["n_stale"] = i.pick.n_stale; p["next_cursor"] = i.pick.next_cursor; p["n_from_stale"] = i.pick.n_from_stale; p["n_from_order"] = i.pick.n_from_order;
            p["kernel_ms"] = i.pick.kernel_ms; p["n_rects"] = i.pick.n_rects; p["whole_frame"] = i.pick.whole_frame;
            f["n_cubes"] = i.found.n_cubes; f["n_runs"] = i.found.n_runs; f["bounds"] = std::vector<int32_t>(i.found.bounds, i.found.bounds + 6);
            f["n_written"] = i.found.n_written; f["merged"] = i.found.merged; f["kernel_ms"] = i.found.kernel_ms;
            d["pick"] = p; d["found"] = f;
            return d;
        }, py::arg("frame_ptr"), py::arg("order_ptr"), py::arg("out_ptr"), py::arg("n"), py::arg("max_stale"), py::arg("flags") = 0u, py::arg("expand") = 1,
           py::arg("max_runs") = 65536u)
        .def_property_readonly("pick_skip_stale", &HipRtRenderer::pick_skip_stale)
        .def_property_readonly("pick_cursor", &HipRtRenderer::pick_cursor)
        .def_property_readonly("pick_skip_unknown", &HipRtRenderer::pick_skip_unknown)
        .def("present_split", [](HipRtRenderer &r, uintptr_t src_ptr, uint32_t out_width, uint32_t out_height, uint32_t flags, uintptr_t out_ptr) -> py::object {
            // out_ptr = 0: the Rendering (RGBA8; flags must be 0); else the image is written to that device pointer -> dict(kernel_ms, levels, t0, bloomed)
            if (!out_ptr) {
                if (flags) throw std::invalid_argument("present_split: a host Rendering is RGBA8; AIC_PRESENT_OUT_F16 needs out_ptr");
                Rendering out;
                { py::gil_scoped_release rel; out = r.present_split(reinterpret_cast<const void *>(src_ptr), out_width, out_height); }
                return py::cast(std::move(out));
            }
            aic_present_info i;
            { py::gil_scoped_release rel; i = r.present_split_to_device(reinterpret_cast<const void *>(src_ptr), reinterpret_cast<void *>(out_ptr), out_width, out_height, flags); }
            py::dict d;
            d["kernel_ms"] = i.kernel_ms; d["levels"] = i.levels; d["t0"] = py::make_tuple(i.t0[0], i.t0[1]); d["bloomed"] = i.bloomed;
            return std::move(d);
        }, py::arg("src_ptr"), py::arg("out_width"), py::arg("out_height"), py::arg("flags") = 0u, py::arg("out_ptr") = (uintptr_t)0)
        .def("export_split", [](HipRtRenderer &r, uintptr_t src_ptr, py::object size) {
            // size = None: logged_image_size_policy of the frame's size; else (width, height). -> dict(size, color [h][w][4] u8, depth [h][w] f32,
            // pinhole (Camera.pinhole()'s tuple), depth_range (near, far), n_surface, depth_min, depth_max, kernel_ms)
            uint32_t w = 0, h = 0;
            if (!size.is_none()) {
                const auto wh = size.cast<std::array<uint32_t, 2>>();
                w = wh[0];
                h = wh[1];
                if (!w && !h) throw std::invalid_argument("export_split: a size of (0, 0) asks for the policy's: pass None");
            }
            HipRtRenderer::SplitExport e;
            { py::gil_scoped_release rel; e = r.export_split(reinterpret_cast<const void *>(src_ptr), w, h); }
            py::array_t<uint8_t> color({(py::ssize_t)e.height, (py::ssize_t)e.width, (py::ssize_t)4});
            if (!e.color.empty()) std::memcpy(color.mutable_data(), e.color.data(), e.color.size());
            py::array_t<float> depth({(py::ssize_t)e.height, (py::ssize_t)e.width});
            if (!e.depth.empty()) std::memcpy(depth.mutable_data(), e.depth.data(), e.depth.size() * sizeof(float));
            py::array_t<float> m(9);
            std::memcpy(m.mutable_data(), e.pinhole.image_from_camera.data(), sizeof(float) * 9);
            py::array_t<float> res(2);
            std::memcpy(res.mutable_data(), e.pinhole.resolution.data(), sizeof(float) * 2);
            py::dict d;
            d["size"] = py::make_tuple(e.width, e.height); d["color"] = color; d["depth"] = depth;
            d["pinhole"] = py::make_tuple(m, res, e.pinhole.transform);
            d["depth_range"] = py::make_tuple(e.depth_range[0], e.depth_range[1]);
            d["n_surface"] = e.info.n_surface; d["depth_min"] = e.info.depth_min; d["depth_max"] = e.info.depth_max; d["kernel_ms"] = e.info.kernel_ms;
            return d;
        }, py::arg("src_ptr"), py::arg("size") = py::none())
        .def("present_split_lines", [](HipRtRenderer &r, uintptr_t src_ptr, uint32_t out_width, uint32_t out_height, py::object lines, uint32_t flags, uintptr_t out_ptr) {
            // lines = None: the cursor of the last update(); else [2 n, 7] f32 (position, linear RGBA). -> (present_split's result, dict(n_clipped_away,
            // n_fragments, n_passed, n_pixels))
            std::vector<aic_line_vertex> v;
            if (!lines.is_none()) {
                const auto a = lines.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                if (a.size() % 14 != 0) throw std::invalid_argument("lines: [2 n, 7] floats");
                v.resize((size_t)a.size() / 7);
                if (!v.empty()) std::memcpy(v.data(), a.data(), v.size() * sizeof(aic_line_vertex));
            }
            const std::vector<aic_line_vertex> *given = lines.is_none() ? nullptr : &v;
            aic_lines_info li{};
            py::object first;
            if (!out_ptr) {
                if (flags) throw std::invalid_argument("present_split_lines: a host Rendering is RGBA8; AIC_PRESENT_OUT_F16 needs out_ptr");
                Rendering out;
                { py::gil_scoped_release rel; out = r.present_split(reinterpret_cast<const void *>(src_ptr), out_width, out_height, given, &li); }
                first = py::cast(std::move(out));
            } else {
                aic_present_info i;
                { py::gil_scoped_release rel; i = r.present_split_to_device(reinterpret_cast<const void *>(src_ptr), reinterpret_cast<void *>(out_ptr), out_width, out_height, flags, given, &li); }
                py::dict d;
                d["kernel_ms"] = i.kernel_ms; d["levels"] = i.levels; d["t0"] = py::make_tuple(i.t0[0], i.t0[1]); d["bloomed"] = i.bloomed;
                first = std::move(d);
            }
            py::dict l;
            l["n_clipped_away"] = li.n_clipped_away; l["n_fragments"] = li.n_fragments; l["n_passed"] = li.n_passed; l["n_pixels"] = li.n_pixels;
            return py::make_tuple(first, l);
        }, py::arg("src_ptr"), py::arg("out_width"), py::arg("out_height"), py::arg("lines") = py::none(), py::arg("flags") = 0u, py::arg("out_ptr") = (uintptr_t)0)
        .def("present_split_text", [](HipRtRenderer &r, uintptr_t src_ptr, uint32_t out_width, uint32_t out_height, const std::string &info_text, bool with_lines,
                                      py::object lines, uint32_t flags, uintptr_t out_ptr) {
            // present_split_lines' arguments and result, with the info text; with_lines = false: no lines pass
            std::vector<aic_line_vertex> v;
            if (!lines.is_none()) {
                const auto a = lines.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                if (a.size() % 14 != 0) throw std::invalid_argument("lines: [2 n, 7] floats");
                v.resize((size_t)a.size() / 7);
                if (!v.empty()) std::memcpy(v.data(), a.data(), v.size() * sizeof(aic_line_vertex));
            }
            const std::vector<aic_line_vertex> *given = lines.is_none() ? nullptr : &v;
            aic_lines_info li{};
            py::object first;
            if (!out_ptr) {
                if (flags) throw std::invalid_argument("present_split_text: a host Rendering is RGBA8; AIC_PRESENT_OUT_F16 needs out_ptr");
                Rendering out;
                { py::gil_scoped_release rel; out = r.present_split(reinterpret_cast<const void *>(src_ptr), out_width, out_height, info_text, with_lines, given, &li); }
                first = py::cast(std::move(out));
            } else {
                aic_present_info i;
                {
                    py::gil_scoped_release rel;
                    i = r.present_split_to_device(reinterpret_cast<const void *>(src_ptr), reinterpret_cast<void *>(out_ptr), out_width, out_height, flags, info_text, with_lines, given, &li);
                }
                py::dict d;
                d["kernel_ms"] = i.kernel_ms; d["levels"] = i.levels; d["t0"] = py::make_tuple(i.t0[0], i.t0[1]); d["bloomed"] = i.bloomed;
                first = std::move(d);
            }
            py::dict l;
            l["n_clipped_away"] = li.n_clipped_away; l["n_fragments"] = li.n_fragments; l["n_passed"] = li.n_passed; l["n_pixels"] = li.n_pixels;
            return py::make_tuple(first, l);
        }, py::arg("src_ptr"), py::arg("out_width"), py::arg("out_height"), py::arg("info_text"), py::arg("with_lines") = false, py::arg("lines") = py::none(),
           py::arg("flags") = 0u, py::arg("out_ptr") = (uintptr_t)0)
        .def("world_camera", [](const HipRtRenderer &r) { return Camera(r.world_camera()); })
        .def("ui_camera", [](const HipRtRenderer &r) { return Camera(r.ui_camera()); })
        .def("set_world_camera_override", [](HipRtRenderer &r, py::object inv, float exposure) {
            if (inv.is_none()) { r.set_world_camera_override(nullptr, 1.0f); return; }
            const auto m = inv.cast<std::array<double, 16>>();
            r.set_world_camera_override(m.data(), exposure);
        }, py::arg("inverse_projection_view"), py::arg("exposure") = 1.0f)
        .def("draw_rgba", [](HipRtRenderer &r, const std::string &t) { py::gil_scoped_release rel; return r.draw_rgba(t); }, py::arg("info_text") = "")
        .def("draw_split", [](HipRtRenderer &r) { py::gil_scoped_release rel; return r.draw_split(); })
        .def("set_bloom", &HipRtRenderer::set_bloom, py::arg("on"))
        .def_property_readonly("bloom", &HipRtRenderer::bloom)
        .def("draw_rows_to_device", [](HipRtRenderer &r, uintptr_t ptr, uint32_t strip_rows, uint32_t n_parts, uint32_t part, bool counters, bool no_feedback) {
            py::gil_scoped_release rel;
            return r.draw_rows_to_device(reinterpret_cast<void *>(ptr), strip_rows, n_parts, part, counters, no_feedback);
        }, py::arg("device_ptr"), py::arg("strip_rows"), py::arg("n_parts"), py::arg("part"), py::arg("counters") = false, py::arg("no_feedback") = false)
        .def("partition_rows", &HipRtRenderer::partition_rows)
        .def("submit_rows_to_device", [](HipRtRenderer &r, uintptr_t ptr, uint32_t strip_rows, uint32_t n_parts, uint32_t part, uint32_t slot) {
            r.submit_rows_to_device(reinterpret_cast<void *>(ptr), strip_rows, n_parts, part, slot);
        }, py::arg("device_ptr"), py::arg("strip_rows"), py::arg("n_parts"), py::arg("part"), py::arg("slot"))
        .def("submit_rows_batch_to_device", [](HipRtRenderer &r, const std::vector<uintptr_t> &ptrs, uint32_t strip_rows, uint32_t n_parts, uint32_t part, uint32_t slot,
                                               const std::vector<std::array<double, 16>> &views) {
            std::vector<void *> outs;
            for (uintptr_t p : ptrs) outs.push_back(reinterpret_cast<void *>(p));
            r.submit_rows_batch_to_device(outs, strip_rows, n_parts, part, slot, views);
        }, py::arg("device_ptrs"), py::arg("strip_rows"), py::arg("n_parts"), py::arg("part"), py::arg("slot"), py::arg("inverse_projection_views") = std::vector<std::array<double, 16>>())
        .def("wait_rows", [](HipRtRenderer &r, uint32_t slot) { py::gil_scoped_release rel; return r.wait_rows(slot); }, py::arg("slot"))
        .def("synchronize", [](HipRtRenderer &r) { py::gil_scoped_release rel; r.synchronize(); })
        .def("assemble_strips", [](HipRtRenderer &r, uintptr_t gathered, uintptr_t out, uint32_t strip_rows, uint32_t n_parts, bool wait) {
            r.assemble_strips(reinterpret_cast<const void *>(gathered), reinterpret_cast<void *>(out), strip_rows, n_parts, wait);
        }, py::arg("gathered"), py::arg("out"), py::arg("strip_rows"), py::arg("n_parts"), py::arg("wait") = true)
        .def("modified_viewport", &HipRtRenderer::modified_viewport)
        .def("device_name", &HipRtRenderer::device_name)
        .def("stream", [](const HipRtRenderer &r) { return reinterpret_cast<uintptr_t>(r.stream()); })
        .def("wait_event", [](HipRtRenderer &r, uintptr_t ev) { r.wait_event(reinterpret_cast<void *>(ev)); })
        .def("stream_wait_rows", [](HipRtRenderer &r, uint32_t slot, uintptr_t stream) { r.stream_wait_rows(slot, reinterpret_cast<void *>(stream)); },
             py::arg("slot"), py::arg("hip_stream"))
        .def("evaluate_light", [](HipRtRenderer &r, int maximum_distance, bool fast, int epsilon, int batch, int queue_order, int lanes_per_cube, bool continue_queue,
                                  uint64_t max_updates) {
            const HipRtRenderer::LightUpdateInfo i = r.evaluate_light(maximum_distance, fast, epsilon, batch, queue_order, lanes_per_cube, continue_queue, max_updates);
            py::dict d;
            d["updates"] = i.updates; d["batches"] = i.batches; d["cost"] = i.cost; d["device_ms"] = i.device_ms;
            d["total_ms"] = i.total_ms; d["queue_left"] = i.queue_left; d["bundles_visited"] = i.bundles_visited;
            return d;
        }, py::arg("maximum_distance"), py::arg("fast") = true, py::arg("epsilon") = 1, py::arg("batch") = 32, py::arg("queue_order") = 16, py::arg("lanes_per_cube") = 0, py::arg("continue_queue") = false,
           py::arg("max_updates") = 0)
        .def("evaluate_light_submit", [](HipRtRenderer &r, int maximum_distance, bool fast, int epsilon, int batch, int queue_order, int lanes_per_cube, bool continue_queue,
                                         uint64_t max_updates) { r.evaluate_light_submit(maximum_distance, fast, epsilon, batch, queue_order, lanes_per_cube, continue_queue, max_updates); },
             py::arg("maximum_distance"), py::arg("fast") = true, py::arg("epsilon") = 1, py::arg("batch") = 32, py::arg("queue_order") = 16, py::arg("lanes_per_cube") = 0,
             py::arg("continue_queue") = false, py::arg("max_updates") = 0)
        .def("evaluate_light_done", &HipRtRenderer::evaluate_light_done)
        .def("evaluate_light_wait", [](HipRtRenderer &r) {
            py::gil_scoped_release rel;
            const HipRtRenderer::LightUpdateInfo i = r.evaluate_light_wait();
            py::gil_scoped_acquire acq;
            py::dict d;
            d["updates"] = i.updates; d["batches"] = i.batches; d["cost"] = i.cost; d["device_ms"] = i.device_ms;
            d["total_ms"] = i.total_ms; d["queue_left"] = i.queue_left; d["bundles_visited"] = i.bundles_visited;
            return d;
        })
        .def_readwrite("device_light", &HipRtRenderer::device_light)
        .def_readwrite("device_light_queue_order", &HipRtRenderer::device_light_queue_order)
        .def_readwrite("enable_counters", &HipRtRenderer::enable_counters);

    py::class_<ExposureState>(m, "ExposureState")
        .def(py::init<>())
        .def("step", [](ExposureState &s, HipRtRenderer &r, const ViewTransform &vt, int maximum_distance_or_minus_one, double dt) {
            py::gil_scoped_release rel;
            s.step(r, vt, maximum_distance_or_minus_one, dt);
        }, py::arg("renderer"), py::arg("view_transform"), py::arg("maximum_distance_or_minus_one"), py::arg("dt"))
        .def("exposure", &ExposureState::exposure)
        .def("luminance_average", &ExposureState::luminance_average)
        .def("samples", [](const ExposureState &s) {
            const std::array<float, AIC_EXPOSURE_SAMPLES> v = s.samples();
            py::array_t<float> out((py::ssize_t)v.size());
            std::memcpy(out.mutable_data(), v.data(), sizeof(float) * v.size());
            return out;
        })
        .def_property_readonly("sample_index", &ExposureState::sample_index)
        .def_property_readonly("exposure_log", &ExposureState::exposure_log)
        .def_static("compute_target_exposure", &ExposureState::compute_target_exposure);
}
