"""The restatements of the Split presentation path against the reference's golden images, without a device: tests/present_ref.py (tone map order, sRGB8
from f16), tests/present_lines_ref.py (DESIGN.md 4.13's line rule under the frame's real depth plane) and tests/present_text_ref.py (the text grid) are
our own reading of the reference's shaders, and the kernels are held to them bit for bit -- so a reading that drifts from the reference has to fail
here. tests/test_gpu_present_goldens.py holds the device and the host mirror to the same images end to end. Cases, bounds and the restated frames are
tests/present_golden_cases.py's; every test prints the figures it measured before it asserts."""
import numpy as np
import pytest

from tests import present_golden_cases as G
from tests.test_oracle_light import image_diff


def test_cursor_basic(golden_dir):
    """cursor_basic-all within one level under the harness's comparison, with the cursor found by cursor_ref's raycast, made into lines by
    aic_cursor_wireframe and drawn by the restated line pass under the oracle's depth through the mirror camera's depth transform; the same frame
    without the lines misses that bound, so the golden does see the cursor."""
    r = G.cursor_restated()
    rec = r["record"]
    assert tuple(rec["cube"]) == (0, 0, 0) and rec["face_entered"] == 6 and rec["face_selected"] == 6  # the face towards the camera, PZ
    assert r["lines"].shape == (56, 7)
    print("cursor_basic-all, restated:", r["counts"], G.cursor_figures(golden_dir, r["image"], r["plain"]))
    assert r["counts"]["n_pixels"] > 0 and r["counts"]["n_passed"] < r["counts"]["n_fragments"]  # the cube's own depth hides part of the box
    assert image_diff(golden_dir, "cursor_basic-all", r["image"]).max() <= 1
    without = image_diff(golden_dir, "cursor_basic-all", r["plain"])
    print("cursor_basic-all, no lines:", G.levels(without))
    assert without.max() > 1


@pytest.mark.parametrize("half", [False, True], ids=["equal-size source", "half-size source"])
@pytest.mark.parametrize("scale,name", G.TEXT_SCALES)
def test_info_text(golden_dir, scale, name, half):
    """The restated text layer over the orange frame in windows of 1, 1.5 and 2 times the nominal 128 x 96, from a source of the window's size and from
    one of half that (raytracer_size_policy traces at half the nominal size); and without the text the golden is missed."""
    sw, sh = G.text_source_size(scale, half)
    color = np.broadcast_to(np.array([*G.ORANGE, 1.0], np.float16).view(np.uint16), (sh, sw, 4)).copy()
    image = G.text_restated(color, scale)
    exact = G.assert_text_golden(golden_dir, name, image)
    print(f"{name} from {sw}x{sh}: {exact} pixels differ exactly")
    bare = np.empty_like(image)
    bare[...] = (255, 188, 0, 255)
    assert image_diff(golden_dir, name, bare).max() > 100


@pytest.mark.parametrize("name", sorted(G.COLOR_CASES))
def test_colour_through_f16(golden_dir, name):
    """The oracle's linear frame times the exposure, stored as f16 and shown by the restated presentation with the case's tone map: the golden at the
    bound of its RGBA8 test, and the oracle's own RGBA8 within the one level an f16 store can tip."""
    assert G.opaque_everywhere(name), name  # every case of the list ends opaque; one that did not would be left out, by name, in the device test
    image = G.present_color_restated(name)
    at = G.assert_color_bounds(golden_dir, name, image, "restated")
    print(f"{name}: pixels at each level from the oracle's RGBA8 {at}, from the golden {G.golden_levels(golden_dir, name, image)}")
