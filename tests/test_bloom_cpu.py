"""AIC_FRAME_BLOOM without a GPU: the chain's geometry, invariants of the NumPy restatement (tests/bloom_ref.py), the restatement against
the reference's golden image through the oracle, the ABI's symbols, and the budget of aic_bloom.hip's kernels.

tests/golden/png_bloom-0.25-all.npy is test-renderers/expected/renderers/bloom-0.25-all.png (cases/src/lib.rs:186-201, threshold 12)
decoded as tests/golden/make_golden.py decodes the others: Image.open(...).convert("RGBA"), then np.save."""
import os
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi
from tests import bloom_ref, scenes
from tests.test_oracle_light import image_diff, spawn_camera

ROOT = Path(__file__).resolve().parent.parent
GEOMETRY = {  # (W, H) -> (L, (T0x, T0y))
    (1, 1): (1, (2, 2)),
    (2, 2): (1, (2, 2)),
    (3, 5): (2, (4, 4)),
    (17, 9): (3, (16, 8)),
    (128, 256): (6, (64, 128)),
    (1920, 1080): (6, (960, 576)),
    (3840, 2160): (6, (1920, 1088)),
}


@pytest.mark.parametrize("size", sorted(GEOMETRY))
def test_chain_geometry(size):
    assert bloom_ref.geometry(*size) == GEOMETRY[size]
    assert abi.bloom_geometry(*size) == GEOMETRY[size]


@pytest.mark.parametrize("size", [(3, 5), (17, 9), (40, 24)])
def test_a_constant_image_stays_constant(size):
    w, h = size
    value = np.array([0.75, 3.5, 0.125, 1.0], np.float32)
    cb = np.broadcast_to(np.array([0.75, 3.5, 0.125, 0.0], np.float32), (h, w, 4)).copy()
    stages = []
    b = bloom_ref.chain(cb, 1.0, stages)
    assert stages and all((m == value).all() for _, _, m in stages), [(n, k) for n, k, m in stages if not (m == value).all()]
    assert (b == value).all()
    # each downsample alone, from a constant input twice the output's size, and downsample 0 from a frame stretched onto mip 0
    inp = np.broadcast_to(value, (2 * h, 2 * w, 4)).copy()
    assert (bloom_ref.downsample(inp, w, h) == value).all()
    _, (tx, ty) = bloom_ref.geometry(w, h)
    assert (bloom_ref.downsample(bloom_ref.scene(cb, 1.0), tx, ty) == value).all()


def test_stage_order():
    stages = []
    bloom_ref.chain(np.zeros((256, 128, 4), np.float32), 1.0, stages)
    order = [(n, k) for n, k, _ in stages]
    rep0 = [("down", k) for k in range(6)] + [("up", k) for k in range(4, -1, -1)]
    rep = [("down", k) for k in range(1, 6)] + [("up", k) for k in range(4, -1, -1)]
    assert order == rep0 + rep + rep


def bloom_scene_colorbuf():
    """The bloom scene as the oracle traces it (opaque everywhere: straight and premultiplied colours agree), as a ColorBuf."""
    sp = scenes.bloom_test_space()
    cam = spawn_camera((128, 256), (1.5, 3.0, 8.0), (0.0, 0.0, -1.0), fov=45.0)
    ref = oracle.render(oracle.Space(sp), oracle.unaltered_colors(lighting=3), cam, threads=4, want_linear=True)
    lin = ref["linear"]
    assert (lin[..., 3] == 1.0).all()
    return np.concatenate([lin[..., :3], 1.0 - lin[..., 3:]], axis=-1).astype(np.float32), ref["rgba8"]


def test_golden_bloom_025():
    """The case's threshold, 12, holds for the restated chain on the scene clamped to [0, 1] (3 levels at most), and fails by far on the HDR
    scene. The inference drawn from it, not a known fact: the renderer that made the golden held its linear scene texture as Rgba8UnormSrgb
    (all-is-cubes-gpu frame_texture.rs:509-520, the format taken where the backend cannot render to Rgba16Float), which stores the emissive
    green 100 of the bloom block as 1. The golden does discriminate between chains: perturbed ones (no H term, one repetition, i = 0.125,
    B = 0) land 16-77 levels away on the clamped scene. The HDR scene this project keeps (Rgba16Float, as a desktop GPU renders) blooms about a
    hundred times as bright and misses the golden by up to 229 levels; that bound is pinned here so that a change of either is noticed."""
    cb, _ = bloom_scene_colorbuf()
    clamped = cb.copy()
    clamped[..., :3] = np.minimum(clamped[..., :3], 1.0)
    img, _ = bloom_ref.bloom_frame(clamped, 1.0, 0.25)
    assert image_diff(ROOT / "tests" / "golden", "bloom-0.25-all", img).max() <= 12
    hdr, _ = bloom_ref.bloom_frame(cb, 1.0, 0.25)
    d = image_diff(ROOT / "tests" / "golden", "bloom-0.25-all", hdr).max()
    assert 200 <= d <= 229, d


def test_zero_intensity_is_the_oracle_frame():
    cb, rgba8 = bloom_scene_colorbuf()
    img, _ = bloom_ref.bloom_frame(cb, 1.0, 0.0)
    assert (img == rgba8).all()


def test_symbols_and_flag():
    header = (ROOT / "include" / "aic_hip.h").read_text()
    m = re.search(r"#define AIC_FRAME_BLOOM (\d+)u", header)
    assert m and int(m.group(1)) == abi.FRAME_BLOOM == 64
    assert "aic_probe_bloom" in abi.ABI_SYMBOLS
    lib = abi.load()
    assert hasattr(lib, "aic_probe_bloom")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_bloom_kernels_budget():
    """aic_bloom.hip for gfx950: nothing in scratch, no FLAT memory instruction, LDS only for the composite's sRGB window table."""
    out = os.path.join(tempfile.mkdtemp(prefix="aic_bloom_isa_"), "aic_bloom.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only", "-S",
           str(ROOT / "all_is_cubes_amd" / "csrc" / "aic_bloom.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    asm = open(out).read()
    flat = [line.strip() for line in asm.split("\n") if re.match(r"\s*flat_(load|store|atomic)", line)]
    assert not flat, flat[:5]
    names = re.findall(r"\.name:\s+(_Z\S*bloom\S*kernel\S*)", asm)
    assert len(names) == 4, names
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm)]
    assert len(scratch) == 4 and not any(scratch), scratch
    assert not re.search(r"^\s*scratch_(load|store)", asm, flags=re.M)
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", asm)]
    assert max(lds) <= 4 * 260 + 64, lds
