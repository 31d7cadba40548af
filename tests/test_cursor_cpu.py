"""aic_cursor_raycast without a GPU: the restatement (tests/cursor_ref.py) against the reference's own seven tests (cursor.rs:310-436), the coverage of
the case list the GPU test runs, what flat.pack / pack_block make of `selectable`, the library's export, and the host side -- aic_cursor_raycast in aic_ray_queries.cpp
and convert_block -- driven by tools/submit_record/cursor_raycast_record.cpp against the recording fake of the HIP runtime. That program has its own main
and is built here with -fsanitize=address,undefined: host code only, nothing of it is loaded into Python."""
import ctypes
import hashlib
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from all_is_cubes_amd import abi, flat, replay, workloads
from tests import cursor_ref as ref

ROOT = Path(__file__).resolve().parent.parent
INF = float("inf")
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


# ---- the restatement -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(7), ids=[t[0] for t in ref.reference_tests()])
def test_the_references_own_tests(case):
    name, make_space, ray, maximum_distance, expected = ref.reference_tests()[case]
    got = ref.Scene(make_space()).raycast(ray, maximum_distance)
    if expected is None:
        assert got["hit"] == 0 and not ref.field_bytes(got).any()
        return
    assert got["hit"] == 1
    for field, value in expected.items():
        assert np.array_equal(got[field], value), (name, field, got[field])


def test_the_slabs_are_the_references():
    assert ref.slab(1, 2).voxels.shape == (2, 1, 2) and ref.slab(3, 4).voxels.shape == (4, 3, 4)
    assert len(np.unique(ref.slab(3, 4).voxels)) == 2


@pytest.fixture(scope="module")
def outcomes():
    """case name -> (records, the outcomes of its rays)"""
    out = {}
    for name, key, rays, maximum_distance in ref.cases():
        seen = set()
        out[name] = (ref.scene(key).raycast_all(rays, maximum_distance, seen), seen)
    return out


def test_the_case_list_reaches_every_outcome(outcomes):
    seen = set().union(*(s for _, s in outcomes.values()))
    assert [r for r in ref.REQUIRED if r not in seen] == []
    assert ref.HIT_VOXEL in seen
    # scenes of at most 8^3 cubes, blocks of resolution 2 to 16, and a batch of two waves and two lanes
    for key in ref.SPACE_MAKERS:
        sp = ref.scene(key).sp
        assert max(sp.size) <= 8 and all(b.resolution <= 16 for b in sp.blocks)
    assert {b.resolution for b in ref.scene("garden").sp.blocks} >= {1, 2, 4, 8, 16}
    assert len(ref.garden_rays()) == 130


def test_no_hit_has_a_nan_distance_and_misses_are_zero(outcomes):
    for name, (records, _) in outcomes.items():
        assert not np.isnan(records["distance_to_point"]).any(), name
        assert (records["distance_to_point"] >= 0).all(), name
        misses = records[records["hit"] == 0]
        assert not ref.field_bytes(misses).any(), name
    odd, _ = outcomes["garden, odd rays"]
    rays = ref.garden_odd_rays()
    strange = ~np.isfinite(rays).all(axis=1) | (rays[:, 3:] == 0).all(axis=1)
    assert strange.sum() >= 8
    # a zero direction normalises to NaN, which the Raycaster takes for "does not move": such a ray sees the cube it is in and nothing else
    for rec in odd[strange]:
        assert rec["hit"] == 0 or (rec["face_entered"] == ref.WITHIN and rec["distance_to_point"] == 0.0 and not rec["has_preceding"])


def test_maximum_distance_is_exclusive_above(outcomes):
    records, seen = outcomes["row: the hit at exactly maximum_distance"]
    assert ref.HIT_AT_MAXIMUM in seen and records["hit"].all() and (records["distance_to_point"] == 1.5).all()
    scene = ref.scene("row")
    assert scene.raycast(ref.X_RAY, np.nextafter(1.5, 0.0))["hit"] == 0


# ---- the flat space --------------------------------------------------------------------------------------------------

def test_default_blocks_pack_as_before():
    """A BlockDef that says nothing of `selectable` packs byte for byte as it did before there was such a thing (the digest is the parent commit's)."""
    sp = workloads.synthetic_space(n=8, resolution=4, n_blocks=6, seed=1)
    p = sp.pack()
    h = hashlib.sha256()
    for a in (p.lo, p.size, p.block_index, p.light, p.always_invisible, p.blocks, p.voxels, p.palette, p.sky):
        h.update(np.ascontiguousarray(a).tobytes())
    for b in sp.blocks:
        for a in flat.pack_block(b):
            h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == "ba2f3aba2feedad283d01bf36e500cb741c7767c6b536e6974f1d30fb132c9f4"
    assert set(int(f) for f in p.blocks["flags"]) <= {0, flat.FLAG_ONE, flat.FLAG_ONE | flat.FLAG_AIR}
    # the eighth float of a palette that carries nothing is handed on as it is: a pad
    odd = flat.atom((0.5, 0.5, 0.5, 1.0))
    odd.palette[0, 7] = 0.37
    d, _, pal = flat.pack_block(odd)
    assert int(d["flags"][0]) == flat.FLAG_ONE and pal[0, 7] == np.float32(0.37)


def test_pack_sets_the_flags_and_the_eighth_float():
    assert (flat.FLAG_UNSELECTABLE, flat.FLAG_VOXEL_SELECTABLE) == (4, 8)
    sp = ref.scene("garden").sp
    p = sp.pack()
    flags = [int(f) for f in p.blocks["flags"]]
    assert flags[ref.AIR_I] == flat.FLAG_ONE | flat.FLAG_AIR and flags[ref.ATOM] == flat.FLAG_ONE
    assert flags[ref.UNSEL_ATOM] == flat.FLAG_ONE | flat.FLAG_UNSELECTABLE
    assert flags[ref.FLAGGED] == flat.FLAG_VOXEL_SELECTABLE and flags[ref.UNSEL_VOXELS] == flat.FLAG_UNSELECTABLE
    assert flags[ref.FLAGGED_GLASS] == flags[ref.FLAGGED_PAINT] == flat.FLAG_ONE | flat.FLAG_VOXEL_SELECTABLE
    for i, b in enumerate(sp.blocks):
        pal = p.palette[int(p.blocks["pal_off"][i]):][:len(b.palette)]
        d, _, pal1 = flat.pack_block(b)
        assert int(d["flags"][0]) == flags[i] and pal1.tobytes() == pal.tobytes()
        if b.voxel_selectable is None:
            assert pal.tobytes() == b.palette.tobytes()
        else:
            assert (pal[:, :7] == b.palette[:, :7]).all() and (pal[:, 7] == np.where(b.voxel_selectable, 1.0, 0.0)).all()
            assert b.palette[:, 7].tolist() == [0.0] * len(b.palette), "packing writes a copy"
    with pytest.raises(ValueError):
        flat.BlockDef(1, (0, 0, 0), np.zeros((1, 1, 1), np.uint16), flat.evoxel((1, 1, 1, 1))[None, :], is_one=True, voxel_selectable=[True, False])


def test_replay_rebuilds_the_blocks_with_their_bits():
    sp = ref.scene("garden").sp
    for b in sp.blocks:
        d, vox, pal = flat.pack_block(b)
        again = replay._block_from_desc(d[0], vox, pal)
        d2, vox2, pal2 = flat.pack_block(again)
        assert d2.tobytes() == d.tobytes() and vox2.tobytes() == vox.tobytes() and pal2.tobytes() == pal.tobytes()
        assert again.selectable == b.selectable and (again.voxel_selectable is None) == (b.voxel_selectable is None)


# ---- the library -----------------------------------------------------------------------------------------------------

def test_the_library_exports_the_entry_point_and_refuses_a_null_context():
    import torch

    lib = abi.load()
    assert "aic_cursor_raycast" in abi.ABI_SYMBOLS and hasattr(lib, "aic_cursor_raycast")
    assert abi.CURSOR_HIT_DTYPE.itemsize == 144 and abi.CURSOR_HIT_DTYPE.itemsize % 8 == 0
    assert ctypes.sizeof(abi.CursorDesc) == 88 == abi.CURSOR_HIT_DTYPE.fields["hit"][1]
    for f in abi.CursorDesc._fields_:
        assert abi.CURSOR_HIT_DTYPE.fields[f[0]][1] == getattr(abi.CursorDesc, f[0]).offset, f[0]
    lib.aic_cursor_raycast.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p]
    rays = np.zeros((1, 6))
    out = np.zeros(1, abi.CURSOR_HIT_DTYPE)
    assert lib.aic_cursor_raycast(None, abi.LAYER_WORLD, 1, rays.ctypes.data, INF, 0, out.ctypes.data) == 1  # AIC_ERR_INVALID, like every entry point
    if not torch.cuda.is_available():
        lib.aic_create.restype = ctypes.c_void_p
        status = ctypes.c_int(0)
        assert lib.aic_create(0, ctypes.byref(status)) is None and status.value == 2  # AIC_ERR_NO_DEVICE
        with pytest.raises(abi.AicError):
            abi.Context(0)


# ---- the host side against the recording fake ------------------------------------------------------------------------------

QUEUED = ("hipMalloc", "hipMemcpyAsync", "hipMemcpy ", "hipMemsetAsync", "launch_")
REJECTIONS = ["no context", "no rays", "no out", "unknown flag", "unknown flag beside AIC_RAYS_DEVICE", "a layer with no space", "no such layer", "NaN maximum_distance",
              "negative maximum_distance", "minus infinity", "too many rays", "device rays off by 4", "device out off by 4", "NULL pointers with n = 0 and a bad distance"]


@pytest.fixture(scope="module")
def record():
    """scenario name -> its lines, from the sanitizer build; the run itself must be clean"""
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_cursor_record_"), "cursor_raycast_record")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe, "cursor_raycast_record.cpp", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"], check=True, capture_output=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    scenarios, name = {}, None
    for line in run.stdout.split("\n"):
        if line.startswith("== "):
            name = line[3:]
            scenarios[name] = []
        elif name is not None:
            scenarios[name].append(line)
    return scenarios


def part(lines, start, stop_prefix="-- "):
    """the lines after the line `start` up to the next line that begins with `stop_prefix`"""
    at = lines.index(start) + 1
    end = next((i for i in range(at, len(lines)) if lines[i].startswith(stop_prefix)), len(lines))
    return lines[at:end]


def blocks_after(lines, header):
    """the "  block ..." lines that follow the line `header`"""
    at = lines.index(header) + 1
    end = next((i for i in range(at, len(lines)) if not lines[i].startswith("  block ")), len(lines))
    return lines[at:end]


@needs_hipcc
def test_nothing_failed_or_leaked(record):
    assert "end" in record and len(record) >= 20
    assert not any("FAILED" in line or "LEAK" in line for lines in record.values() for line in lines)


@needs_hipcc
def test_every_rejection_queues_nothing_and_leaves_the_context_usable(record):
    lines = record["rejections"]
    for what in REJECTIONS:
        refused = part(lines, f"-- reject: {what}")
        assert len(refused) == 1 and refused[0].startswith("aic_cursor_raycast rc 1 : "), (what, refused)
        if what != "no context":
            assert refused[0].startswith("aic_cursor_raycast rc 1 : aic_cursor_raycast: "), refused
        after = part(lines, f"-- after: {what}")
        assert after[-1] == "aic_cursor_raycast rc 0" and sum(line.startswith("launch_cursor_raycast ") for line in after) == 1, (what, after)
    legal = part(lines, "-- legal: n = 0 with NULL pointers; maximum_distance 0 and +infinity")
    assert legal[0] == "aic_cursor_raycast rc 0", "n = 0 is AIC_OK and does nothing"
    assert [line for line in legal if line.startswith("launch_cursor_raycast ")][0].split(" maximum_distance ")[1].startswith("0x0p+0 ")


@needs_hipcc
def test_one_launch_per_call_of_a_wave_per_64_rays(record):
    for n in (1, 10, 64, 65, 130, 4096):
        for on_device in (0, 1):
            lines = record[f"launch {n} {on_device}"]
            for turn in (0, 1):
                call = part(lines, f"-- call {turn}")
                call = call[:next(i for i, line in enumerate(call) if line.startswith("aic_cursor_raycast rc ")) + 1]
                launches = [line for line in call if line.startswith("launch_cursor_raycast ")]
                assert len(launches) == 1 and launches[0].startswith(f"launch_cursor_raycast groups {-(-n // 64)} n {n} "), (n, on_device, launches)
                assert " maximum_distance 0x1.8p+2 " in launches[0] and launches[0].endswith(" index_mask 16383 S8"), "the upload stream, beside the frame slots"
                copies = [line for line in call if line.startswith("hipMemcpyAsync ")]
                if on_device:
                    assert copies == [] and not any(line.startswith("hipMalloc") for line in call)
                    assert " rays A" in launches[0] and "+0 out A" in launches[0]
                else:
                    assert len(copies) == 2 and f" <- host bytes {48 * n} kind 1 " in copies[0] and copies[1].startswith("hipMemcpyAsync host <- ") and f" bytes {144 * n} kind 2 " in copies[1]
                    assert sum(line.startswith("hipMalloc") for line in call) == (1 if turn == 0 else 0)
                    # the records are staged behind the rays, where the launch writes them
                    staged = launches[0].split(" rays ")[1].split(" ")[0], launches[0].split(" out ")[1].split(" ")[0]
                    assert staged[0].split("+")[0] == staged[1].split("+")[0] and int(staged[1].split("+")[1]) - int(staged[0].split("+")[1]) == 48 * n
                assert call[-1] == "aic_cursor_raycast rc 0" and call[-2].startswith("hipStreamSynchronize S8")


UPLOADED = ["  block 0 resolution 0 selectable 0",                      # AIR
            "  block 1 resolution 0 selectable 1",                      # a visible atom
            "  block 2 resolution 0 selectable 0",                      # ... flagged unselectable
            "  block 3 resolution 0 selectable 0",                      # an invisible atom under the default rule
            "  block 4 resolution 0 selectable 1",                      # an invisible atom whose voxel says selectable
            "  block 5 resolution 0 selectable 0",                      # a visible atom whose voxel says not
            "  block 6 resolution 0 selectable 0",                      # AIR stays unselectable whatever its voxel says
            "  block 7 resolution 2 selectable 1 palette i0 v1 v1",     # the default rule: selectable iff not invisible; the invisible entry first
            "  block 8 resolution 2 selectable 1 palette i1 i0 v0 v1",  # the floats as given, carried through the reordering
            "  block 9 resolution 2 selectable 0 palette i1 i0 v0 v1",  # the block's own bit beside them
            "  block 10 resolution 0 selectable 0"]                     # resolution 1, a stored voxel that says not


@needs_hipcc
def test_the_bits_land_where_the_kernel_reads_them(record):
    lines = record["bits"]
    assert blocks_after(lines, "-- bits after aic_upload_space: 11 blocks") == UPLOADED
    in_place = list(UPLOADED)
    in_place[1] = "  block 1 resolution 0 selectable 0"
    in_place[8] = "  block 8 resolution 2 selectable 1 palette i1 i0 v1 v0"
    assert blocks_after(lines, "-- bits after two replacements in place: 11 blocks") == in_place
    appended = list(in_place)
    appended[7] = "  block 7 resolution 4 selectable 1 palette i1 i0 v0 v1 v0"
    appended += ["  block 11 resolution 2 selectable 0 palette i1 i0 v0 v1", "  block 12 resolution 0 selectable 1"]
    assert blocks_after(lines, "-- bits after a block grown past its ranges and two appended: 13 blocks") == appended
    assert blocks_after(lines, "-- bits after aic_compact: 13 blocks") == appended
    assert "aic_compact rc 0" in lines
    refused = [line for line in lines if line.startswith("aic_replace_block rc 1 : ")]
    assert len(refused) == 5 and all("eighth float" in line for line in refused)
    after = list(appended)
    after[12] = "  block 12 resolution 0 selectable 1"  # (replaced five times by an unflagged atom whose pad is anything: visible, so selectable)
    assert blocks_after(lines, "-- bits after the refused palettes: 13 blocks") == after
    bad_upload = record["bits: an upload with a bad palette"]
    assert any(line.startswith("aic_upload_space rc 1 : ") and "eighth float" in line for line in bad_upload)


@needs_hipcc
def test_a_failed_runtime_call_leaves_the_context_usable(record):
    failed = {name: lines for name, lines in record.items() if name.startswith("failures: ")}
    assert {name.split(" ")[2] for name in failed if name.split(" ")[1] == "0"} == {"hipSetDevice", "hipMalloc", "hipMemcpyAsync", "launch_cursor_raycast", "hipStreamSynchronize"}
    assert {name.split(" ")[2] for name in failed if name.split(" ")[1] == "1"} == {"hipSetDevice", "launch_cursor_raycast", "hipStreamSynchronize"}
    for name, lines in failed.items():
        assert sum(line.endswith(" FAILS") for line in lines) == 1, name
        again = lines.index("-- the same call again")
        first = [line for line in lines[:again] if line.startswith("aic_cursor_raycast rc ")]
        second = [line for line in lines[again:] if line.startswith("aic_cursor_raycast rc ")]
        assert len(first) == 1 and not first[0].endswith(" rc 0"), (name, first)
        assert second == ["aic_cursor_raycast rc 0"], (name, second)
