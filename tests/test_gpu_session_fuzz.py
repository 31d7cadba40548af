"""Randomised test of the STATE the interactive loop's calls leave for one another (run with -m gpu on an MI355X): the plans of tests/session_plan.py
-- streamed frames of every output kind on ten slots, scene and light calls, light updates on the worker thread, and between them the work of slot 0
(synchronous frames, the three listed traces, orthographic views), every operation on a resident Split frame R (reproject, the three picks, the three
presentations, export), the two ray queries and the light report -- executed on one context, `a`, with device lists and device targets, against

* `b`, its synchronous twin: the same scene and light calls, never a frame in flight, never the worker thread (it makes `a`'s light update, blocking,
  at the call that publishes it on `a`), the host-pointer form of every listed call. A streamed frame equals b's frame at submit time with its step
  total; a slot-0 trace or ray query equals b's; an in-place trace is compared as the whole of R; the light report equals b's, asked before b's
  blocking update where `a`'s is pending and the call does not publish (session_plan.PUBLISHING, from INTEGRATION.md "Threads" and the header);
* the restatements the suite has (reproject_ref, pick_ref, stale_ref, stale_cubes_ref, present_ref with bloom_ref, present_lines_ref,
  present_text_ref, export_ref), applied to R's bytes as read back from `a`, with every info field and the guard bytes behind each output: these
  operations never run on `b`, so `b` cannot share a stale-scratch error with `a`;
* at a checkpoint every 30 calls (a call of the plan) and at the end, with everything collected: the light volume is b's, the cube grid is
  cube_tags_ref's of the test's own host model of the scene (a flat.FlatSpace kept in step with every scene call), and a linear frame at 64 x 48
  equals oracle.render of that model bit for bit -- a reference that shares no code with the library.

Every comparison is of bytes; there is no tolerance anywhere. (Two planes hold bytes the library does not define: the padding of the first-hit and
cursor records, compared field by field, and the payload of a NaN in an exported depth, as in tests/test_gpu_export.py.) A call refused because a
frame occupies slot 0 must return AIC_ERR_INVALID and leave its sentinel-filled outputs as they were.

Seeds: AIC_SESSION_FUZZ_N (default 6), AIC_SESSION_FUZZ_CALLS calls each (default 160: what tests/test_session_plan_cpu.py's conditions need).
AIC_SESSION_FUZZ_ONLY=seed:n_calls replays a prefix of one seed. A failure names the seed, the call and the last 20 calls of the plan."""
import collections
import os

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat
from all_is_cubes_amd import workloads
from tests import cube_tags_ref, export_ref, pick_ref, present_lines_ref, present_ref, present_text_ref, reproject_ref, stale_cubes_ref, stale_ref
from tests import session_plan as sp
from tests.cursor_ref import field_bytes

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("AIC_SESSION_FUZZ_N", "6"))
N_CALLS = int(os.environ.get("AIC_SESSION_FUZZ_CALLS", "160"))
ONLY = os.environ.get("AIC_SESSION_FUZZ_ONLY")
CASES = [tuple(int(v) for v in ONLY.split(":"))] if ONLY else [(seed, N_CALLS) for seed in range(N_SEEDS)]
GUARD = 256
SENTINEL = 0xA5
WORLD, UI = abi.LAYER_WORLD, abi.LAYER_UI
AIC_ERR_INVALID, AIC_ERR_DEVICE = 1, 4
FLAGS = {"rgba8": 0, "no_feedback": abi.FRAME_NO_FEEDBACK, "split": abi.FRAME_OUT_SPLIT, "resident": abi.FRAME_OUT_SPLIT, "bloom": abi.FRAME_BLOOM,
         "linear": abi.FRAME_OUT_LINEAR, "colorbuf": abi.FRAME_OUT_COLORBUF}
MAX_LIGHT_CUBES = 64  # of a take's cubes, the first so many go to aic_pick_stale_cubes: the restatement projects them one by one
UI_EYE = (1.5, 1.0, 3.0)
TOTALS = collections.Counter()


# --- device memory ----------------------------------------------------------------------------------------------------------------------
def to_device(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def device_bytes(n_bytes, fill=SENTINEL):
    """n_bytes and the guard behind them, sentinel-filled"""
    import torch

    t = torch.full((int(n_bytes) + GUARD,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (torch fills on ITS stream: the fill must not land on what the library's streams write)
    return t


def read_back(t, n_bytes, what):
    raw = t.cpu().numpy()
    assert (raw[n_bytes:n_bytes + GUARD] == SENTINEL).all(), f"guard bytes behind {what}"
    return raw[:n_bytes]


def result_bytes(r):
    """What aic_render / aic_trace_pixels left in `out`, from abi's dict of it"""
    if "rgba8" in r:
        return np.ascontiguousarray(r["rgba8"]).view(np.uint8).reshape(-1)
    return np.concatenate([np.ascontiguousarray(r["color_f16"]).view(np.uint8).reshape(-1), np.ascontiguousarray(r["depth"]).view(np.uint8).reshape(-1)])


def same_fields(got, want):
    return all((np.ascontiguousarray(got[name]).view(np.uint8) == np.ascontiguousarray(want[name]).view(np.uint8)).all() for name in want.dtype.names)


def same_depth_bits(a, b):
    """tests/test_gpu_export.py same_bits: the bit patterns, any NaN equal to any other"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


# --- the scene --------------------------------------------------------------------------------------------------------------------------
def ui_space(variant=0):
    s = flat.FlatSpace((0, 0, 0), (3, 2, 1) if variant == 0 else (2, 2, 1))
    s.set_sky_uniform((1.0, 1.0, 0.5))
    s.add_block(flat.air())
    s.add_block(flat.atom((0.0, 1.0, 0.0, 1.0)))
    s.add_block(flat.atom((0.9, 0.2, 0.1, 0.5)))
    s.block_index[0, 0, 0], s.block_index[-1, 1, 0], s.block_index[1, 0, 0] = 1, 2, variant + 1
    return s


def block_of(spec):
    if spec[0] == "atom":
        return flat.atom(tuple(spec[1]))
    return workloads.synthetic_blocks(8, 1, seed=spec[1], translucent=spec[2])[0]


def font(cell, blank, seed):
    """tests/test_gpu_present_text.py's atlas: random bytes with 0 and 255 among them, the space cell all zero or not"""
    cw, ch, _ = cell
    rng = np.random.default_rng(1000 * cw + 10 * ch + seed)
    atlas = rng.integers(0, 256, (16 * ch, 16 * cw, 4)).astype(np.uint8)
    atlas[rng.random(atlas.shape[:2]) < 0.2] = 0
    atlas[..., 3][rng.random(atlas.shape[:2]) < 0.3] = 255
    if blank:
        atlas[2 * ch:3 * ch, 0:cw] = 0
    else:
        atlas[2 * ch, 0, 3] = 77
    return atlas


def text_grid(cols, rows, corner_only, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    codes[rng.random((rows, cols)) < 0.2] = 0
    codes[rng.random((rows, cols)) < 0.1] = 0x20
    if corner_only:
        codes[(rows + 1) // 2:, :] = 0
        codes[:, (cols + 1) // 2:] = 0
    return codes


def line_vertices(n, seed):
    """[2 n][7] float32: positions across and beside the clip volume, depths in [0, 1), linear RGBA colours; drawn under the identity matrix"""
    rng = np.random.default_rng(seed)
    v = np.zeros((2 * n, 7), np.float32)
    v[:, 0:2] = rng.uniform(-1.3, 1.3, (2 * n, 2))
    v[:, 2] = rng.uniform(0.0, 1.0, 2 * n)
    v[:, 3:7] = rng.random((2 * n, 4))
    return v


def make_rays(n, seed, lo, size):
    """tests/test_gpu_trace_rays.py's recipe around a space: origins in and around it, half the directions aimed into it, some along an axis"""
    rng = np.random.default_rng(seed)
    lo, size = np.asarray(lo, np.float64), np.asarray(size, np.float64)
    o = lo + rng.uniform(-0.3, 1.3, (n, 3)) * size
    aimed = lo + rng.uniform(0.0, 1.0, (n, 3)) * size - o
    d = np.where((rng.random(n) < 0.5)[:, None], aimed, rng.normal(size=(n, 3)))
    d = d * rng.choice([1e-3, 1.0, 40.0], n)[:, None]
    kind = rng.random(n)
    d[kind < 0.10, 0] = 0.0
    d[(kind >= 0.10) & (kind < 0.15), 1:] = 0.0
    return np.ascontiguousarray(np.concatenate([o, d], 1))


class Session:
    """One seed: the two contexts, the host model, R and everything a later call needs of an earlier one."""

    def __init__(self, seed):
        rng = np.random.default_rng(5100 + seed)
        self.seed = seed
        self.has_ui = sp.seed_has_ui(seed)
        self.opts = dict(fog=int(rng.integers(0, 4)), transparency=int(rng.integers(0, 3)), lighting=int(rng.integers(0, 5)), antialiasing=0, bloom_intensity=0.125,
                         view_distance=float(rng.choice([30.0, 200.0])))
        self.ui_opts = dict(fog=0, transparency=1, lighting=0, view_distance=self.opts["view_distance"])
        self.model = workloads.synthetic_space(n=16, resolution=8, n_blocks=6, seed=20 + seed, light="field")
        self.ui_model = ui_space() if self.has_ui else None
        self.a, self.b = abi.Context(0), abi.Context(0)
        for c in (self.a, self.b):
            c.upload_space(WORLD, self.model)
            c.set_options(WORLD, abi.make_options(**self.opts))
            if self.has_ui:
                c.upload_space(UI, self.ui_model)
                c.set_options(UI, abi.make_options(bloom_intensity=0.0, **self.ui_opts))
        self.in_flight = {}     # slot -> [(device buffer, expected bytes, expected steps)]
        self.light_kw = None    # the parameters of the update pending on a's worker
        self.uncollected = None  # b's info of an update that a has published and not yet reported
        self.resident = [device_bytes(96 * 64 * 12), device_bytes(96 * 64 * 12)]
        self.cur = 0
        self.size = None        # R's (w, h)
        self.r_host = None      # R's bytes
        self.r_cam = None
        self.splat = None       # (w, h, R of reproject_ref) of the last reprojection
        self.pick = None        # (device list, host copy) of the most recent pick
        self.light_cubes = np.zeros((0, 3), np.int32)
        self.font = None
        self.orders = {}
        self.checked = collections.Counter()

    def close(self):
        self.a.close()
        self.b.close()

    # -- cameras ---------------------------------------------------------------------------------------------------------------------
    def matrices(self, cam, w, h):
        return oracle.camera_matrices(cam["fov"], self.opts["view_distance"], w / h, oracle.look_at_y_up(cam["eye"], cam["target"]), cam["eye"])

    def ui_inv(self, w, h):
        return oracle.camera_matrices(90.0, self.ui_opts["view_distance"], w / h, (0, 0, 0, 1), UI_EYE)[2] if self.has_ui else None

    def frame(self, w, h, cam, out="rgba8", part=None, exchanging=False):
        return abi.Context.make_frame(w, h, world_inv=self.matrices(cam, w, h)[2], ui_inv=self.ui_inv(w, h), partition=part, flags=FLAGS[out],
                                      tuning=abi.tuning(variant=abi.VARIANT_EXCHANGING) if exchanging else 0)

    def view_projection(self, cam, w, h):
        p, w2e, _ = self.matrices(cam, w, h)
        return (w2e @ p).reshape(16).copy()  # euclid's row-vector matrices, view.then(projection), read column-major

    def ipzw(self, cam, w, h):
        ip = np.linalg.inv(self.matrices(cam, w, h)[0])
        return np.array([ip[2, 2], ip[3, 2], ip[2, 3], ip[3, 3]], np.float32)

    def order(self, kind, w, h):
        """(device tensor or None, host array or None) of the picker's order"""
        if kind != "picker":
            return None, None
        if (w, h) not in self.orders:
            host = abi.pixel_order(w, h)[0]
            self.orders[(w, h)] = (to_device(host), host)
        return self.orders[(w, h)]

    # -- the light update on the worker -------------------------------------------------------------------------------------------------
    def before(self, kind):
        """In front of a call that publishes a's pending update: the twin makes the same update now, blocking."""
        if self.light_kw is not None and kind in sp.PUBLISHING:
            self.uncollected = self.b.evaluate_light(WORLD, fast=False, queue=[], **self.light_kw)
            self.light_kw = None

    def collect_light(self):
        """Behind it: a's report of the update (the call itself has published it) is the blocking one's."""
        if self.uncollected is not None:
            ia, ib = self.a.evaluate_light_wait(WORLD), self.uncollected
            self.uncollected = None
            assert (ia.updates, ia.queue_left) == (ib.updates, ib.queue_left), "the worker's light update differs from the blocking one"

    # -- frame traffic ---------------------------------------------------------------------------------------------------------------
    def submit(self, p):
        frames = [self.frame(p["w"], p["h"], cam, p["out"], p["part"], p["exchanging"]) for cam in p["cams"]]
        items = []
        for f in frames:
            ref = self.b.render(f)  # the twin draws it now: what the scene stands for at this moment
            want = result_bytes(ref).copy()
            items.append((device_bytes(len(want)), want, int(ref["info"].cubes_traced)))
        if len(frames) == 1:
            self.a.render_submit(frames[0], items[0][0].data_ptr(), p["slot"])
        else:
            self.a.render_submit_batch(frames, [it[0].data_ptr() for it in items], p["slot"])
        self.in_flight[p["slot"]] = items

    def collect(self, slot):
        items = self.in_flight.pop(slot)
        infos = [self.a.render_wait(slot)] if len(items) == 1 else self.a.render_wait_batch(slot, len(items))
        for (buf, want, steps), info in zip(items, infos):
            got = read_back(buf, len(want), f"the frame of slot {slot}")
            assert (got == want).all(), f"slot {slot} differs from the frame at submit time in {int((got != want).sum())} bytes"
            assert int(info.cubes_traced) == steps, f"slot {slot}: cubes_traced"
            self.checked["streamed frame"] += 1

    # -- scene and light calls -------------------------------------------------------------------------------------------------------
    def both(self, fn):
        fn(self.a)
        self.collect_light()
        fn(self.b)

    def light_volume(self, seed):
        rng = np.random.default_rng(seed)
        size = tuple(self.model.size)
        light = rng.integers(0, 256, size + (4,)).astype(np.uint8)
        light[..., 3] = rng.choice([1, 128, 255, 255], size)
        return light

    def scene_call(self, kind, p):
        m = self.model
        if kind in ("update_cubes", "light_submit", "light_blocking"):
            xyz, blocks = np.array(p["xyz"], np.int32), np.array(p["blocks"], np.uint16)
            light = np.array(p["light"], np.uint8) if p.get("light") else None
            self.both(lambda c: c.update_cubes(WORLD, xyz, blocks, light))
            for i, cube in enumerate(xyz):
                q = tuple(int(v) - int(l) for v, l in zip(cube, m.lo))
                if all(0 <= v < s for v, s in zip(q, m.size)):
                    m.block_index[q] = blocks[i]
            if kind != "update_cubes":
                kw = dict(maximum_distance=p["maximum_distance"], max_updates=p["max_updates"], batch=p["batch"])
                self.both(lambda c: c.light_cubes_changed(WORLD, xyz))
                if kind == "light_submit":
                    self.a.evaluate_light_submit(WORLD, fast=False, queue=[], **kw)
                    self.light_kw = kw
                else:
                    ia, ib = (c.evaluate_light(WORLD, fast=False, queue=[], **kw) for c in (self.a, self.b))
                    assert (ia.updates, ia.queue_left) == (ib.updates, ib.queue_left)
        elif kind == "replace_block":
            block = block_of(p["block"])
            self.both(lambda c: c.replace_block(WORLD, p["index"], block))
            if p["index"] == len(m.blocks):
                m.blocks.append(block)
            else:
                m.blocks[p["index"]] = block
        elif kind == "compact":
            self.both(lambda c: c.compact(WORLD))
        elif kind == "update_light_volume":
            light = self.light_volume(p["seed"])
            self.both(lambda c: c.update_light_volume(WORLD, light))
        elif kind == "set_options":
            self.opts.update(fog=p["fog"], lighting=p["lighting"], antialiasing=p["antialiasing"], bloom_intensity=p["bloom_intensity"])
            self.both(lambda c: c.set_options(WORLD, abi.make_options(**self.opts)))
        elif kind == "set_depth_transform":
            proj = oracle.camera_matrices(90.0, p["view_distance"], 1.5)[0]
            zw = (1.0, 0.0, 0.0, 1.0) if p["which"] == "linear" else (proj[2, 2], proj[3, 2], proj[2, 3], proj[3, 3])
            self.both(lambda c: c.set_depth_transform(zw))
        elif kind == "upload_world":
            self.model = workloads.synthetic_space(n=p["n"], resolution=8, n_blocks=6, seed=p["seed"], light="field")
            self.model.lo = tuple(p["lo"])
            self.both(lambda c: c.upload_space(WORLD, self.model))
            self.light_cubes = np.zeros((0, 3), np.int32)
        elif kind == "clear_ui":
            self.both(lambda c: c.clear_space(UI))
            self.ui_model = None
        elif kind == "upload_ui":
            self.ui_model = ui_space(p["variant"])
            self.both(lambda c: c.upload_space(UI, self.ui_model))
        elif kind == "light_changed_count":
            # no update is waited for: where a's is pending the twin, which has not made it yet, answers for the same published volume
            (na, ba), (nb, bb) = self.a.light_changed(WORLD, take=False), self.b.light_changed(WORLD, take=False)
            assert na == nb and (ba == bb).all(), f"light_changed count: {na} {ba.tolist()} against the twin's {nb} {bb.tolist()}"
            self.checked[kind] += 1
        else:
            assert kind == "light_changed_take", kind
            xa, ba = self.a.light_changed(WORLD, take=True)
            self.collect_light()
            xb, bb = self.b.light_changed(WORLD, take=True)
            assert xa.shape == xb.shape and (xa == xb).all() and (ba == bb).all(), f"light_changed take: {len(xa)} cubes against the twin's {len(xb)}"
            self.light_cubes = xa.copy()
            self.checked[kind] += 1

    # -- slot 0 between the streamed frames ---------------------------------------------------------------------------------------------
    def render(self, p):
        w, h, out = p["w"], p["h"], p["out"]
        f = self.frame(w, h, p["cam"], out, exchanging=p["exchanging"])
        ref = self.b.render(f)
        want = result_bytes(ref)
        if out == "resident":
            for t in self.resident:
                t.fill_(SENTINEL)
            import torch
            torch.cuda.synchronize()
            buf = self.resident[self.cur]
        else:
            buf = device_bytes(len(want))
        info = self.a.render_to_device(f, buf.data_ptr())
        got = read_back(buf, len(want), "the frame")
        assert (got == want).all(), f"{int((got != want).sum())} bytes differ from the twin's frame"
        assert info.cubes_traced == ref["info"].cubes_traced
        if out == "resident":
            self.size, self.r_host, self.r_cam = (w, h), got.copy(), p["cam"]
            if self.pick is not None and self.pick[2] != (w, h):
                self.pick = None

    def trace_rays(self, p):
        space = self.ui_model if p["layer"] == UI else self.model
        rays = make_rays(p["n"], p["seed"], space.lo, space.size)
        flags = FLAGS[p["out"]]
        ref = self.b.trace_rays(p["layer"], rays, include_sky=not p["no_sky"], flags=flags, want_aux=p["aux"])
        want = result_bytes(ref)
        if p["device"]:
            out = device_bytes(len(want))
            aux = to_device(np.zeros(p["n"], abi.PIXEL_AUX_DTYPE)) if p["aux"] else None
            info = self.a.trace_rays_device(p["layer"], p["n"], to_device(rays).data_ptr(), out.data_ptr(), aux.data_ptr() if p["aux"] else 0, include_sky=not p["no_sky"], flags=flags)
            got = read_back(out, len(want), "the rays' results")
            got_aux = aux.cpu().numpy().view(abi.PIXEL_AUX_DTYPE) if p["aux"] else None
        else:
            r = self.a.trace_rays(p["layer"], rays, include_sky=not p["no_sky"], flags=flags, want_aux=p["aux"])
            got, got_aux, info = result_bytes(r), r["aux"], r["info"]
        assert (got == want).all(), f"{int((got != want).sum())} bytes differ from the twin's rays"
        assert info.cubes_traced == ref["info"].cubes_traced and info.rows_rendered == p["n"]
        assert not p["aux"] or same_fields(got_aux, ref["aux"]), "first-hit records"

    def trace_patches(self, p):
        rng = np.random.default_rng(p["seed"])
        lo = rng.uniform(-1.0, 0.9, (p["n"], 2))
        rects = np.concatenate([lo, lo + rng.uniform(0.001, 0.2, (p["n"], 2))], 1)
        f = self.frame(p["w"], p["h"], p["cam"], p["out"])
        ra, rb = self.a.trace_patches(f, rects), self.b.trace_patches(f, rects)
        assert (result_bytes(ra) == result_bytes(rb)).all() and ra["info"].cubes_traced == rb["info"].cubes_traced

    def ortho(self, p):
        ra, rb = self.a.render_orthographic(p["layer"], p["resolution"]), self.b.render_orthographic(p["layer"], p["resolution"])
        assert ra["rgba8"].shape == rb["rgba8"].shape and (ra["rgba8"] == rb["rgba8"]).all() and ra["info"].cubes_traced == rb["info"].cubes_traced

    def trace_pixels(self, p):
        w, h, n = p["w"], p["h"], p["n"]
        f = self.frame(w, h, p["cam"], p["out"])
        if p["source"] == "pick":
            listed_dev, listed, _ = self.pick
            assert len(listed) == n
        else:
            listed = np.random.default_rng(p["seed"]).integers(0, w * h, n).astype(np.uint32)
            listed_dev = to_device(listed)
        ref = self.b.trace_pixels(f, listed, want_aux=bool(p.get("aux")))
        if p["mode"] == "in_place":
            assert (w, h) == self.size
            count = w * h
            want = self.r_host.copy()
            want[:count * 8].view(np.uint64)[listed] = np.ascontiguousarray(ref["color_f16"]).view(np.uint64).reshape(-1)
            want[count * 8:count * 12].view(np.uint32)[listed] = np.ascontiguousarray(ref["depth"]).view(np.uint32)
            info = self.a.trace_pixels_device(f, n, listed_dev.data_ptr(), self.resident[self.cur].data_ptr(), in_place=True)
            got = read_back(self.resident[self.cur], count * 12, "R")
            assert (got == want).all(), f"R differs in {int((got != want).sum())} bytes after an in-place trace of {n} pixels"
            self.r_host = got.copy()
        else:
            want = result_bytes(ref)
            out = device_bytes(len(want))
            aux = to_device(np.zeros(n, abi.PIXEL_AUX_DTYPE)) if p.get("aux") else None
            info = self.a.trace_pixels_device(f, n, listed_dev.data_ptr(), out.data_ptr(), aux.data_ptr() if aux is not None else 0)
            got = read_back(out, len(want), "the pixels' results")
            assert (got == want).all(), f"{int((got != want).sum())} bytes differ from the twin's pixels"
            assert aux is None or same_fields(aux.cpu().numpy().view(abi.PIXEL_AUX_DTYPE), ref["aux"]), "first-hit records"
        assert info.cubes_traced == ref["info"].cubes_traced and info.rows_rendered == n
        assert (listed_dev.cpu().numpy().view(np.uint32)[:n] == listed).all(), "the list changed"

    # -- the Split-frame operations on R: `a` alone, against the restatements ------------------------------------------------------------
    def planes(self):
        """(colour [h, w, 4] uint16, depth [h, w] float32) of R's bytes"""
        w, h = self.size
        n = w * h
        return self.r_host[:n * 8].view(np.uint16).reshape(h, w, 4), self.r_host[n * 8:n * 12].view(np.float32).reshape(h, w)

    def r_unchanged(self):
        w, h = self.size
        assert (read_back(self.resident[self.cur], w * h * 12, "R") == self.r_host).all(), "R changed under an operation that only reads it"

    def reproject(self, p):
        w, h = self.size
        color, depth = self.planes()
        old_inv = self.matrices(self.r_cam, w, h)[2]
        m = (old_inv @ self.view_projection(p["cam"], w, h).reshape(4, 4)).reshape(16).astype(np.float32)
        zw = self.ipzw(p["cam"], w, h)
        flags = abi.REPROJECT_KEEP_SPLATS if p["keep"] else 0
        want = reproject_ref.reproject(color, depth, m, zw, flags)
        src, dst = self.resident[self.cur], self.resident[1 - self.cur]
        dst.fill_(SENTINEL)
        import torch
        torch.cuda.synchronize()
        info = self.a.reproject_split(w, h, m, zw, src.data_ptr(), dst.data_ptr(), flags)
        self.r_unchanged()
        got = read_back(dst, w * h * 12, "the reprojected frame")
        n = w * h
        got_color, got_depth = got[:n * 8].view(np.uint16).reshape(h, w, 4), got[n * 8:].view(np.uint32).reshape(h, w)
        assert (got_depth == want["D"].view(np.uint32)).all(), f"{int((got_depth != want['D'].view(np.uint32)).sum())} depths differ from the restatement"
        assert (got_color == want["color"]).all(), f"{int((got_color != want['color']).any(-1).sum())} colour texels differ from the restatement"
        assert (info.n_splats, info.n_dropped, info.n_gaps, info.n_unfilled) == (want["n_splats"], want["n_dropped"], want["n_gaps"], want["n_unfilled"])
        assert (info.levels, tuple(info.t0)) == (want["levels"], want["t0"])
        self.cur, self.r_host, self.r_cam, self.splat = 1 - self.cur, got.copy(), p["cam"], (w, h, want["R"])  # the two buffers swap roles

    def picked(self, p, call, want, want_info, fields):
        """One pick into a fresh sentinel-filled list: the list, the info and the guard words are the restatement's."""
        n = p["n"]
        out = device_bytes(4 * n)
        info = call(out.data_ptr())
        got = read_back(out, 4 * n, "pixels_out").view(np.uint32)
        assert {k: getattr(info, k) for k in fields} == {k: want_info[k] for k in fields}, ({k: getattr(info, k) for k in fields}, want_info)
        assert (got == want).all(), f"{int((got != want).sum())} of {n} entries differ from the restatement"
        self.r_unchanged()
        self.pick = (out, got.copy(), self.size)

    def pick_pixels(self, p):
        w, h = self.size
        order_dev, order = self.order(p["order"], w, h)
        known = self.splat[2] if p["max_unknown"] else None
        assert known is None or self.splat[:2] == (w, h)
        want, want_info = pick_ref.pick_list(w * h, order, p["n"], R=known, max_unknown=p["max_unknown"], skip_unknown=p["skip"], cursor=p["cursor"])
        self.picked(p, lambda out: self.a.pick_pixels(w, h, p["n"], order_dev.data_ptr() if order_dev is not None else 0, out, cursor=p["cursor"], max_unknown=p["max_unknown"],
                                                      skip_unknown=p["skip"]), want, want_info, ("n_unknown", "next_cursor", "n_from_unknown", "n_from_order"))

    def pick_stale(self, p):
        w, h = self.size
        order_dev, order = self.order(p["order"], w, h)
        color, depth = self.planes()
        rects = abi.stale_rects(self.view_projection(self.r_cam, w, h), w, h, np.array(p["boxes"], np.int32).reshape(-1, 6), 1)
        flags = abi.STALE_DEPTH_TEST if p["depth_test"] else 0
        want, want_info = stale_ref.pick_list(w, h, order, p["n"], rect_list=rects, color_bits=color, depth=depth, flags=flags, max_stale=p["max_stale"], skip_stale=p["skip"],
                                              cursor=p["cursor"])
        self.picked(p, lambda out: self.a.pick_stale(w, h, p["n"], rects, self.resident[self.cur].data_ptr(), order_dev.data_ptr() if order_dev is not None else 0, out,
                                                     cursor=p["cursor"], max_stale=p["max_stale"], skip_stale=p["skip"], flags=flags), want, want_info,
                    ("n_stale", "next_cursor", "n_from_stale", "n_from_order"))

    def pick_stale_cubes(self, p):
        w, h = self.size
        order_dev, order = self.order(p["order"], w, h)
        color, depth = self.planes()
        vp = self.view_projection(self.r_cam, w, h)
        boxes, cubes = np.array(p["boxes"], np.int32).reshape(-1, 6), self.light_cubes[:MAX_LIGHT_CUBES]
        want, want_info = stale_cubes_ref.pick_list(vp, w, h, order, p["n"], boxes=boxes, light_cubes=cubes, expand=1, color_bits=color, depth=depth, flags=p["flags"],
                                                    max_stale=p["max_stale"], skip_stale=p["skip"], cursor=p["cursor"])
        self.picked(p, lambda out: self.a.pick_stale_cubes(vp, w, h, p["n"], boxes, cubes, self.resident[self.cur].data_ptr(), order_dev.data_ptr() if order_dev is not None else 0,
                                                           out, cursor=p["cursor"], max_stale=p["max_stale"], skip_stale=p["skip"], flags=p["flags"]), want, want_info,
                    ("n_stale", "next_cursor", "n_from_stale", "n_from_order", "n_rects", "whole_frame"))

    def presented(self, p, call, want):
        """One presentation into a sentinel-filled device image or a host one: the image is the restatement's."""
        ow, oh = p["out"]
        dtype = np.uint16 if p["f16"] else np.uint8
        n_bytes = ow * oh * 4 * np.dtype(dtype).itemsize
        if p["device"]:
            out = device_bytes(n_bytes)
            result = call(out.data_ptr())
            got = read_back(out, n_bytes, "the presented image").view(dtype).reshape(oh, ow, 4)
        else:
            result = call(None)
            got = result[0]
        info = result[1]
        levels, t0 = abi.bloom_geometry(ow, oh)
        assert got.dtype == want.dtype and (got == want).all(), f"{int((got != want).any(-1).sum())} of {ow * oh} pixels differ from the restatement"
        assert (info.bloomed, info.levels, tuple(info.t0)) == (int(p["case"][0] > 0), levels, t0), (info.bloomed, info.levels, tuple(info.t0))
        self.r_unchanged()
        return result

    def present(self, p):
        color, _ = self.planes()
        want = present_ref.present(color, p["out"], *p["case"], out_f16=p["f16"])
        flags = abi.PRESENT_OUT_F16 if p["f16"] else 0
        self.presented(p, lambda out: self.a.present_split(self.resident[self.cur].data_ptr(), self.size, p["out"], *p["case"], flags=flags, out_device=out), want)

    def present_lines(self, p):
        color, depth = self.planes()
        vertices, m = line_vertices(p["n_lines"], p["seed"]), np.eye(4, dtype=np.float32).reshape(16)
        want, counts = present_lines_ref.present(color, depth.view(np.uint32), p["out"], vertices, m, *p["case"], out_f16=p["f16"])
        flags = abi.PRESENT_OUT_F16 if p["f16"] else 0
        on_device = to_device(vertices)
        _, _, lines_info = self.presented(p, lambda out: self.a.present_split_lines(self.resident[self.cur].data_ptr(), self.size, p["out"], *p["case"], m,
                                                                                    on_device.data_ptr() if p["device"] else vertices, p["n_lines"], flags=flags, out_device=out), want)
        assert {k: getattr(lines_info, k) for k in present_lines_ref.COUNTS} == counts, "the line counts"

    def present_text(self, p):
        ow, oh = p["out"]
        color, depth = self.planes()
        cell, atlas = self.font
        cols, rows, scale, origin = abi.text_geometry((float(ow), float(oh)), cell)
        codes = text_grid(cols, rows, p["corner"], p["seed"])
        layer = present_text_ref.text_layer(ow, oh, atlas, cell, codes, scale, origin)
        s = present_ref.scene(color, ow, oh)
        vertices, m, counts = None, None, dict.fromkeys(present_lines_ref.COUNTS, 0)
        if p["n_lines"]:
            vertices, m = line_vertices(p["n_lines"], p["seed"]), np.eye(4, dtype=np.float32).reshape(16)
            s, counts = present_lines_ref.draw(s, depth.view(np.uint32), vertices, m)
        bloom = present_ref.chain(s) if p["case"][0] > 0 else None
        want = present_text_ref.composite(s, bloom, *p["case"], out_f16=p["f16"], text=layer)
        flags = abi.PRESENT_OUT_F16 if p["f16"] else 0
        codes_dev = to_device(codes)
        text = ((codes_dev.data_ptr(), cols, rows) if p["device"] else codes, scale, origin)
        _, _, lines_info = self.presented(p, lambda out: self.a.present_split_text(self.resident[self.cur].data_ptr(), self.size, p["out"], *p["case"], text=text, view_projection=m,
                                                                                   vertices=vertices, flags=flags, out_device=out), want)
        assert {k: getattr(lines_info, k) for k in present_lines_ref.COUNTS} == counts, "the line counts"

    def export(self, p):
        ow, oh = p["out"]
        color, depth = self.planes()
        zw = self.ipzw(self.r_cam, *self.size)
        want_c, want_z, want_stats = export_ref.export(color, depth, zw, p["out"])
        n = ow * oh
        bufs = [device_bytes(GUARD + n * 4) if wanted else None for wanted in (p["color"], p["depth"])]
        ptrs = [b.data_ptr() + GUARD if b is not None else 0 for b in bufs]
        _, _, info = self.a.export_split(self.resident[self.cur].data_ptr(), self.size, p["out"], zw, device_outs=ptrs)
        raws = [b.cpu().numpy() if b is not None else None for b in bufs]
        for raw in raws:
            assert raw is None or ((raw[:GUARD] == SENTINEL).all() and (raw[GUARD + n * 4:] == SENTINEL).all()), "guard bytes around an exported plane"
        assert raws[0] is None or (raws[0][GUARD:GUARD + n * 4].reshape(oh, ow, 4) == want_c).all(), "exported colour"
        assert raws[1] is None or same_depth_bits(raws[1][GUARD:GUARD + n * 4].view(np.float32).reshape(oh, ow), want_z), "exported depth"
        got_stats = (info.n_surface, np.float32(info.depth_min).view(np.uint32), np.float32(info.depth_max).view(np.uint32))
        assert got_stats == (want_stats[0], np.float32(want_stats[1]).view(np.uint32), np.float32(want_stats[2]).view(np.uint32)), (got_stats, want_stats)
        self.r_unchanged()

    # -- the ray queries ------------------------------------------------------------------------------------------------------------
    def ray_query(self, kind, p):
        space = self.ui_model if p["layer"] == UI else self.model
        rays, n = make_rays(p["n"], p["seed"], space.lo, space.size), p["n"]
        luminance = kind == "sample_luminance"
        item = 4 if luminance else abi.CURSOR_HIT_DTYPE.itemsize
        if p["device"]:
            out = to_device(np.zeros(n * item, np.uint8)) if not luminance else device_bytes(n * item)
            rays_dev = to_device(rays)
            if luminance:
                self.a.sample_luminance_device(p["layer"], n, rays_dev.data_ptr(), p["max_steps"], out.data_ptr())
                got = read_back(out, n * item, "the samples").view(np.float32)
            else:
                self.a.cursor_raycast_device(p["layer"], n, rays_dev.data_ptr(), p["maximum_distance"], out.data_ptr())
                got = out.cpu().numpy().view(abi.CURSOR_HIT_DTYPE)
        else:
            got = self.a.sample_luminance(p["layer"], rays, p["max_steps"]) if luminance else self.a.cursor_raycast(p["layer"], rays, p["maximum_distance"])
        self.collect_light()
        want = self.b.sample_luminance(p["layer"], rays, p["max_steps"]) if luminance else self.b.cursor_raycast(p["layer"], rays, p["maximum_distance"])
        if luminance:
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {n} samples differ from the twin's"
        else:
            assert (field_bytes(got) == field_bytes(want)).all(), f"{int((field_bytes(got) != field_bytes(want)).any(1).sum())} of {n} cursor records differ from the twin's"

    # -- a slot-0 call while a frame occupies slot 0 ---------------------------------------------------------------------------------------
    def refused(self, p):
        kind, a = p["kind"], self.a
        w, h = self.size if self.size is not None else (17, 9)
        cam = self.r_cam if self.r_cam is not None else {"eye": (8.5, 14.5, 26.0), "target": (8.0, 5.0, 8.0), "fov": 90.0}
        out = device_bytes(96 * 64 * 16)
        host = np.full((4, 4, 4), SENTINEL, np.uint8)
        r_ptr = self.resident[self.cur].data_ptr()
        other = self.resident[1 - self.cur]
        other_before = other.cpu().numpy().copy()
        f = self.frame(w, h, cam)
        rays = to_device(make_rays(8, p["seed"], self.model.lo, self.model.size))
        listed = to_device(np.arange(min(8, w * h), dtype=np.uint32))
        m = np.eye(4, dtype=np.float32).reshape(16)
        rect = np.array([[-0.5, -0.5, 0.5, 0.5]])
        calls = {
            "render": lambda: a.render_to_device(f, out.data_ptr()),
            "trace_rays": lambda: a.trace_rays_device(WORLD, 8, rays.data_ptr(), out.data_ptr()),
            "trace_patches": lambda: a._check(a._lib.aic_trace_patches(a._h, f, 1, rect.ctypes.data, host.ctypes.data, None, abi.FrameInfo())),
            "trace_pixels": lambda: a.trace_pixels_device(self.frame(w, h, cam, "split"), min(8, w * h), listed.data_ptr(), r_ptr, in_place=True),
            "ortho": lambda: a.render_orthographic(WORLD, 1),
            "reproject": lambda: a.reproject_split(w, h, m, self.ipzw(cam, w, h), r_ptr, other.data_ptr()),
            "pick_pixels": lambda: a.pick_pixels(w, h, 8, 0, out.data_ptr()),
            "pick_stale": lambda: a.pick_stale(w, h, 8, abi.stale_rects(self.view_projection(cam, w, h), w, h, [self.model.lo + self.model.hi]), r_ptr, 0, out.data_ptr(), max_stale=8),
            "pick_stale_cubes": lambda: a.pick_stale_cubes(self.view_projection(cam, w, h), w, h, 8, [self.model.lo + self.model.hi], None, r_ptr, 0, out.data_ptr(), max_stale=8),
            "present": lambda: a.present_split(r_ptr, (w, h), (w, h), 0.125, 0, np.inf, out_device=out.data_ptr()),
            "present_lines": lambda: a.present_split_lines(r_ptr, (w, h), (w, h), 0.125, 0, np.inf, m, line_vertices(3, 1), out_device=out.data_ptr()),
            "present_text": lambda: a.present_split_text(r_ptr, (w, h), (w, h), 0.0, 0, np.inf, text=(np.full((1, 1), 65, np.uint8), (1.0, 1.0), (0.0, 0.0)), out_device=out.data_ptr()),
            "export": lambda: a.export_split(r_ptr, (w, h), (w, h), self.ipzw(cam, w, h), device_outs=(out.data_ptr(), out.data_ptr() + 96 * 64 * 4)),
        }
        try:
            calls[kind]()
            code = None
        except abi.AicError as e:
            code = e.code
        assert code == AIC_ERR_INVALID, f"{kind} with a frame on slot 0 was not refused with AIC_ERR_INVALID: {code}"
        assert (out.cpu().numpy() == SENTINEL).all() and (host == SENTINEL).all(), f"a refused {kind} wrote to its output"
        assert (other.cpu().numpy() == other_before).all(), f"a refused {kind} wrote to the other Split buffer"
        if self.size is not None:
            self.r_unchanged()

    # -- the checkpoint ----------------------------------------------------------------------------------------------------------------
    def checkpoint(self):
        for slot in sorted(self.in_flight):
            self.collect(slot)
        self.collect_light()  # (the plan counts a checkpoint among the publishing calls: the twin has made the update)
        self.a.synchronize()
        m = self.model
        light = self.a.read_light_volume(WORLD, tuple(m.size))
        assert (light == self.b.read_light_volume(WORLD, tuple(m.size))).all(), "the light volume differs from the twin's"
        grid, cls, tagged = self.a.probe_cube_grid(WORLD, m.size, len(m.blocks))
        want = cube_tags_ref.tagged_grid(m)
        d = cube_tags_ref.diff(grid, want, cube_tags_ref.is_tagged(m))
        assert not cube_tags_ref.n_differences(d) and (grid == want).all(), ("the cube grid differs from the host model's", d)
        assert (cls == cube_tags_ref.cls_words(m.blocks)).all() and tagged == cube_tags_ref.is_tagged(m), "the class table"
        m.light[...] = light
        w, h = 64, 48
        cam = {"eye": tuple(float(l + s * f) for l, s, f in zip(m.lo, m.size, (0.53, 0.9, 1.62))), "target": tuple(float(l + s * f) for l, s, f in zip(m.lo, m.size, (0.5, 0.31, 0.5))),
               "fov": 90.0}
        inv = self.matrices(cam, w, h)[2]
        o = self.opts
        opt = oracle.make_options(fog=o["fog"], transparency=o["transparency"], lighting=o["lighting"], antialiasing=o["antialiasing"], view_distance=o["view_distance"])
        ui = {}
        if self.ui_model is not None:
            u = self.ui_opts
            ui = dict(ui=oracle.Space(self.ui_model), ui_opt=oracle.make_options(fog=u["fog"], transparency=u["transparency"], lighting=u["lighting"], view_distance=u["view_distance"]),
                      ui_cam=oracle.make_camera(self.ui_inv(w, h), w, h))
        ref = oracle.render(oracle.Space(m), opt, oracle.make_camera(inv, w, h), want_linear=True, **ui)
        got = self.a.render(self.frame(w, h, cam, "linear"))["rgba8"]
        bad = (got.view(np.uint32) != ref["linear"].view(np.uint32)).any(-1)
        assert not bad.any(), f"{int(bad.sum())} of {w * h} pixels of the checkpoint's linear frame differ from the oracle's of the host model"
        self.checked["checkpoint"] += 1

    def call(self, kind, p):
        self.before(kind)
        if kind == "submit":
            self.submit(p)
        elif kind == "checkpoint":
            self.checkpoint()
        elif kind == "collect":
            self.collect(p["slot"])
        elif kind in sp.SCENE_CALLS:
            self.scene_call(kind, p)
        elif kind == "set_text_font":
            atlas = font(tuple(p["cell"]), p["blank"], p["seed"])
            self.a.set_text_font(atlas, *p["cell"])
            self.font = (tuple(p["cell"]), atlas)
        elif kind in sp.RAY_QUERIES:
            self.ray_query(kind, p)
        elif kind == "refused":
            self.refused(p)
        else:
            getattr(self, kind)(p)
        if kind in sp.CHECKED_KINDS or kind == "refused":
            self.checked[kind] += 1


@pytest.mark.parametrize("seed,n_calls", CASES)
def test_sessions_against_a_synchronous_twin_and_the_restatements(seed, n_calls):
    calls = sp.plan(seed, n_calls)
    s = Session(seed)
    try:
        for i, kind, p, st in sp.walk(calls, s.has_ui):
            try:
                assert sorted(st.in_flight) == sorted(s.in_flight) and st.pending == (s.light_kw is not None), "the plan's state is not the session's"
                s.call(kind, p)
                if i + 1 == len(calls) and kind != "checkpoint":
                    s.call("checkpoint", {})
            except (AssertionError, abi.AicError) as e:
                if isinstance(e, abi.AicError) and e.code == AIC_ERR_DEVICE:
                    pytest.exit(f"seed {seed}, call {i} ({kind}): the device reported an error, nothing more is started on it: {e}", returncode=3)
                recent = "\n".join(f"  {j}: {calls[j][0]} {calls[j][1]}" for j in range(max(0, i - 19), i + 1))
                raise AssertionError(f"seed {seed}, call {i} ({kind}; replay with AIC_SESSION_FUZZ_ONLY={seed}:{i + 1}): {e}\nthe last calls of the plan:\n{recent}") from e
        print(f"seed {seed}: checked {dict(sorted(s.checked.items()))}")
        TOTALS.update(s.checked)
        print(f"checked so far, all seeds: {dict(sorted(TOTALS.items()))}")
        assert sum(s.checked.values()) > n_calls // 3
    finally:
        s.close()
