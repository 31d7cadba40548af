"""The call plan of tests/test_gpu_session_fuzz.py, made without a device: `plan(seed, n_calls)` is the sequence of calls of one interactive
session as plain tuples (kind, parameters) drawn from np.random.default_rng -- sizes, cameras, slots, flags, list lengths, cube coordinates, block
choices, light parameters, which pick feeds which trace. Nothing in it depends on what a device answers, so tests/test_session_plan_cpu.py can show
from the plans of the default seeds alone that they meet the cases they are there for, and `plan(seed, n)` is a prefix of `plan(seed, m)` for n < m.

The planner keeps the protocol's state as far as the protocol alone decides it (`State`): which slots hold a frame, whether a light update is
pending on the worker, the size of the resident Split frame R and of the last reprojection, the boxes changed since the last stale pick. It
collects a slot before it submits on it again, frees slot 0 before work that runs there, and occupies it before a call that must be refused.
`walk(calls)` replays that state over any list of calls: (index, kind, parameters, state before the call)."""
import copy

import numpy as np

# frames and resident Split frames: the smallest shapes of the per-operation tests; (33, 17) is a resident size only, for its stretch
FRAME_SIZES = [(1, 1), (3, 5), (17, 9), (61, 37), (64, 48), (96, 64)]
RESIDENT_SIZES = FRAME_SIZES + [(33, 17)]
STRETCH = {(3, 5): (7, 11), (64, 48): (40, 30), (33, 17): (65, 31)}
SLOTS = 10
RAY_COUNTS = [1, 63, 64, 65, 257]
LINE_COUNTS = [1, 28, 65]
TEXT_CELLS = [(9, 18, 1), (5, 7, 0)]
PRESENT_CASES = [(0.0, 0, float("inf")), (0.0, 1, 1.0), (0.125, 0, float("inf")), (0.25, 1, 1.0)]  # (bloom_intensity, tone_mapping, maximum_intensity)
FRAME_KINDS = ["rgba8", "no_feedback", "split", "bloom", "linear"]
RENDER_KINDS = ["rgba8", "linear", "colorbuf", "split", "resident", "resident"]  # `resident`: a Split frame left in device memory as R
WORLD, UI = 0, 1
N_BLOCKS_0 = 11  # workloads.synthetic_space(n_blocks=6): air, four atoms, six recursive blocks
MAX_BOXES = 24
CHECKPOINT_EVERY = 30  # calls between two checkpoints; the session ends with one more

FRAME_TRAFFIC = ("submit", "collect")
SCENE_CALLS = ("update_cubes", "replace_block", "compact", "update_light_volume", "set_options", "set_depth_transform", "light_submit", "light_blocking",
               "light_changed_count", "light_changed_take", "upload_world", "clear_ui", "upload_ui")
LISTED_TRACES = ("trace_rays", "trace_patches", "trace_pixels")
SLOT0_WORK = ("render",) + LISTED_TRACES + ("ortho",)
SPLIT_OPS = ("reproject", "pick_pixels", "pick_stale", "pick_stale_cubes", "present", "present_lines", "present_text", "export")
RAY_QUERIES = ("sample_luminance", "cursor_raycast")
SLOT0_KINDS = SLOT0_WORK + SPLIT_OPS  # everything that queues on slot 0's stream and is refused while a frame occupies it
CHECKED_KINDS = SLOT0_KINDS + RAY_QUERIES
ALL_KINDS = FRAME_TRAFFIC + SCENE_CALLS + SLOT0_KINDS + RAY_QUERIES + ("set_text_font", "refused", "checkpoint")
# INTEGRATION.md "Threads" and include/aic_hip.h: the calls that end a pending light update and publish it before they do anything else. Frames, the
# listed traces, the Split-frame operations, aic_set_options and aic_light_changed_count do not.
PUBLISHING = ("update_cubes", "replace_block", "compact", "update_light_volume", "set_depth_transform", "light_submit", "light_blocking",
              "light_changed_take", "upload_world", "clear_ui", "upload_ui", "sample_luminance", "cursor_raycast", "checkpoint")
SCENE_DECK = ["update_cubes", "update_cubes", "replace_block", "replace_block", "compact", "update_light_volume", "set_options", "set_depth_transform", "light_submit",
              "light_submit", "light_blocking", "light_changed_count", "light_changed_take", "light_changed_take"]
SCENE_WRITES = ("update_cubes", "replace_block", "compact", "update_light_volume", "set_depth_transform", "upload_world", "clear_ui", "upload_ui")


class State:
    """What the protocol alone decides."""

    def __init__(self, has_ui):
        self.in_flight = {}          # slot -> the submit's parameters
        self.pending = False         # a light update runs on the worker and is not published
        self.has_ui = has_ui         # the seed uses the UI layer: every frame carries a UI camera
        self.ui_present = has_ui
        self.lo, self.n = (0, 0, 0), 16
        self.n_blocks = N_BLOCKS_0
        self.resident = None         # (w, h) of R
        self.resident_cam = None
        self.reproject_size = None   # the size of the context's last aic_reproject_split
        self.last_pick = None        # (w, h, n) of the most recent pick, while R keeps that size
        self.boxes = []              # the boxes changed since the last stale pick
        self.antialiasing = 0

    def others_in_flight(self):
        return [s for s in self.in_flight if s != 0]

    def apply(self, kind, p):
        if kind == "submit":
            self.in_flight[p["slot"]] = p
        elif kind == "checkpoint":  # everything in flight is collected, the light read back
            self.in_flight.clear()
        elif kind == "collect":
            del self.in_flight[p["slot"]]
        if kind == "light_submit":
            self.pending = True
        elif kind in PUBLISHING:
            self.pending = False
        if kind in ("update_cubes", "light_submit", "light_blocking"):
            self.boxes += [[x, y, z, x + 1, y + 1, z + 1] for x, y, z in p["xyz"]]
        elif kind == "replace_block":
            self.boxes.append(self.whole_box())
            self.n_blocks = max(self.n_blocks, p["index"] + 1)
        elif kind == "upload_world":
            self.lo, self.n, self.n_blocks = tuple(p["lo"]), p["n"], N_BLOCKS_0
            self.boxes = [self.whole_box()]
        elif kind == "clear_ui":
            self.ui_present = False
        elif kind == "upload_ui":
            self.ui_present = True
        elif kind == "set_options":
            self.antialiasing = p["antialiasing"]
        elif kind == "render" and p["out"] == "resident":
            if self.resident != (p["w"], p["h"]):
                self.last_pick = None
            self.resident, self.resident_cam = (p["w"], p["h"]), p["cam"]
        elif kind == "reproject":
            self.reproject_size, self.resident_cam = self.resident, p["cam"]
        elif kind in ("pick_pixels", "pick_stale", "pick_stale_cubes"):
            self.last_pick = self.resident + (p["n"],)
            if kind != "pick_pixels":
                self.boxes = []
        if len(self.boxes) > MAX_BOXES:
            self.boxes = [self.whole_box()]

    def whole_box(self):
        return [*self.lo, *(v + self.n for v in self.lo)]


def walk(calls, has_ui):
    """(index, kind, parameters, a copy of the state before the call) of every call"""
    st = State(has_ui)
    for i, (kind, p) in enumerate(calls):
        before = copy.copy(st)
        before.in_flight = dict(st.in_flight)
        before.boxes = list(st.boxes)
        yield i, kind, p, before
        st.apply(kind, p)


def seed_has_ui(seed):
    return seed % 2 == 1


def size_of(kind, p, st):
    """The figure a call's scratch is sized by: the list length of a listed trace, the pixels of R for what reads it, those of the output for what
    writes an image."""
    if kind in LISTED_TRACES:
        return p["n"]
    if kind in ("present", "present_lines", "present_text", "export"):
        return p["out"][0] * p["out"][1]
    return st.resident[0] * st.resident[1]


class _Planner:
    def __init__(self, seed):
        self.rng = np.random.default_rng(77000 + seed)
        self.seed = seed
        self.st = State(seed_has_ui(seed))
        self.calls = []
        self.refuse_next = 4 * seed  # the kinds take turns, each seed from another start
        self.uploads = 0
        self.last_size = {}
        self.deck = []
        self.turns = {}

    # -- drawing parameters ------------------------------------------------------------------------------------------------------------------
    def pick(self, items):
        return items[int(self.rng.integers(0, len(items)))]

    def turn(self, key, items):
        """The items in turn, from a start the seed draws: a short plan meets every one of them"""
        if key not in self.turns:
            self.turns[key] = int(self.rng.integers(0, len(items)))
        self.turns[key] += 1
        return items[self.turns[key] % len(items)]

    def other_size(self, key, sizes):
        """A size of `sizes` that differs from the one `key` drew last: consecutive calls of one operation change size, up and down."""
        choices = [s for s in sizes if s != self.last_size.get(key)]
        s = self.pick(choices)
        self.last_size[key] = s
        return s

    def camera(self):
        r, st = self.rng, self.st
        n, lo = st.n, st.lo
        eye = tuple(float(lo[a] + n * f) for a, f in enumerate((0.53 + r.uniform(-0.31, 0.31), 0.9 + r.uniform(-0.19, 0.25), 1.62 + r.uniform(-0.37, 0.37))))
        target = tuple(float(lo[a] + n * f) for a, f in enumerate((0.5, 0.31, 0.5)))
        return {"eye": eye, "target": target, "fov": float(self.pick([60.0, 90.0]))}

    def moved(self, cam):
        d = self.rng.uniform(-0.6, 0.6, 3)
        return {"eye": tuple(float(e + v) for e, v in zip(cam["eye"], d)), "target": cam["target"], "fov": cam["fov"]}

    def cubes(self, n, margin, outside=False):
        """n distinct cubes (a batch that names a cube twice with two values has no defined order), `margin` cubes inside the bounds -- or with
        cubes beside the bounds among them"""
        st, r = self.st, self.rng
        lo, hi = margin, st.n - margin
        if outside:
            lo, hi = -2, st.n + 2
        seen = {}
        while len(seen) < n:
            c = tuple(int(st.lo[a] + r.integers(lo, hi)) for a in range(3))
            seen[c] = None
        return [list(c) for c in seen]

    # -- emitting ----------------------------------------------------------------------------------------------------------------------------
    def emit(self, call, **p):
        self.calls.append((call, p))
        self.st.apply(call, p)

    def free_slot0(self):
        if 0 in self.st.in_flight:
            self.emit("collect", slot=0)

    def submit(self, slot=None, kind=None, size=None, count=None):
        r = self.rng
        slot = int(r.integers(0, SLOTS)) if slot is None else slot
        if slot in self.st.in_flight:
            self.emit("collect", slot=slot)
        kind = self.pick(FRAME_KINDS) if kind is None else kind
        w, h = self.other_size("submit", FRAME_SIZES) if size is None else size
        count = int(self.pick([1, 1, 1, 2, 4])) if count is None else count
        part = None
        if kind in ("rgba8", "no_feedback", "split") and h >= 9 and r.random() < 0.3:
            n_parts = int(r.integers(2, 4))
            part = (8, n_parts, int(r.integers(0, n_parts)))
        self.emit("submit", slot=slot, out=kind, w=w, h=h, count=count, part=part, exchanging=bool(r.random() < 0.3), cams=[self.camera() for _ in range(count)],
                  ui=self.st.has_ui)

    def ensure_resident(self):
        if self.st.resident is None:
            self.render(out="resident")

    def render(self, out=None, size=None):
        self.free_slot0()
        out = self.pick(RENDER_KINDS) if out is None else out
        w, h = self.other_size("resident", RESIDENT_SIZES) if out == "resident" and size is None else self.other_size("render", FRAME_SIZES) if size is None else size
        self.emit("render", out=out, w=w, h=h, cam=self.camera(), exchanging=bool(self.rng.random() < 0.3))

    def trace_rays(self):
        self.free_slot0()
        st, r = self.st, self.rng
        layer = UI if st.ui_present and r.random() < 0.5 else WORLD
        self.emit("trace_rays", layer=layer, n=self.other_size("trace_rays", RAY_COUNTS + [700]), seed=int(r.integers(1 << 30)), device=bool(r.random() < 0.5),
                  no_sky=bool(r.random() < 0.4), aux=bool(r.random() < 0.4), out=self.pick(["rgba8", "colorbuf", "linear"]))

    def trace_patches(self):
        self.free_slot0()
        w, h = self.pick(FRAME_SIZES)
        self.emit("trace_patches", w=w, h=h, cam=self.camera(), n=self.other_size("trace_patches", [1, 7, 64, 65, 300]), seed=int(self.rng.integers(1 << 30)),
                  out=self.pick(["rgba8", "linear"]))

    def trace_pixels(self, size=None):
        self.free_slot0()
        st, r = self.st, self.rng
        seed = int(r.integers(1 << 30))
        in_place = size is None and st.resident is not None and r.random() < 0.6
        if in_place:
            w, h = st.resident
            from_pick = st.last_pick is not None and st.last_pick[:2] == (w, h) and r.random() < 0.6
            n = st.last_pick[2] if from_pick else self.other_size("trace_pixels", [1, 5, 64, 65, 300])
            self.emit("trace_pixels", mode="in_place", source="pick" if from_pick else "plan", w=w, h=h, n=n, seed=seed, cam=st.resident_cam, out="split")
        else:
            w, h = self.pick(FRAME_SIZES) if size is None else size
            self.emit("trace_pixels", mode="compact", source="plan", w=w, h=h, n=self.other_size("trace_pixels", [1, 5, 64, 65, 300]), seed=seed, cam=self.camera(),
                      out=self.pick(["rgba8", "linear", "split"]), aux=bool(r.random() < 0.3))

    def ortho(self):
        self.free_slot0()
        self.emit("ortho", layer=UI if self.st.ui_present and self.rng.random() < 0.3 else WORLD, resolution=int(self.other_size("ortho", [1, 2, 4])))

    def out_size(self, key):
        """The resident frame's own size, its stretch where it has one, or any size of the set -- never the size the operation wrote last"""
        src = self.st.resident
        choices = [src, src] + ([STRETCH[src]] * 2 if src in STRETCH else []) + [self.pick(FRAME_SIZES)]
        choices = [s for s in choices if s != self.last_size.get(key)] or [s for s in FRAME_SIZES if s != self.last_size.get(key)]
        s = self.pick(choices)
        self.last_size[key] = s
        return s

    def new_resident_sometimes(self, p=0.35):
        """The Split-frame operations follow R's size: a new R of another size in front of some of them"""
        if self.st.resident is None or self.rng.random() < p:
            self.render(out="resident")

    def split_op(self, kind):
        st, r = self.st, self.rng
        self.new_resident_sometimes()
        self.free_slot0()
        w, h = st.resident
        count = w * h
        pick_common = dict(n=int(self.pick([1, 7, 64, 65, 200])), cursor=int(self.pick([0, 3, max(count // 2 - 1, 0), 2 ** 40 + 3])), order=self.pick(["picker", "row_major"]))
        if kind == "reproject":
            self.emit("reproject", cam=self.moved(st.resident_cam), keep=bool(r.random() < 0.5))
        elif kind == "pick_pixels":
            known = st.reproject_size == (w, h)
            self.emit("pick_pixels", max_unknown=int(self.pick([0, 5, count])) if known else 0, skip=int(self.pick([0, 0, 2])) if known else 0, **pick_common)
        elif kind == "pick_stale":
            self.emit("pick_stale", boxes=[list(b) for b in st.boxes], max_stale=int(self.pick([0, 5, count])), skip=int(self.pick([0, 0, 2])), depth_test=bool(r.random() < 0.5),
                      **pick_common)
        elif kind == "pick_stale_cubes":
            self.emit("pick_stale_cubes", boxes=[list(b) for b in st.boxes], max_stale=int(self.pick([5, count, count])), skip=int(self.pick([0, 0, 2])),
                      flags=int(self.turn("stale_cubes flags", [0, 1, 2, 3])), **pick_common)
        elif kind == "present":
            self.emit("present", out=self.out_size("present"), case=self.pick(PRESENT_CASES), f16=bool(r.random() < 0.5), device=bool(r.random() < 0.7))
        elif kind == "present_lines":
            self.emit("present_lines", out=self.out_size("present_lines"), case=self.pick(PRESENT_CASES), f16=bool(r.random() < 0.5), n_lines=int(self.turn("n_lines", LINE_COUNTS)),
                      device=bool(r.random() < 0.5), seed=int(r.integers(1 << 30)))
        elif kind == "present_text":
            if r.random() < 0.5:
                self.emit("set_text_font", cell=self.other_size("font", TEXT_CELLS), blank=bool(r.random() < 0.5), seed=int(r.integers(1 << 10)))
            self.emit("present_text", out=self.out_size("present_text"), case=self.pick(PRESENT_CASES), f16=bool(r.random() < 0.5), n_lines=int(self.pick([0, 0, 1, 28])),
                      device=bool(r.random() < 0.5), corner=bool(r.random() < 0.5), seed=int(r.integers(1 << 30)))
        else:
            assert kind == "export", kind
            self.emit("export", out=self.out_size("export"), color=bool(r.random() < 0.85), depth=bool(r.random() < 0.85))

    def ray_query(self, kind=None):
        st, r = self.st, self.rng
        kind = self.pick(RAY_QUERIES) if kind is None else kind
        common = dict(layer=UI if st.ui_present and r.random() < 0.3 else WORLD, n=int(self.turn(kind, RAY_COUNTS)), device=bool(r.random() < 0.5), seed=int(r.integers(1 << 30)))
        if kind == "sample_luminance":
            self.emit(kind, max_steps=int(self.pick([0, 16, 60])), **common)
        else:
            self.emit(kind, maximum_distance=float(self.pick([6.0, 40.0, float("inf")])), **common)

    def light_params(self):
        return dict(maximum_distance=int(self.pick([4, 8])), max_updates=int(self.pick([0, 40, 200])), batch=int(self.pick([32, 256])))

    def light_update(self, blocking):
        n = int(self.rng.integers(1, 6))
        self.emit("light_blocking" if blocking else "light_submit", xyz=self.cubes(n, 1), blocks=[int(v) for v in self.rng.integers(0, self.st.n_blocks, n)], **self.light_params())

    def scene(self, kind=None):
        st, r = self.st, self.rng
        if kind is None:  # the kinds are dealt from a shuffled deck, so that the rare ones come up in every seed
            if not self.deck:
                self.deck = [SCENE_DECK[i] for i in r.permutation(len(SCENE_DECK))]
            kind = self.deck.pop()
        if kind == "update_cubes":
            n = int(r.integers(1, 12))
            with_light = bool(r.random() < 0.5)
            light = [[int(v) for v in r.integers(0, 256, 3)] + [int(self.pick([1, 128, 255]))] for _ in range(n)] if with_light else None
            self.emit(kind, xyz=self.cubes(n, 0, outside=bool(r.random() < 0.4)), blocks=[int(v) for v in r.integers(0, st.n_blocks, n)], light=light)
        elif kind == "replace_block":
            index = st.n_blocks if st.n_blocks < N_BLOCKS_0 + 3 and r.random() < 0.25 else int(r.integers(1, st.n_blocks))
            if r.random() < 0.5:
                block = ("atom", [float(v) for v in r.random(3)] + [float(self.pick([1.0, 0.5]))])
            else:
                block = ("voxels", int(r.integers(1, 1 << 30)), bool(r.random() < 0.5))
            self.emit(kind, index=index, block=block)
        elif kind in ("compact", "light_changed_count", "light_changed_take"):
            self.emit(kind)
        elif kind == "update_light_volume":
            self.emit(kind, seed=int(r.integers(1 << 30)))
        elif kind == "set_options":
            self.emit(kind, fog=int(r.integers(0, 4)), lighting=int(r.integers(0, 5)), antialiasing=int(self.pick([0, 2])), bloom_intensity=float(self.pick([0.0, 0.125, 0.25])))
        elif kind == "set_depth_transform":
            self.emit(kind, which=self.pick(["linear", "projection"]), view_distance=float(self.pick([30.0, 200.0])))
        else:
            self.light_update(blocking=kind == "light_blocking")

    def upload_world(self):
        """A re-upload of the world at another size and a negative lower corner, with a light update pending and frames in flight"""
        r = self.rng
        self.light_update(blocking=False)
        self.submit(slot=int(r.integers(1, SLOTS)))
        self.uploads += 1
        self.emit("upload_world", n=int(self.pick([12, 20]) if self.st.n == 16 else 16), lo=[int(v) for v in r.integers(-9, -1, 3)], seed=int(r.integers(1, 1000)))

    def refused(self):
        """A slot-0 call while a submitted frame occupies slot 0; the kinds take turns"""
        kind = SLOT0_KINDS[self.refuse_next % len(SLOT0_KINDS)]
        self.refuse_next += 1
        if kind in SPLIT_OPS or kind == "trace_pixels":
            self.ensure_resident()
        if 0 not in self.st.in_flight:
            self.submit(slot=0, count=1)
        self.emit("refused", kind=kind, seed=int(self.rng.integers(1 << 30)))

    def motif(self):
        """The sequences a random draw meets too rarely"""
        r = self.rng
        which = int(r.integers(0, 6))
        if which == 0:  # a listed trace, shaped into an image by batch_image, then a whole frame of the same width on slot 0
            size = self.pick(FRAME_SIZES[2:])
            self.trace_pixels(size=size)
            self.render(out=self.pick(["rgba8", "split", "linear"]), size=size)
        elif which == 1:
            size = self.pick(FRAME_SIZES[1:])
            self.render(out="rgba8", size=size)
            self.trace_rays()
            self.render(out="rgba8", size=size)
        elif which == 2:  # a bloomed frame, then an unbloomed one of the same size on the same slot
            slot, size = int(r.integers(0, SLOTS)), self.pick(FRAME_SIZES[1:])
            self.submit(slot=slot, kind="bloom", size=size, count=1)
            self.submit(slot=slot, kind="rgba8", size=size, count=1)
        elif which == 3:  # a publishing call as the first call after a submit
            self.submit()
            what = self.pick(["sample_luminance", "cursor_raycast", "light_changed_take", "scene"])
            if what in RAY_QUERIES:
                self.ray_query(what)
            elif what == "scene":
                self.scene(self.pick(list(SCENE_WRITES[:5])))
            else:
                self.scene(what)
        elif which == 4:  # checked calls with a light update pending and frames in flight
            self.light_update(blocking=False)
            self.submit(slot=int(r.integers(1, SLOTS)))
            for _ in range(2):
                self.step(checked_only=True)
        elif self.st.ui_present:  # rays on the UI layer (traced in the world's seat) beside frames that carry a UI camera
            self.submit(slot=int(r.integers(1, SLOTS)))
            self.free_slot0()
            self.emit("trace_rays", layer=UI, n=self.other_size("trace_rays", RAY_COUNTS), seed=int(r.integers(1 << 30)), device=bool(r.random() < 0.5), no_sky=False, aux=False,
                      out="rgba8")

    def step(self, checked_only=False):
        st, r = self.st, self.rng
        u = r.random() if not checked_only else r.uniform(0.44, 0.86)
        if u < 0.13:
            self.submit()
        elif u < 0.19:
            if st.in_flight:
                self.emit("collect", slot=int(self.pick(sorted(st.in_flight))))
        elif u < 0.44:
            self.scene()
        elif u < 0.58:
            kind = self.pick(["render", "render", "trace_rays", "trace_rays", "trace_patches", "ortho", "trace_pixels", "trace_pixels"])
            getattr(self, kind)()
        elif u < 0.80:
            self.split_op(self.pick(list(SPLIT_OPS)))
        elif u < 0.86:
            self.ray_query()
        elif u < 0.925:
            self.refused()
        else:
            self.motif()


def plan(seed, n_calls):
    """The first n_calls calls of seed's session: [(kind, parameters)]."""
    p = _Planner(seed)
    p.emit("set_text_font", cell=TEXT_CELLS[0], blank=True, seed=0)
    next_upload = 35 + int(p.rng.integers(0, 20))
    next_ui = 60 + int(p.rng.integers(0, 20))
    next_checkpoint = CHECKPOINT_EVERY
    while len(p.calls) < n_calls:
        if len(p.calls) >= next_checkpoint:
            p.emit("checkpoint")
            next_checkpoint = len(p.calls) + CHECKPOINT_EVERY
        elif len(p.calls) >= next_upload:
            p.upload_world()
            next_upload += 75 + int(p.rng.integers(0, 20))
        elif p.st.has_ui and len(p.calls) >= next_ui:
            p.emit("clear_ui")
            p.emit("upload_ui", variant=int(p.rng.integers(0, 2)))
            next_ui += 80 + int(p.rng.integers(0, 30))
        else:
            p.step()
    return p.calls[:n_calls]
