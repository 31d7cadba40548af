"""(no device needed) The plans tests/test_gpu_session_fuzz.py executes are not vacuous: from the plans of the default seeds alone -- tests/session_plan.py
draws them without a device -- every call kind occurs, the checked calls meet frames in flight and pending light updates, sizes go up and down, and
the sequences the fuzz is there for (a listed trace shaped into an image and then a whole frame of that width on slot 0, a bloomed frame followed by an
unbloomed one on its slot, rays in the world's seat beside frames with a UI camera, a world re-upload under frames and a pending update) all happen.
These are conditions on the plan: they are met by tuning its weights or raising the default number of calls, never by lowering them."""
import collections
import os

from tests import session_plan as sp

N_SEEDS = int(os.environ.get("AIC_SESSION_FUZZ_N", "6"))
N_CALLS = int(os.environ.get("AIC_SESSION_FUZZ_CALLS", "160"))
DEFAULT_SEEDS, DEFAULT_CALLS = 6, 160
ONCE_PER_SEED = ("upload_world", "clear_ui", "upload_ui")  # the scene's own events, not weighted call kinds: once or twice per seed


def walks():
    """[(seed, [(index, kind, parameters, state before)])] of the default plans"""
    return [(seed, list(sp.walk(sp.plan(seed, DEFAULT_CALLS), sp.seed_has_ui(seed)))) for seed in range(DEFAULT_SEEDS)]


def test_the_environment_defaults_are_the_plans_checked_here():
    if "AIC_SESSION_FUZZ_N" not in os.environ and "AIC_SESSION_FUZZ_CALLS" not in os.environ:
        assert (N_SEEDS, N_CALLS) == (DEFAULT_SEEDS, DEFAULT_CALLS)


def test_a_plan_is_a_pure_function_of_its_seed_and_a_prefix_of_a_longer_one():
    a, b, longer = sp.plan(3, 90), sp.plan(3, 90), sp.plan(3, 400)
    assert repr(a) == repr(b) and repr(longer[:90]) == repr(a) and len(longer) == 400
    assert repr(sp.plan(4, 90)) != repr(a)


def test_the_plan_keeps_the_protocol():
    """A slot is collected before it is submitted on again; slot 0 is free for what runs there and occupied for a refused call; a list that comes
    from a pick has that pick's length and R still has its size; unknown pixels are asked for only after a reprojection of R's size."""
    for seed, w in walks():
        for i, kind, p, st in w:
            what = (seed, i, kind)
            if kind == "submit":
                assert p["slot"] not in st.in_flight and p["ui"] == st.has_ui, what
            elif kind == "collect":
                assert p["slot"] in st.in_flight, what
            elif kind in sp.SLOT0_KINDS:
                assert 0 not in st.in_flight, what
            elif kind == "refused":
                assert 0 in st.in_flight and p["kind"] in sp.SLOT0_KINDS, what
                assert st.resident is not None or p["kind"] not in sp.SPLIT_OPS + ("trace_pixels",), what
            if kind in sp.SPLIT_OPS:
                assert st.resident is not None, what
            if kind == "trace_pixels" and p["source"] == "pick":
                assert st.last_pick == (p["w"], p["h"], p["n"]) and st.resident == (p["w"], p["h"]), what
            if kind == "pick_pixels" and p["max_unknown"]:
                assert st.reproject_size == st.resident, what
            if kind == "trace_rays" and p["layer"] == sp.UI or kind in sp.RAY_QUERIES + ("ortho",) and p["layer"] == sp.UI:
                assert st.ui_present, what
            if kind in ("update_cubes", "light_submit", "light_blocking"):
                assert len({tuple(c) for c in p["xyz"]}) == len(p["xyz"]) == len(p["blocks"]) and max(p["blocks"]) < st.n_blocks, what


def test_every_call_kind_occurs():
    counts = collections.Counter()
    refused = collections.Counter()
    for seed, w in walks():
        here = collections.Counter(kind for _, kind, _, _ in w)
        counts += here
        refused += collections.Counter(p["kind"] for _, kind, p, _ in w if kind == "refused")
        assert 1 <= here["upload_world"] <= 2, (seed, here["upload_world"])
        if sp.seed_has_ui(seed):
            assert here["upload_ui"] >= 1 and here["clear_ui"] - here["upload_ui"] in (0, 1), seed  # (1: the plan ends between the two)
    print(sorted(counts.items()))
    for kind in sp.ALL_KINDS:
        if kind not in ONCE_PER_SEED:
            assert counts[kind] >= 8, (kind, counts[kind])
    for kind in sp.SLOT0_KINDS:
        assert refused[kind] >= 1, ("never refused", kind)
    # the parameters that select another path of a call
    seen = collections.defaultdict(set)
    for _, w in walks():
        for _, kind, p, _ in w:
            for key in ("out", "device", "mode", "source", "keep", "no_sky", "aux", "layer", "n_lines", "n", "count", "f16", "flags", "depth_test", "order"):
                if key in p and kind != "refused":
                    seen[(kind, key)].add(p[key] if not isinstance(p[key], list) else tuple(p[key]))
    assert seen[("submit", "out")] == set(sp.FRAME_KINDS) and seen[("submit", "count")] == {1, 2, 4}
    assert seen[("render", "out")] == set(sp.RENDER_KINDS)
    assert seen[("trace_rays", "device")] == {True, False} and seen[("trace_rays", "layer")] == {sp.WORLD, sp.UI}
    assert seen[("trace_rays", "no_sky")] == {True, False} and seen[("trace_rays", "aux")] == {True, False}
    assert seen[("trace_pixels", "mode")] == {"compact", "in_place"} and seen[("trace_pixels", "source")] == {"plan", "pick"}
    assert seen[("reproject", "keep")] == {True, False}
    assert seen[("present_lines", "n_lines")] == set(sp.LINE_COUNTS) and seen[("present_lines", "device")] == {True, False}
    for kind in sp.RAY_QUERIES:
        assert seen[(kind, "n")] == set(sp.RAY_COUNTS) and seen[(kind, "device")] == {True, False} and seen[(kind, "layer")] == {sp.WORLD, sp.UI}, kind
    assert seen[("pick_stale_cubes", "flags")] == {0, 1, 2, 3} and seen[("pick_stale", "depth_test")] == {True, False}
    stretched = {(st.resident, tuple(p["out"])) for _, w in walks() for _, kind, p, st in w if kind in ("present", "present_lines", "present_text", "export")}
    for src, out in sp.STRETCH.items():
        assert (src, out) in stretched, (src, out)
    fonts = [p["cell"] for _, w in walks() for _, kind, p, _ in w if kind == "set_text_font"]
    assert len(set(map(tuple, fonts))) == len(sp.TEXT_CELLS)


def test_checked_calls_meet_frames_in_flight_and_pending_updates():
    checked = with_frames = with_pending = 0
    for _, w in walks():
        for _, kind, p, st in w:
            if kind in sp.CHECKED_KINDS:
                checked += 1
                with_frames += bool(st.others_in_flight())
                with_pending += st.pending
    print(f"checked {checked}, with frames in flight on other slots {with_frames}, with a light update pending {with_pending}")
    assert 3 * with_frames >= checked
    assert with_pending >= 10


def test_sizes_change_both_ways():
    """Every Split-frame operation and every listed trace is called at least once at a size smaller and once at a size larger than its previous call."""
    up, down = collections.Counter(), collections.Counter()
    for _, w in walks():
        last = {}
        for _, kind, p, st in w:
            if kind in sp.SPLIT_OPS + sp.LISTED_TRACES:
                size = sp.size_of(kind, p, st)
                if kind in last:
                    up[kind] += size > last[kind]
                    down[kind] += size < last[kind]
                last[kind] = size
    for kind in sp.SPLIT_OPS + sp.LISTED_TRACES:
        assert up[kind] >= 1 and down[kind] >= 1, (kind, up[kind], down[kind])


def test_publishing_calls_come_first_after_a_submit():
    first = collections.Counter()
    for _, w in walks():
        for (_, before, _, _), (_, kind, _, _) in zip(w, w[1:]):
            if before == "submit":
                first[kind] += 1
    for kind in sp.RAY_QUERIES + ("light_changed_take",):
        assert first[kind] >= 1, kind
    assert sum(first[k] for k in sp.SCENE_WRITES) >= 1


def test_the_sequences_on_slot_0_and_on_one_slot():
    pixels_then_render = render_rays_render = bloom_then_plain = 0
    for _, w in walks():
        slot0 = [(kind, p) for _, kind, p, _ in w if kind in sp.SLOT0_KINDS]
        for (k0, p0), (k1, p1) in zip(slot0, slot0[1:]):
            pixels_then_render += k0 == "trace_pixels" and k1 == "render" and p0["w"] == p1["w"]
        for (k0, _), (k1, _), (k2, _) in zip(slot0, slot0[1:], slot0[2:]):
            render_rays_render += (k0, k1, k2) == ("render", "trace_rays", "render")
        last = {}
        for _, kind, p, _ in w:
            if kind == "submit":
                before = last.get(p["slot"])
                bloom_then_plain += before is not None and before["out"] == "bloom" and p["out"] != "bloom" and (before["w"], before["h"]) == (p["w"], p["h"])
                last[p["slot"]] = p
    assert pixels_then_render >= 1 and render_rays_render >= 1 and bloom_then_plain >= 1, (pixels_then_render, render_rays_render, bloom_then_plain)


def test_ui_rays_beside_frames_with_a_ui_camera():
    n = sum(1 for _, w in walks() for _, kind, p, st in w
            if kind == "trace_rays" and p["layer"] == sp.UI and any(f["ui"] for s, f in st.in_flight.items() if s != 0))
    assert n >= 1


def test_world_reuploads_under_frames_and_a_pending_update():
    n = sum(1 for _, w in walks() for _, kind, _, st in w if kind == "upload_world" and st.others_in_flight() and st.pending)
    assert n >= 1
    assert all(min(p["lo"]) < 0 and p["n"] != st.n for _, w in walks() for _, kind, p, st in w if kind == "upload_world")
