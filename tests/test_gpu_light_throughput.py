"""GPU tests (-m gpu) of the light updater in the configurations bench.py and a sim loop run: batches of
thousands of queue entries in first-in-first-out order, the relight loop's budgeted calls that continue the layer's queue, and
random scenes at those batch sizes. The oracle pops the same `batch` entries, computes them against one light state and applies
them in pop order, as aic_evaluate_light does, so at every batch size and order the device must give the oracle's bytes: the
light volume, the update count, the summed ComputedLight::cost and the queue left -- compared exactly, never within a tolerance.

Which kernel a case reaches (csrc/aic_light.hip launch_compute_light_waves): lanes_per_cube 1 is compute_light_kernel; a batch
that launches more than 256 waves (257 cubes and up) is compute_light_wave_kernel_dense, and then every wave walks several cubes
once the batch exceeds the resident waves (n_cus x per_cu); smaller launches are compute_light_wave_kernel_ldsq; and
compute_light_wave_kernel is the walk with its queue in global memory: maximum_distance 255 (its LDS queue does not fit), and
the child process started with AIC_LIGHT_GLOBAL_QUEUE."""
import copy
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi, flat, workloads
from tests import scenes
from tests.test_gpu_light_update import _random_light_scene

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))  # the oracle's compute_light calls of a batch (results unchanged)


def atrium_lamp_space():
    """bench.py's relight scene: the atrium with the lamp block added (the last block index) and its light cleared."""
    sp = workloads.atrium_like_space()
    sp.add_block(flat.atom((1.0, 0.9, 0.7, 1.0), (8.0, 7.0, 5.0), name="lamp"))
    sp.light[...] = 0
    return sp


def light_bench_space():
    sp = scenes.light_bench_space()
    sp.light[...] = 0
    return sp


SCENES = {"fog": scenes.fog_test_space, "light_bench": light_bench_space, "atrium_lamp": atrium_lamp_space}


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


_oracle_cache = {}


def oracle_fast(name, batch, order, maximum_distance=30, max_updates=1 << 62):
    """fast_evaluate_light + evaluate_light(1) in the oracle: (light volume, updates, cost, queue left), cached per configuration."""
    key = (name, batch, order, maximum_distance, max_updates)
    if key not in _oracle_cache:
        with oracle.LightSession(SCENES[name](), maximum_distance, hb_width=order, threads=THREADS) as s:
            n, cost, left = s.evaluate(fast=True, epsilon=1, batch=batch, max_updates=max_updates)
            _oracle_cache[key] = (s.light(), n, cost, left)
    return _oracle_cache[key]


def assert_same(info, got, want, what=""):
    vol, n, cost, left = want
    bad = (got != vol.reshape(got.shape)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} texels differ, first at {np.argwhere(bad)[:4].tolist()}"
    assert info.updates == n, f"{what}: updates {info.updates} != {n}"
    assert info.queue_left == left, f"{what}: queue_left {info.queue_left} != {left}"
    assert info.cost == cost, f"{what}: cost {info.cost} != {cost}"


def device_fast(c, name, batch, order, lanes, maximum_distance=30, max_updates=0, dep_pool_chunks=0):
    sp = SCENES[name]()
    c.upload_space(abi.LAYER_WORLD, sp)
    info = c.evaluate_light(abi.LAYER_WORLD, maximum_distance, fast=True, epsilon=1, batch=batch, queue_order=order, lanes_per_cube=lanes,
                            max_updates=max_updates, dep_pool_chunks=dep_pool_chunks)
    return info, c.read_light_volume(abi.LAYER_WORLD, sp.size)


@pytest.mark.parametrize("name,batch,order,lanes", [
    ("light_bench", 8192, 0, 256),   # bench.py's throughput line
    ("light_bench", 2048, 16, 64),
    ("light_bench", 65, 0, 1),
    ("fog", 257, 0, 256),
    ("fog", 2048, 0, 1),
    ("fog", 8192, 16, 64),
    ("fog", 65, 16, 256),
    ("atrium_lamp", 8192, 0, 256),   # bench.py's relight starting light
    ("atrium_lamp", 2048, 16, 64),
    ("atrium_lamp", 257, 0, 1),
])
def test_throughput_batches_match_the_oracle(ctx, name, batch, order, lanes):
    info, got = device_fast(ctx, name, batch, order, lanes)
    want = oracle_fast(name, batch, order)
    assert want[1] > batch  # several batches
    assert_same(info, got, want, f"{name} batch {batch} order {order} lanes {lanes}")
    assert info.batches >= (want[1] + batch - 1) // batch


@pytest.mark.parametrize("name,batch", [("light_bench", 2048), ("fog", 8192)])
def test_dependency_pool_grows_at_throughput_batches(name, batch):
    """A fresh context started with a four-chunk dependency pool (aic_light_params.hooks): the first large batch overflows it on the
    copying result path, the pool grows and the batch is computed again -- with the oracle's result."""
    with abi.Context(0) as c:
        info, got = device_fast(c, name, batch, 0, 256, dep_pool_chunks=4)
    assert_same(info, got, oracle_fast(name, batch, 0), f"{name} batch {batch}, pool of 4 chunks")


def test_maximum_distance_255_with_an_update_limit(ctx):
    """The full chart: one resident wave per CU, so batch 2048 makes every wave walk several cubes; max_updates stops after three
    batches with the queue still full."""
    info, got = device_fast(ctx, "light_bench", 2048, 0, 256, maximum_distance=255, max_updates=6144)
    want = oracle_fast("light_bench", 2048, 0, maximum_distance=255, max_updates=6144)
    assert want[1] == 6144 and want[3] > 0
    assert_same(info, got, want, "distance 255")


def _global_queue_child():
    """Run in a child process with AIC_LIGHT_GLOBAL_QUEUE set (read once per process): the walk keeps its queue in global memory
    (compute_light_wave_kernel) for launches of up to 256 waves; still the oracle's bytes."""
    with abi.Context(0) as c:
        for batch, order in ((32, 16), (2048, 0)):
            info, got = device_fast(c, "fog", batch, order, 256)
            assert_same(info, got, oracle_fast("fog", batch, order), f"global queue, batch {batch}")
            print(f"global queue batch {batch}: {info.updates} updates in {info.batches} launches, equal to the oracle")


def test_global_queue_kernel_in_a_child_process():
    env = dict(os.environ, AIC_LIGHT_GLOBAL_QUEUE="1")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_light_throughput import _global_queue_child as f; f()"],
                       cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("equal to the oracle") == 2


# bench.py's relight loop: a lamp toggled every 10 steps, every step one call with a budget that equals its batch. The budgets
# mix bench's 2048, the carry of one and two lagging steps (4096, 6144) and two small batches.
RELIGHT_BUDGETS = [2048, 2048, 4096, 2048, 6144, 48, 257, 2048, 2048, 4096]
RELIGHT_STEPS = 90


def _relight_sites(sp):
    """bench.py SceneLoop's lamp sites: 30 air cubes drawn with default_rng(7)."""
    size = np.array(sp.size)
    air = next(i for i, b in enumerate(sp.blocks) if b.is_air)
    bi = np.asarray(sp.block_index)
    rng = np.random.default_rng(7)
    sites = []
    while len(sites) < 30:
        c = rng.integers(0, size)
        if int(bi[tuple(c)]) == air and tuple(c) not in sites:
            sites.append(tuple(int(v) for v in c))
    return [tuple(int(l + c) for l, c in zip(sp.lo, s)) for s in sites], air


def _relight_change(step, sites, air, lamp):
    """Every 10 steps a change at bench's sites: event j places the lamp at site j // 2 and event j + 1 removes it again."""
    if step % 10:
        return None
    j = step // 10
    return sites[j // 2], (lamp if j % 2 == 0 else air)


def test_relight_loop_matches_the_oracle_session():
    sp = atrium_lamp_space()
    lamp = len(sp.blocks) - 1
    sites, air = _relight_sites(sp)
    # the oracle's run: the starting light, then every step's (volume, updates, cost, queue left)
    with oracle.LightSession(sp, 30, hb_width=0, threads=THREADS) as s:
        n0, cost0, left0 = s.evaluate(fast=True, epsilon=1, batch=8192)
        start = (s.light(), n0, cost0, left0)
        want = []
        for i in range(RELIGHT_STEPS):
            ch = _relight_change(i, sites, air, lamp)
            if ch:
                s.set_cubes([ch[0]], [ch[1]])
            n_b = RELIGHT_BUDGETS[i % len(RELIGHT_BUDGETS)]
            n, cost, left = s.evaluate(fast=False, epsilon=1, batch=n_b, max_updates=n_b)
            want.append((s.light(), n, cost, left))
    assert sum(w[1] for w in want) > 10000 and any(w[3] > 0 for w in want), "the loop never lagged behind its queue"

    def run(blocking):
        with abi.Context(0) as c:
            c.upload_space(abi.LAYER_WORLD, sp)
            info = c.evaluate_light(abi.LAYER_WORLD, 30, fast=True, epsilon=1, batch=8192, queue_order=0)
            assert_same(info, c.read_light_volume(abi.LAYER_WORLD, sp.size), start, "starting light")
            pending = None
            for i in range(RELIGHT_STEPS):
                if pending is not None:
                    info = c.evaluate_light_wait(abi.LAYER_WORLD)
                    assert_same(info, c.read_light_volume(abi.LAYER_WORLD, sp.size), want[pending], f"worker thread, step {pending}")
                    pending = None
                ch = _relight_change(i, sites, air, lamp)
                if ch:
                    c.update_cubes(abi.LAYER_WORLD, [ch[0]], [ch[1]])
                    c.light_cubes_changed(abi.LAYER_WORLD, [ch[0]], queue_order=0)
                n_b = RELIGHT_BUDGETS[i % len(RELIGHT_BUDGETS)]
                if blocking:
                    info = c.evaluate_light(abi.LAYER_WORLD, 30, fast=False, epsilon=1, batch=n_b, queue_order=0, queue=[], max_updates=n_b)
                    assert_same(info, c.read_light_volume(abi.LAYER_WORLD, sp.size), want[i], f"blocking, step {i}")
                else:
                    c.evaluate_light_submit(abi.LAYER_WORLD, 30, fast=False, epsilon=1, batch=n_b, queue_order=0, queue=[], max_updates=n_b)
                    pending = i
            if pending is not None:
                info = c.evaluate_light_wait(abi.LAYER_WORLD)
                assert_same(info, c.read_light_volume(abi.LAYER_WORLD, sp.size), want[pending], f"worker thread, step {pending}")

    run(True)
    run(False)


@pytest.mark.parametrize("seed", range(int(os.environ.get("AIC_LIGHT_TP_FUZZ_N", "8"))))
def test_light_updater_throughput_fuzz(ctx, seed):
    """Random scenes of 16-40 cubes per axis with the block mix of the small-scene fuzz, at throughput batch sizes."""
    sp = _random_light_scene(500 + seed, sizes=(16, 41))
    rng = np.random.default_rng(9000 + seed)
    batch = int(rng.choice([65, 300, 2048, 8192]))
    order = int(rng.choice([0, 16]))
    lanes = int(rng.choice([1, 64, 256]))
    maxd = int(rng.choice([5, 30, 60]))
    with oracle.LightSession(copy.deepcopy(sp), maxd, hb_width=order, threads=THREADS) as s:
        n, cost, left = s.evaluate(fast=True, epsilon=1, batch=batch)
        want = (s.light(), n, cost, left)
    ctx.upload_space(abi.LAYER_WORLD, sp)
    info = ctx.evaluate_light(abi.LAYER_WORLD, maxd, fast=True, epsilon=1, batch=batch, queue_order=order, lanes_per_cube=lanes)
    got = ctx.read_light_volume(abi.LAYER_WORLD, sp.size)
    assert_same(info, got, want, f"seed {seed}: size {sp.size}, batch {batch}, order {order}, lanes {lanes}, distance {maxd}")
