"""The wave-scheduler model's SIM_FIRST_LOOKUP switch (tools/wave_sim): the ENTER and RAY phases consume a leading 'l' token -- the first lookup of the
level they set up, when it finds nothing -- of the lane they serve, as the kernel's ENTER and NEWRAY events do. CPU only; the `small` workload."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools", "wave_sim"))

# the kernel's policy as built (the exchange constants of aic_tunables.h), and no exchange at all
SETTINGS = (dict(pool=64, reservoir=1, policy=3, deposit_free=3, min_gain=8, c_xchg_base=75, c_xchg_move=450, c_pass=120), dict())


def test_first_lookup_switch_serves_every_event_once_with_no_more_passes(monkeypatch):
    import run as R

    lib = R.build_lib()
    tok, off, w, h, _, _ = R.tokens(lib, "small", 1)
    t = tok.view(np.uint8)
    shade_tokens = int(((t == ord("S")) | (t == ord("O"))).sum())
    enter_tokens = int((t == ord("E")).sum())
    assert (t == ord("l")).sum() > 0, "the workload has first lookups that find nothing"

    def run(**kw):
        p = R.defaults(w, h)
        p.n_cus = 4
        for k, v in kw.items():
            setattr(p, k, v)
        o = R.Out()
        assert lib.simulate(tok.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), ctypes.byref(p), ctypes.byref(o)) == 0
        return o

    for kw in SETTINGS:
        monkeypatch.delenv("SIM_FIRST_LOOKUP", raising=False)
        off_ = run(**kw)
        monkeypatch.setenv("SIM_FIRST_LOOKUP", "0")
        zero = run(**kw)
        assert (zero.busy_inst, zero.trips, zero.pass_iters) == (off_.busy_inst, off_.trips, off_.pass_iters), "SIM_FIRST_LOOKUP=0 is the switch off"
        monkeypatch.setenv("SIM_FIRST_LOOKUP", "1")
        on = run(**kw)
        assert on.lanes[1] == shade_tokens and on.lanes[2] == enter_tokens, "every SHADE / ENTER token is still served exactly once"
        assert off_.lanes[1] == shade_tokens and off_.lanes[2] == enter_tokens
        assert on.pass_iters <= off_.pass_iters and on.trips <= off_.trips, (kw, on.pass_iters, off_.pass_iters, on.trips, off_.trips)
        # the lookups that moved into the events are no longer made by full passes: at most as many lane-passes as before, and fewer
        assert on.pass_lanes < off_.pass_lanes
