"""The one table of named launch schedules: pt_tuning keyword sets for Renderer.SetTuning (include/ptrt.h pt_tuning; every value inside
what pt_context_set_tuning accepts), and what a frame rendered under each must show in its pt_stats. Plain data and two checks: no
import of the package. Test helpers only.

A schedule changes how a frame's paths are cut into launches and never a pixel. With `finish_below = 0` no shard runs its paths to their
end inside one launch, so path states really are stored by one launch and loaded by the next; `crosses` says so, and `check_stats` holds
a frame to it, so that a sweep which silently runs in finish mode fails instead of passing for nothing.

Pytest rewrites `assert` only in test modules, so every assert here carries its own message."""
from collections import namedtuple

# tuning: the keywords of SetTuning; crosses: path states cross launch boundaries (finish_below = 0);
# repacks: None = not stated, False = pt_stats.reserved[1] == 0, True = pt_stats.reserved[1] > 0
Schedule = namedtuple("Schedule", "name tuning crosses repacks")

# one ray per lane and launch: every launch boundary may separate a vertex's shadow ray from its extension ray
PASS = dict(bounces=1, finish_below=0)


def _row(name, tuning, repacks=None):
    return Schedule(name, dict(tuning), tuning.get("finish_below") == 0, repacks)


TABLE = (
    _row("default", {}),                                                         # the control: the library's own choices
    _row("pass", PASS),
    _row("odd", dict(bounces=3, finish_below=0)),                                # a boundary after every third ray: both kinds of ray wait
    _row("even", dict(bounces=2, finish_below=0)),
    _row("long", dict(bounces=16, finish_below=0)),
    _row("finish_always", dict(bounces=1, finish_below=1000000)),                # every shard in finish mode from the first launch
    _row("never_repack", dict(PASS, compact_below=0.0), repacks=False),          # queues carried in place with their holes
    _row("repack_every", dict(PASS, compact_below=2.0, sticky_samples=0), repacks=True),
    _row("ratio", dict(bounces=2, finish_below=0, compact_below=0.9, sticky_samples=0)),
    _row("sticky", dict(bounces=2, finish_below=0, compact_below=0.9, sticky_samples=32)),
    _row("sparse_half", dict(bounces=4, finish_below=0, compact_below=2.0, sparse_below=0.5)),
    _row("sparse_all", dict(bounces=4, finish_below=0, compact_below=2.0, sparse_below=1.0)),
    _row("loops1", dict(PASS, loops=1)),
    _row("loops2", dict(PASS, loops=2)),
    _row("loops4", dict(PASS, loops=4)),
    _row("lag2", dict(PASS, lag=2)),
    _row("lag5", dict(PASS, lag=5)),
    _row("copyback", dict(PASS, readback=1)),
)
NAMES = tuple(s.name for s in TABLE)
_BY_NAME = {s.name: s for s in TABLE}


def schedule(name):
    return _BY_NAME[name]


def tuned(P, name, w, h):
    """A Renderer of its own under schedule `name`, initialised; the caller disposes of it."""
    r = P.Renderer(P.Window(w, h))
    r.Init()
    try:
        r.SetTuning(**_BY_NAME[name].tuning)
    except Exception:
        r.Dispose()
        raise
    return r


def can_cross(name, spp, streams, rays_per_sample):
    """Whether a frame can carry a path state across a launch under schedule `name` at all: a slot traces its stream's samples one after
    the other, at most ceil(spp / streams) x `rays_per_sample` rays, and a launch lets it trace `bounces` of them."""
    s = _BY_NAME[name]
    return s.crosses and s.tuning["bounces"] < -(-spp // max(streams, 1)) * rays_per_sample


def check_stats(name, st, default_st, slots, ctx, crossing=True):
    """What schedule `name` must show in the pt_stats `st` of a frame whose first launch starts `slots` path states and whose `default`
    schedule gave `default_st`. crossing=False: the frame is too short for this schedule to cut (can_cross)."""
    s = _BY_NAME[name]
    if s.crosses and crossing:
        assert st.iterations > default_st.iterations, \
            ("schedule did not add launches", name, ctx, st.iterations, default_st.iterations)
        # reserved[2]: path states read + written by the loop = the paths alive at every launch's start, the first launch's included
        assert st.reserved[2] > slots, \
            ("no path state crossed a launch", name, ctx, st.reserved[2], slots)
    if s.repacks is False:
        assert st.reserved[1] == 0, ("queues were re-packed", name, ctx, st.reserved[1])
    if s.repacks is True:
        assert st.reserved[1] > 0, ("no queue was re-packed", name, ctx, st.reserved[1])
