"""The decode of a frame's pipeline (pathtracing_amd/csrc/pipeline.h, through tests/pipeline_ref/) against a restatement of the rules,
over every input: the eight flags that matter x pt_tuning.extend_kernel 0..3 x environment x specular materials = 4096 rows. No device.

The restatement below (`expected`) was written from the frame loop as it stood before the header existed — plan_frame's decode and
refusals, ExtendFrame::launch_kernel, run_loops' shading mode and fuse argument, render_frame's loop count — and from the comments of
include/ptrt.h (PT_FLAG_*, pt_tuning.extend_kernel, pt_scene_set_environment), not from the header."""
import itertools
import re

import pipeline_checker as pc
import pipelines as pl

F = pl.FLAGS
BITS = [F[n] for n in ("PROFILE_KERNELS", "COUNT_VISITS", "EXTEND_PACKED", "EXTEND_SIMPLE", "BUCKET_SPECULAR", "SPLIT_KERNELS", "EXTEND_POOL",
                       "NEXT_EVENT")]
SIMPLE, PACKED, POOL = pl.EXT_SIMPLE, pl.EXT_PACKED, pl.EXT_POOL
SHADE_NONE, SHADE_QUEUE, SHADE_BUCKETS, SHADE_INLINE = -1, 0, 1, 2
ENV_TEXT = (b"a scene with an environment map renders on the one-ray-per-lane kernel only: not with PT_FLAG_EXTEND_PACKED, "
            b"PT_FLAG_EXTEND_POOL, PT_FLAG_SPLIT_KERNELS, PT_FLAG_BUCKET_SPECULAR, PT_FLAG_COUNT_VISITS or pt_tuning.extend_kernel 2 / 3")
NEE_TEXT = (b"PT_FLAG_NEXT_EVENT runs on the one-ray-per-lane kernel only: not with PT_FLAG_EXTEND_PACKED, "
            b"PT_FLAG_EXTEND_POOL, PT_FLAG_SPLIT_KERNELS, PT_FLAG_BUCKET_SPECULAR or pt_tuning.extend_kernel 2 / 3")
NEE_COUNT_TEXT = b"PT_FLAG_NEXT_EVENT does not count visits (PT_FLAG_COUNT_VISITS)"


def inputs():
    for bits in itertools.product((0, 1), repeat=len(BITS)):
        flags = sum(b for b, on in zip(BITS, bits) if on)
        for tuned, env, spec in itertools.product(range(4), (False, True), (False, True)):
            yield flags, tuned, env, spec


def expected(flags, tuned, env, spec):
    """(status, message) of a refusal, or a dict of what the parent commit's frame loop derived."""
    profile, count = bool(flags & F["PROFILE_KERNELS"]), bool(flags & F["COUNT_VISITS"])
    bucket = bool(flags & F["BUCKET_SPECULAR"])
    split = bucket or bool(flags & F["SPLIT_KERNELS"])            # _BUCKET_SPECULAR implies _SPLIT_KERNELS
    # a frame's PT_FLAG_EXTEND_* overrides pt_tuning.extend_kernel; pooled before lane-packing before one ray per lane
    forced = POOL if flags & F["EXTEND_POOL"] else PACKED if flags & F["EXTEND_PACKED"] else SIMPLE if flags & F["EXTEND_SIMPLE"] else tuned
    nee = bool(flags & F["NEXT_EVENT"])
    if env:
        if split or count or forced in (PACKED, POOL):
            return pl.PT_ERR_UNSUPPORTED, ENV_TEXT
        forced = SIMPLE
    if nee:
        if split or forced in (PACKED, POOL):
            return pl.PT_ERR_UNSUPPORTED, NEE_TEXT
        if count:
            return pl.PT_ERR_UNSUPPORTED, NEE_COUNT_TEXT
        forced = SIMPLE
    full_state = split or forced == POOL
    shade = SHADE_INLINE if (spec or env) else SHADE_QUEUE

    def launch_kernel(choice, probing, it):  # ExtendFrame::launch_kernel; probing(g, it) needs choice == 0 and it in (2, 3)
        probing = probing and choice == 0
        return PACKED if (choice == PACKED or (probing and it == 3)) else POOL if (choice == POOL and not split) else SIMPLE

    return dict(forced=forced, profile=profile, count=count, split=split, bucket=bucket, nee=nee, env=env, shade=shade,
                fuse=SHADE_NONE if split else shade, full_state=full_state,
                resolves_sky=not full_state and not count and not env,
                instrumented=count or profile,
                single_loop=[profile or count or probing for probing in (False, True)],
                generate_mode=[1 if full_state else 2 if dense else 0 for dense in (False, True)],
                kernel_for=[[launch_kernel(choice, it != 0, it) for it in (0, 2, 3)] for choice in range(4)])


def test_every_input_decodes_as_the_rules_say():
    pc.build()
    refused = accepted = 0
    for flags, tuned, env, spec in inputs():
        want, got, ctx = expected(flags, tuned, env, spec), pc.decode(flags, tuned, env, spec), (flags, tuned, env, spec)
        if isinstance(want, tuple):
            refused += 1
            assert (got.status, got.message) == want, ctx
            continue
        accepted += 1
        assert got.status == 0 and got.message is None, ctx
        for k, v in want.items():
            g = getattr(got, k)
            if k == "kernel_for":
                g = [list(row) for row in g]
            elif isinstance(v, list):
                g, v = [int(x) for x in g], [int(x) for x in v]
            assert g == v, (ctx, k, g, v)
    assert refused + accepted == 4096 and refused > 0 and accepted > 0


def test_every_accepted_pipeline_launches_an_instantiation_that_exists():
    """Whatever kernel an accepted frame can launch — its forced one, or any the probe can remember or try — with its fuse, counting,
    NEE and environment, is an instantiation that exists; and the predicate is not vacuous."""
    lib = pc.build()
    for flags, tuned, env, spec in inputs():
        d = pc.decode(flags, tuned, env, spec)
        if d.status != 0:
            continue
        choices = [d.forced] if d.forced else [0, SIMPLE, PACKED]   # the probe remembers one ray per lane or lane-packing only
        for choice in choices:
            for kernel in d.kernel_for[choice]:
                assert lib.pr_extend_instantiated(kernel, d.fuse, d.count, d.nee, d.env), (flags, tuned, env, spec, choice, kernel)
    yes = {(k, f, c, n, e) for k, f, c, n, e in itertools.product((1, 2, 3), (-1, 0, 2), (0, 1), (0, 1), (0, 1))
           if lib.pr_extend_instantiated(k, f, c, n, e)}
    # k_extend: 3 fuse x 2 count, + NEE with 2 fused modes, + ENV (with and without NEE) all-kinds; packed 3 x 2; pool 2 x 2
    assert len(yes) == (6 + 2 + 2) + 6 + 4
    assert not lib.pr_extend_instantiated(POOL, SHADE_NONE, 0, 0, 0) and not lib.pr_extend_instantiated(SIMPLE, SHADE_BUCKETS, 0, 0, 0)
    assert not lib.pr_extend_instantiated(0, SHADE_QUEUE, 0, 0, 0) and not lib.pr_extend_instantiated(4, SHADE_QUEUE, 0, 0, 0)
    assert (lib.pr_extend_kernel_first(), lib.pr_extend_kernel_last()) == (SIMPLE, POOL)


def test_forced_compaction():
    """Buckets re-append, so they always re-pack; otherwise only a sticky frame of at most two samples per stream does."""
    lib = pc.build()
    for flags, sticky, sps in itertools.product((0, F["BUCKET_SPECULAR"], F["SPLIT_KERNELS"], F["EXTEND_PACKED"]), (0, 1), (1, 2, 3, 64)):
        assert bool(lib.pr_forces_compact(flags, sticky, sps)) == (bool(flags & F["BUCKET_SPECULAR"]) or (bool(sticky) and sps <= 2))


def test_the_tables_agree_with_the_package_and_the_decode():
    from pathtracing_amd import _native as N
    for name, value in F.items():
        assert getattr(N, "PT_FLAG_" + name) == value, name
    assert N.PT_ERR_UNSUPPORTED == pl.PT_ERR_UNSUPPORTED
    assert [p.name for p in pl.RUNNABLE] == ["probed", "simple", "packed", "pool", "split", "split+packed", "bucket"]
    for p in pl.RUNNABLE:
        for spec in (False, True):
            d = pc.decode(p.flags, 0, False, spec)
            assert d.status == 0 and bool(d.full_state) == p.full_state and d.forced == (p.kernel or 0), p.name
    assert len({p.flags for p in pl.RUNNABLE}) == len(pl.RUNNABLE)
    for r in pl.REFUSED:
        d = pc.decode(r.flags | (F["NEXT_EVENT"] if r.needs == "nee" else 0), r.tuned_kernel, r.needs == "env", False)
        assert d.status == r.status and r.says.encode() in d.message, r.name
    # the rule text exists once in C++
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hits = [f for f in glob.glob(os.path.join(root, "pathtracing_amd", "csrc", "*")) if f.endswith((".h", ".cpp", ".hip"))
            and re.search(r"only: not with PT_FLAG_EXTEND_PACKED", open(f, errors="replace").read())]
    assert [os.path.basename(f) for f in hits] == ["pipeline.h"]
