"""The pipelines a path-traced frame can run, and the requests pt_render refuses: the two tables every test that sweeps "all the
pipelines" selects from, by name. The library's own statement is pathtracing_amd/csrc/pipeline.h; test_pipeline.py holds it to a
restatement of the rules over every input, and these flag values to pathtracing_amd/_native.py. Plain data: no import of the package."""
from collections import namedtuple

# pt_render_params.flags (include/ptrt.h) that choose or narrow the pipeline
FLAGS = {"PROFILE_KERNELS": 1, "COUNT_VISITS": 2, "EXTEND_PACKED": 4, "EXTEND_SIMPLE": 8, "BUCKET_SPECULAR": 32, "SPLIT_KERNELS": 64,
         "EXTEND_POOL": 128, "NEXT_EVENT": 256}
PT_ERR_UNSUPPORTED = 6
EXT_SIMPLE, EXT_PACKED, EXT_POOL = 1, 2, 3  # pt_stats.reserved[0], pt_tuning.extend_kernel

# full_state: the frame starts with k_generate writing every slot's path state (k_shade and the pooled kernel read it from memory);
# the others start from the cached template and build the state in registers, and only they resolve sky pixels.
# kernel: pt_stats.reserved[0] of such a frame, None where the scene's probe decides.
Pipeline = namedtuple("Pipeline", "name flags full_state kernel")
RUNNABLE = (
    Pipeline("probed", 0, False, None),                                                      # the default
    Pipeline("simple", FLAGS["EXTEND_SIMPLE"], False, EXT_SIMPLE),                           # one ray per lane, fused shading
    Pipeline("packed", FLAGS["EXTEND_PACKED"], False, EXT_PACKED),                           # lane-packing, fused shading
    Pipeline("pool", FLAGS["EXTEND_POOL"], True, EXT_POOL),                                  # pooled, fused shading
    Pipeline("split", FLAGS["SPLIT_KERNELS"], True, None),                                   # probed extend-only kernel, then k_shade
    Pipeline("split+packed", FLAGS["SPLIT_KERNELS"] | FLAGS["EXTEND_PACKED"], True, EXT_PACKED),  # lane-packing extend-only, then k_shade
    Pipeline("bucket", FLAGS["BUCKET_SPECULAR"], True, None),                                # split, specular kinds shaded from buckets
)
_BY_NAME = {p.name: p for p in RUNNABLE}


def select(*names):
    """The named rows of RUNNABLE, in the order asked for (all of them, in table order, without names)."""
    return [_BY_NAME[n] for n in names] if names else list(RUNNABLE)


def flags_of(*names):
    return [p.flags for p in select(*names)]


def named_flags(*names):
    return [(p.name, p.flags) for p in select(*names)]


# What pt_render refuses. needs: what the frame has ("nee": PT_FLAG_NEXT_EVENT, "env": a scene with an environment map); with: the flag
# or the pt_tuning.extend_kernel that it is refused with; says: a part of the message that names the rule.
#   Next-event estimation and the environment map live in the fused one-ray-per-lane kernel only, so whatever asks for another extend
# kernel or for k_shade is refused; and neither counts visits (a shadow ray's traversal stops at its tmax, which the counters do not
# describe). With both, the environment's refusal comes first.
Refusal = namedtuple("Refusal", "name needs flags tuned_kernel status says")
_OTHER = (("packed", FLAGS["EXTEND_PACKED"], 0), ("pool", FLAGS["EXTEND_POOL"], 0), ("split", FLAGS["SPLIT_KERNELS"], 0),
          ("bucket", FLAGS["BUCKET_SPECULAR"], 0), ("tuned packed", 0, EXT_PACKED), ("tuned pool", 0, EXT_POOL))
REFUSED = tuple(
    [Refusal("nee+" + n, "nee", f, k, PT_ERR_UNSUPPORTED, "PT_FLAG_NEXT_EVENT runs on the one-ray-per-lane kernel only") for n, f, k in _OTHER]
    + [Refusal("nee+count", "nee", FLAGS["COUNT_VISITS"], 0, PT_ERR_UNSUPPORTED, "PT_FLAG_NEXT_EVENT does not count visits")]
    + [Refusal("env+" + n, "env", f, k, PT_ERR_UNSUPPORTED, "a scene with an environment map renders on the one-ray-per-lane kernel only")
       for n, f, k in _OTHER + (("count", FLAGS["COUNT_VISITS"], 0),)])


def refused(needs, tuned=False):
    """The refusals of a `needs` frame: by a frame flag (tuned=False) or by pt_tuning.extend_kernel (tuned=True)."""
    return [r for r in REFUSED if r.needs == needs and bool(r.tuned_kernel) == tuned]
