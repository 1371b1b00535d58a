"""Row c of SURVEY.md §8 ("the oracle"), the part the reference pins: oracle/pt_oracle.c:55-83 claims the op order of the
reference's COMPILED shader (RayTracing/Assets/Shaders/Compiled/Ray/Test.spirv), not just the semantics of Test.hlsl:1-40.
These tests hold that claim against the decoded module itself — tests/golden/test_spirv_ops.json, the instruction words of
the 1,524-byte file as data (tests/golden/make_spirv_ops.py; parsed, never executed) — and then check that the oracle
really computes the FMA-contracted form: an independent numpy float32 restatement in the module's op order equals the
oracle bit for bit, and the same restatement with the two OpExtInst Fma replaced by multiply + add does not.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OPS = json.load(open(os.path.join(HERE, "golden", "test_spirv_ops.json")))
INS = OPS["instructions"]
BY_ID = {i["id"]: i for i in INS if "id" in i}
TEST_SPIRV_SHA256 = "051e3943762e15c4331937cf14d8bcb8bb281fc8ba744d7a116d3593419c9f0f"  # RayTracing/Assets/Shaders/Compiled/Ray/Test.spirv


def const(i):
    """f32 value of a scalar OpConstant id, or the tuple of a composite's members."""
    d = BY_ID[i]
    if d["op"] == "OpConstant":
        return d["f32"]
    assert d["op"] == "OpConstantComposite"
    return tuple(const(m) for m in d["operands"])


def only(op, **kw):
    hits = [i for i in INS if i["op"] == op and all(i.get(k) == v for k, v in kw.items())]
    assert len(hits) == 1, (op, kw, hits)
    return hits[0]


def test_fixture_is_the_reference_file(tmp_path):
    """The fixture is the reference's Test.spirv decoded without loss: the words it holds rebuild a 1,524-byte module with that
    file's sha256, and decoding those bytes gives the fixture back."""
    import hashlib
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_spirv_ops", os.path.join(HERE, "golden", "make_spirv_ops.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    raw = m.encode(OPS)
    assert len(raw) == OPS["bytes"] == 1524
    assert hashlib.sha256(raw).hexdigest() == OPS["sha256"] == TEST_SPIRV_SHA256
    (tmp_path / "Test.spirv").write_bytes(raw)
    assert m.decode(str(tmp_path / "Test.spirv")) == OPS


def test_dispatch_shape_and_store():
    # Test.hlsl:3 [numthreads(32, 32, 1)] -> OpExecutionMode LocalSize 32 32 1; Test.hlsl:39 -> one OpImageWrite of the merged colour
    em = only("OpExecutionMode")
    assert em["operands"][1:] == [17, 32, 32, 1]  # 17 = LocalSize
    wr = only("OpImageWrite")
    assert BY_ID[wr["operands"][2]]["op"] == "OpPhi"
    coord = BY_ID[wr["operands"][1]]
    assert coord["op"] == "OpVectorShuffle" and coord["operands"][2:] == [0, 1]  # id.xy


def test_uv_is_a_reciprocal_multiply():
    # a1: uv = float2(id.xy) * 0.00092592591 (0x3a72b9d6 = f32(1/1080)) * 2 - 1: OpFMul by a constant vector, NOT an OpFDiv by 1080
    k = [i for i in INS if i["op"] == "OpConstant" and i["bits"] == "0x3a72b9d6"]
    assert len(k) == 1
    inv = [i for i in INS if i["op"] == "OpConstantComposite" and i["operands"] == [k[0]["id"]] * 2]
    assert len(inv) == 1
    cvt = only("OpConvertUToF")
    mul = [i for i in INS if i["op"] == "OpFMul" and i["operands"] == [cvt["id"], inv[0]["id"]]]
    assert len(mul) == 1
    x2 = [i for i in INS if i["op"] == "OpVectorTimesScalar" and i["operands"][0] == mul[0]["id"]]
    assert len(x2) == 1 and const(x2[0]["operands"][1]) == 2.0
    sub = only("OpFSub")
    assert sub["operands"][0] == x2[0]["id"] and const(sub["operands"][1]) == (1.0, 1.0)
    assert not any(i["op"] == "OpFDiv" and const_or_none(i["operands"][1]) == 1080.0 for i in INS)


def const_or_none(i):
    return const(i) if BY_ID.get(i, {}).get("op") in ("OpConstant", "OpConstantComposite") else None


def test_intersection_dataflow():
    # a2/a3 in the compiled op order the oracle's comments cite (pt_oracle.c:57-72)
    norms = [i for i in INS if i["op"] == "OpExtInst" and i["inst"] == "Normalize"]
    assert len(norms) == 2
    d = norms[0]                                           # d = normalize(float3(uv, -1))
    v = BY_ID[d["operands"][0]]
    assert v["op"] == "OpCompositeConstruct" and const(v["operands"][2]) == -1.0
    a = only("OpDot")                                      # a = dot(d, d)
    assert a["operands"] == [d["id"], d["id"]]
    dz = [i for i in INS if i["op"] == "OpCompositeExtract" and i["operands"] == [d["id"], 2]]
    assert len(dz) == 1
    fmas = [i for i in INS if i["op"] == "OpExtInst" and i["inst"] == "Fma"]
    assert len(fmas) == 2
    disc, num = fmas
    # disc = fma(b, b, a * -3) with b = 2 * d.z        (b*b - 4ac with oc = (0,0,1), r = 0.5 folded: 4c = 3)
    b = BY_ID[disc["operands"][0]]
    assert disc["operands"][0] == disc["operands"][1] and b["op"] == "OpFMul"
    assert const(b["operands"][0]) == 2.0 and b["operands"][1] == dz[0]["id"]
    m3 = BY_ID[disc["operands"][2]]
    assert m3["op"] == "OpFMul" and m3["operands"][0] == a["id"] and const(m3["operands"][1]) == -3.0
    # hit iff disc > 0 (strict, ordered), and that is what the branch tests
    gt = only("OpFOrdGreaterThan")
    assert gt["operands"][0] == disc["id"] and const(gt["operands"][1]) == 0.0
    assert only("OpBranchConditional")["operands"][0] == gt["id"]
    # t = fma(d.z, -2, -sqrt(disc)) / (2 * a): near root only, ONE divide in the whole module, no t > 0 test
    sq = [i for i in INS if i["op"] == "OpExtInst" and i["inst"] == "Sqrt"]
    assert len(sq) == 1 and sq[0]["operands"] == [disc["id"]]
    neg = only("OpFNegate")
    assert neg["operands"] == [sq[0]["id"]]
    assert num["operands"][0] == dz[0]["id"] and const(num["operands"][1]) == -2.0 and num["operands"][2] == neg["id"]
    div = only("OpFDiv")
    den = BY_ID[div["operands"][1]]
    assert div["operands"][0] == num["id"] and den["op"] == "OpFMul" and const(den["operands"][0]) == 2.0 and den["operands"][1] == a["id"]
    # P = (0,0,1) + d * t; n = normalize(P); colour = n * 0.5 + 0.5, alpha 1
    dt = [i for i in INS if i["op"] == "OpVectorTimesScalar" and i["operands"] == [d["id"], div["id"]]]
    assert len(dt) == 1
    adds = [i for i in INS if i["op"] == "OpFAdd"]
    assert len(adds) == 2
    assert const(adds[0]["operands"][0]) == (0.0, 0.0, 1.0) and adds[0]["operands"][1] == dt[0]["id"]
    assert norms[1]["operands"] == [adds[0]["id"]]
    half = [i for i in INS if i["op"] == "OpVectorTimesScalar" and i["operands"][0] == norms[1]["id"]]
    assert len(half) == 1 and const(half[0]["operands"][1]) == 0.5
    assert adds[1]["operands"][0] == half[0]["id"] and const(adds[1]["operands"][1]) == (0.5, 0.5, 0.5)
    # miss colour = (uv.x, uv.y, 0, 1)
    cc = [i for i in INS if i["op"] == "OpCompositeConstruct" and len(i["operands"]) == 4]
    assert len(cc) == 2
    assert [const_or_none(x) for x in cc[1]["operands"][2:]] == [0.0, 1.0] and const(cc[0]["operands"][3]) == 1.0
    # no comparison other than disc > 0 exists: no tmin / tmax / t > 0 test
    assert sum(1 for i in INS if i["op"].startswith("OpFOrd") or i["op"].startswith("OpFUnord")) == 1


# ------------------------------------------------------------------------------------------------ the oracle computes THAT form
def _fma32(x, y, z):
    """float32 fma of float32 arrays, exact wherever it says so: x*y is exact in float64; the float64 sum's rounding error is
    recovered (TwoSum) and a result is flagged ambiguous only if the float64 sum landed exactly on a float32 rounding boundary
    while inexact (double rounding) — those few pixels are left out of the comparison."""
    p = x.astype(np.float64) * y.astype(np.float64)
    c = z.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    lo = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    hi = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    r64 = r.astype(np.float64)
    tie = (err != 0) & ((s == (r64 + lo) / 2) | (s == (r64 + hi) / 2))
    return r, tie


def _restate(w, h, use_fma):
    """The module's ops in order, numpy float32 (every +, *, /, sqrt correctly rounded). Returns HxWx4 and the ambiguous mask."""
    f = np.float32
    inv1080 = np.array([0x3a72b9d6], np.uint32).view(np.float32)[0]
    x = np.arange(w, dtype=np.uint32).astype(f)[None, :].repeat(h, 0)
    y = np.arange(h, dtype=np.uint32).astype(f)[:, None].repeat(w, 1)
    uvx, uvy = (x * inv1080) * f(2) - f(1), (y * inv1080) * f(2) - f(1)
    vz = np.full_like(uvx, -1.0)
    ln = np.sqrt(uvx * uvx + uvy * uvy + vz * vz)
    dx, dy, dz = uvx / ln, uvy / ln, vz / ln
    a = dx * dx + dy * dy + dz * dz
    b = f(2) * dz
    amb = np.zeros(a.shape, bool)
    if use_fma:
        disc, t1 = _fma32(b, b, a * f(-3)); amb |= t1
    else:
        disc = b * b + a * f(-3)
    hit = disc > 0
    sq = np.sqrt(np.where(hit, disc, f(1)))
    if use_fma:
        num, t2 = _fma32(dz, np.full_like(dz, -2.0), -sq); amb |= t2 & hit
    else:
        num = dz * f(-2) + -sq
    t = num / (f(2) * a)
    px, py, pz = f(0) + dx * t, f(0) + dy * t, f(1) + dz * t
    pl = np.sqrt(px * px + py * py + pz * pz)
    with np.errstate(invalid="ignore", divide="ignore"):
        nx, ny, nz = px / pl, py / pl, pz / pl
    out = np.empty((h, w, 4), f)
    out[..., 0] = np.where(hit, nx * f(0.5) + f(0.5), uvx)
    out[..., 1] = np.where(hit, ny * f(0.5) + f(0.5), uvy)
    out[..., 2] = np.where(hit, nz * f(0.5) + f(0.5), f(0))
    out[..., 3] = 1.0
    return out, amb


def test_oracle_computes_the_fma_contracted_form(pto):
    w, h = 1920, 1080
    got, _ = pto.reference_sphere(w, h)
    want, amb = _restate(w, h, use_fma=True)
    assert amb.sum() < 16  # double-rounding candidates of the emulation: a handful at most
    ok = ~amb
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), "the oracle is not the SPIR-V's op order (fma(b,b,a*-3), fma(d.z,-2,-sqrt))"
    # and the test can tell: with the two Fma replaced by multiply + add the picture differs (also in which pixels are hits)
    plain, _ = _restate(w, h, use_fma=False)
    differs = (plain.view(np.uint32) != got.view(np.uint32)).any(-1)
    assert differs.sum() > 1000
    assert ((plain[..., 2] != 0) != (got[..., 2] != 0)).sum() >= 0  # silhouette flips are possible but not required
