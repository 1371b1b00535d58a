"""Developer aid: did an edit change the device code? Compiles pathtracing_amd/csrc/kernels.hip of two source trees to gfx950 assembly (the
Makefile's COMMON and DEVFLAGS) and compares it per kernel (demangled name up to the '('), as text. "Identical" is modulo what is left out: the
kernel's own symbol, the position number in its block labels, comments, the __hip_cuid_ lines.   usage: python tools/isa_diff.py <tree A> <tree B>"""
import difflib, os, re, subprocess, sys, tempfile
META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
def compile_tree(tree, out):
    csrc = os.path.join(tree, "pathtracing_amd/csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name}\s*[:?]?=\s*(.*)$", mk, re.M).group(1).strip()
    flags = f"{var('COMMON')} {var('DEVFLAGS')}".replace("$(ARCH)", var("ARCH")).split()
    return subprocess.Popen([var("HIPCC"), *flags, "--cuda-device-only", "-S", "kernels.hip", "-o", out], cwd=csrc)
def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s+\.amdhsa_kernel (\S+)$", text, re.M)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    recs = {m.group(1): r for r in text[text.index("\namdhsa.kernels:"):].split("\n  - ")[1:] if (m := re.search(r"^    \.name:\s+(\S+)$", r, re.M))}
    out = {}
    for sym, dem in zip(names, plain):
        key = dem.split("(")[0].replace("void ptrt::", "")
        body = text[text.index(f"\n{sym}:") + 1:]
        body = re.sub(r"BB\d+_", "BB_", body[:re.search(r"^\.Lfunc_end\d+:$", body, re.M).start()].replace(sym, key))
        code = [c for l in body.splitlines() if "__hip_cuid_" not in l and (c := re.sub(r"\s*;.*", "", l))]
        out[key] = (code, [int(re.search(rf"^    \.{k}:\s*(\d+)$", recs[sym], re.M).group(1)) for k in META])
    return out
with tempfile.TemporaryDirectory() as tmp:
    files = [os.path.join(tmp, f"{i}.s") for i in (0, 1)]
    if any(p.wait() for p in [compile_tree(t, f) for t, f in zip(sys.argv[1:3], files)]): sys.exit("kernels.hip did not compile")
    ka, kb = kernels(files[0]), kernels(files[1])
differ, only = [k for k in sorted(ka.keys() & kb.keys()) if ka[k] != kb[k]], sorted(ka.keys() ^ kb.keys())
for k in differ:
    print(f"{k}: {len(ka[k][0])} -> {len(kb[k][0])} lines; " + ", ".join(f"{n} {x} -> {y}" for n, x, y in zip(META, ka[k][1], kb[k][1])))
    d = list(difflib.unified_diff(ka[k][0], kb[k][0], "a", "b", n=1, lineterm=""))
    if len(d) < 40: print("\n".join("    " + l for l in d))
print(f"{len(ka)} / {len(kb)} kernels, {len(differ)} differ" + (f"; in one build only: {only}" if only else ""))
sys.exit(1 if only else 0)
