"""Generated code of the rasterizer kernels, one source tree against another (no GPU): compiles the rasterizer
translation units of both for the device only with the library's flags plus
-Rpass-analysis=kernel-resource-usage, and once more with -S.  Per kernel instantiation: VGPR, AGPR, scratch, LDS,
occupancy and instruction count, parent=new where equal and parent!new where not; whether the two instruction
streams are identical (branch labels normalised), a reordering (equal per-opcode counts) or which opcode counts
differ; and for the forward kernels the v_fma_f32 / v_mul_f32 / v_add_f32 counts.
    python tools/raster_resources.py PARENT_CSRC [NEW_CSRC] > profiles/raster_helpers_resources.txt
PARENT_CSRC holds the parent commit's csrc/ (git archive or a worktree).  Exit status 1 when LDS, scratch or
occupancy of a kernel differ, or a floating-point, LDS, global or atomic opcode count does (forms of one IEEE
operation folded together: packed / scalar, fma / fmac, sub / add of the negated operand)."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from splatformer_amd import build_lib  # noqa: E402
from tools.gemm_resources import parse_remarks  # noqa: E402

UNITS = ("render.hip", "render_nd.hip", "rasterize.hip")
KERNELS = re.compile(r"rasterize_(fwd|bwd)|pack_raster_records|isect_(count|emit)_cull|render_prep_project_kernel")
_INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
# opcode classes whose counts have to agree; a packed op counts as two of its scalar form
_CLASS = re.compile(r"^(v_(pk_)?(fma|mul|add|sub|mac|fmac|min|max|exp|log|rcp|rsq|sqrt|cvt|div|ldexp|frexp|trig|med3)\w*_f(16|32|64)\w*"
                    r"|ds_\w+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+)$")


def compile_unit(csrc, unit, tmp):
    flags = [f for f in build_lib.CFLAGS if not f.startswith("-I")] + [f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}"]
    src, asm = os.path.join(csrc, unit), os.path.join(tmp, unit + ".s")
    r = subprocess.run([build_lib.HIPCC, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        src, "-o", asm], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return parse_remarks(r.stderr), open(asm).read()


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    short = lambda s: re.sub(r"^(?:void )?\(anonymous namespace\)::|\(.*$", "", s)
    return {n: short(d) for n, d in zip(names, out.stdout.splitlines())}


def bodies(text):
    """assembly -> {mangled kernel: [instruction lines, branch labels normalised]}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur is None:
            continue
        m = _INSTR.match(line)
        if m and not m.group(1).startswith("p2align"):
            cur.append(re.sub(r"\.LBB\d+_\d+", ".L", re.sub(r"\s*;.*$", "", line.strip())))
    return out


def opcounts(body, fold):
    c = collections.Counter()
    for ins in body:
        op = re.sub(r"_e(32|64)$|_dpp$|_sdwa$", "", ins.split()[0])
        n = 1
        if fold:  # forms of one IEEE operation: packed = two scalar, fmac = fma into its addend, a - b = a + (-b)
            if op.startswith("v_pk_") and op.endswith("_f32"):
                op, n = op.replace("v_pk_", "v_"), 2
            op = {"v_fmac_f32": "v_fma_f32", "v_sub_f32": "v_add_f32", "v_subrev_f32": "v_add_f32"}.get(op, op)
        c[op] += n
    return c


def tree(csrc, tmp):
    res, asm = {}, {}
    for u in UNITS:
        if os.path.exists(os.path.join(csrc, u)):
            r, a = compile_unit(csrc, u, tmp)
            res.update(r)
            asm.update(bodies(a))
    names = demangle(sorted(asm))
    keep = {names[n]: n for n in asm if KERNELS.search(names[n])}
    return {k: (res[m], asm[m]) for k, m in keep.items()}


def main():
    parent = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "splatformer_amd", "csrc")
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        A, B = tree(parent, ta), tree(new, tb)
    bad = 0
    print("Rasterizer helpers (raster_common.h): generated code of the parent commit vs this change")
    print("=" * 88)
    print("render.hip + render_nd.hip (parent) and render.hip + rasterize.hip (new) compiled for gfx950 with the library's\n"
          "flags (build_lib.CFLAGS) plus --cuda-device-only -Rpass-analysis=kernel-resource-usage -S.  Per kernel\n"
          "instantiation: parent=new where a figure is equal, parent!new where it differs.  \"instr\": instruction lines of\n"
          "the kernel body.  \"stream\": the two instruction streams compared line by line with branch-label numbers\n"
          "normalised; where they differ, whether the per-opcode counts still agree (a pure reordering / register\n"
          "renaming) or which floating-point, LDS, global or scratch opcodes changed count (forms of one IEEE operation\n"
          "folded: a packed f32 op is two scalar ones, v_fmac is v_fma, v_sub is v_add of the negated operand), else\n"
          "\"integer / scalar / control ops only\".  \"fma/mul/add\": the\n"
          "kernel's v_fma_f32 / v_mul_f32 / v_add_f32 counts (packed forms folded in), parent=new.\n")
    print(f"{'kernel':<44}{'VGPR':>10}{'AGPR':>8}{'scratch':>10}{'LDS':>14}{'occ':>6} {'instr parent':>13}{'new':>6}  "
          f"{'fma/mul/add':<28}stream")
    for k in sorted(set(A) | set(B)):
        if k not in A or k not in B:
            print(f"{k:<44} only in {'parent' if k in A else 'new'}")
            bad += 1
            continue
        (ra, ba), (rb, bb) = A[k], B[k]
        f = lambda key: f"{ra.get(key, 0)}{'=' if ra.get(key, 0) == rb.get(key, 0) else '!'}{rb.get(key, 0)}"
        flagged = any(ra.get(key, 0) != rb.get(key, 0)
                      for key in ("ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"))
        ca, cb = opcounts(ba, True), opcounts(bb, True)
        fp = " ".join(f"{ca[o]}{'=' if ca[o] == cb[o] else '!'}{cb[o]}" for o in ("v_fma_f32", "v_mul_f32", "v_add_f32"))
        if ba == bb:
            stream = "identical"
        else:
            ndiff = sum(1 for x, y in zip(ba, bb) if x != y) + abs(len(ba) - len(bb))
            ra_, rb_ = opcounts(ba, False), opcounts(bb, False)
            if ra_ == rb_:
                stream = f"differs: {ndiff} of {len(bb)} lines; same opcode counts (order / registers only)"
            else:
                d = {o: cb[o] - ca[o] for o in set(ca) | set(cb) if ca[o] != cb[o] and _CLASS.match(o)}
                if d:
                    flagged = True
                    stream = f"differs: {ndiff} of {len(bb)} lines; opcode counts differ in " + ", ".join(
                        f"{o} {v:+d}" for o, v in sorted(d.items()))
                else:
                    d2 = {o: rb_[o] - ra_[o] for o in set(ra_) | set(rb_) if ra_[o] != rb_[o]}
                    stream = (f"differs: {ndiff} of {len(bb)} lines; opcode counts differ in integer / scalar / control "
                              "ops only (" + ", ".join(f"{o} {v:+d}" for o, v in sorted(d2.items())) + ")")
        print(f"{k:<44}{f('VGPRs'):>10}{f('AGPRs'):>8}{f('ScratchSize [bytes/lane]'):>10}"
              f"{f('LDS Size [bytes/block]'):>14}{f('Occupancy [waves/SIMD]'):>6} {len(ba):>13}{len(bb):>6}  {fp:<28}{stream}")
        bad += flagged
    print(f"kernels whose LDS, scratch, occupancy or floating-point / memory opcode counts differ: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
