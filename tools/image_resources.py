"""Generated code of the image-quality kernels, one source tree against another (no GPU), as tools/raster_resources.py
does for the rasterizer: eval_metrics.hip, loss.hip and lpips.hip of both trees compiled for the device only with the
library's flags plus -Rpass-analysis=kernel-resource-usage -S.  Per kernel instantiation: VGPR, scratch, LDS,
occupancy, instruction count, the fp64 fma / mul / add counts, and whether the instruction streams are identical,
a reordering, or differ in a floating-point, LDS or memory opcode count.
    python tools/image_resources.py PARENT_CSRC [NEW_CSRC] > profiles/image_helpers_resources.txt
Exit status 1 when LDS, scratch or occupancy of a kernel differ, or a floating-point, LDS, global or atomic opcode
count does."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.raster_resources import _CLASS, bodies, compile_unit, demangle, opcounts  # noqa: E402

UNITS = ("eval_metrics.hip", "loss.hip", "lpips.hip")
KERNELS = re.compile(r"eval_metrics_kernel|eval_ssim_reduce_kernel|loss_(moments|reduce|grad)_kernel|lpips_input_kernel")
FP64 = ("v_fma_f64", "v_mul_f64", "v_add_f64")


def tree(csrc, tmp):
    res, asm = {}, {}
    for u in UNITS:
        r, a = compile_unit(csrc, u, tmp)
        res.update(r)
        asm.update(bodies(a))
    names = demangle(sorted(asm))
    return {names[n]: (res[n], asm[n]) for n in asm if KERNELS.search(names[n])}


def main():
    parent = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "splatformer_amd", "csrc")
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        A, B = tree(parent, ta), tree(new, tb)
    bad = 0
    print("Image-quality helpers (image_common.h): generated code of the parent commit vs this change")
    print("=" * 88)
    print("eval_metrics.hip, loss.hip and lpips.hip of both trees compiled for gfx950 with the library's flags plus\n"
          "--cuda-device-only -Rpass-analysis=kernel-resource-usage -S.  parent=new where a figure is equal, parent!new\n"
          "where it differs.  \"fma/mul/add f64\": v_fma_f64 / v_mul_f64 / v_add_f64 counts.  \"stream\": the instruction\n"
          "streams compared line by line with branch labels normalised.\n")
    print(f"{'kernel':<36}{'VGPR':>10}{'scratch':>9}{'LDS':>14}{'occ':>6} {'instr parent':>13}{'new':>6}  "
          f"{'fma/mul/add f64':<26}stream")
    for k in sorted(set(A) | set(B)):
        if k not in A or k not in B:
            print(f"{k:<36} only in {'parent' if k in A else 'new'}")
            bad += 1
            continue
        (ra, ba), (rb, bb) = A[k], B[k]
        f = lambda key: f"{ra.get(key, 0)}{'=' if ra.get(key, 0) == rb.get(key, 0) else '!'}{rb.get(key, 0)}"  # noqa: E731
        flagged = any(ra.get(key, 0) != rb.get(key, 0)
                      for key in ("ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"))
        ca, cb = opcounts(ba, True), opcounts(bb, True)
        fp = " ".join(f"{ca[o]}{'=' if ca[o] == cb[o] else '!'}{cb[o]}" for o in FP64)
        if ba == bb:
            stream = "identical"
        else:
            ndiff = sum(1 for x, y in zip(ba, bb) if x != y) + abs(len(ba) - len(bb))
            d = {o: cb[o] - ca[o] for o in set(ca) | set(cb) if ca[o] != cb[o] and _CLASS.match(o)}
            if d:
                flagged = True
                stream = f"differs: {ndiff} of {len(bb)} lines; opcode counts differ in " + ", ".join(
                    f"{o} {v:+d}" for o, v in sorted(d.items()))
            elif opcounts(ba, False) == opcounts(bb, False):
                stream = f"differs: {ndiff} of {len(bb)} lines; same opcode counts (order / registers only)"
            else:
                stream = f"differs: {ndiff} of {len(bb)} lines; integer / scalar / control ops only"
        print(f"{k:<36}{f('VGPRs'):>10}{f('ScratchSize [bytes/lane]'):>9}{f('LDS Size [bytes/block]'):>14}"
              f"{f('Occupancy [waves/SIMD]'):>6} {len(ba):>13}{len(bb):>6}  {fp:<26}{stream}")
        bad += flagged
    print(f"kernels whose LDS, scratch, occupancy or floating-point / memory opcode counts differ: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
