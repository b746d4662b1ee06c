"""Static resource report of the fused Block MLP's kernels (no GPU): compiles csrc/mlp.hip for the device only with
the library's flags plus -Rpass-analysis=kernel-resource-usage, and reads the generated assembly.  One row per
`mlp_kernel` instantiation: VGPRs, AGPRs, scratch bytes per lane, LDS bytes, occupancy (waves per SIMD), and three
counts of waits the compiler added (a written wait stands between #ASMSTART / #ASMEND, or behind a
`; written wait vmcnt(N)` comment and no stricter than it, and is not counted):
  * `s_waitcnt` with vmcnt(0) between the first and the last 16-byte store behind the main loop (the epilogue: on
    CDNA vmcnt counts stores, so such a wait holds the next store until the previous one is acknowledged);
  * `s_waitcnt` with vmcnt(0) inside the main loop (the hidden-chunk loop: the outermost loop that holds MFMAs, or
    the span from the first to the last MFMA where a split leaves one chunk and no loop): each drains the LDS-DMA
    ring;
  * whether a loop in front of the first MFMA (the parameter-table copy) waits for vmcnt(0) once per iteration.
The same columns follow for `heads_kernel` and `attn_proj_kernel`, which stream through the same LDS-DMA builtin
(information only).
    python tools/mlp_resources.py [--csrc DIR] [--include DIR] > table.txt
Exit status 1 when an `mlp_kernel` row has scratch, a counted wait, or a waiting table copy."""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from splatformer_amd import build_lib  # noqa: E402
from tools.gemm_resources import parse_remarks  # noqa: E402

UNITS = (("mlp.hip", "mlp_kernel"), ("heads.hip", "heads_kernel"), ("attn_proj.hip", "attn_proj_kernel"))
KINDS = {0: "eval", 1: "train", 2: "bwd"}

_INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_STORE16 = re.compile(r"^(buffer|global)_store_dwordx4")


def template_args(mangled, kernel):
    """integer / bool template arguments of a mangled kernel<...> instantiation, or None"""
    m = re.search(kernel + r"I((?:L[ib]n?\d+E)+)E", mangled)
    if not m:
        return None
    return [-int(v[1:]) if v.startswith("n") else int(v) for v in re.findall(r"L[ib](n?\d+)E", m.group(1))]


def kernel_bodies(text):
    """assembly text -> {mangled name: ([(op, args, written)], {label: index}, {label: loop header label})};
    written: the instruction stands in inline assembly, or is the s_waitcnt behind a `; written wait vmcnt(N)`
    marker and waits for no less than vmcnt(N) asks (a wait the compiler made stricter counts as its own)"""
    out = {}
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        body, labels, headers, in_asm, marked = [], {}, {}, False, None
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            raw = lines[i]
            i += 1
            if "#ASMSTART" in raw:
                in_asm = True
                continue
            if "#ASMEND" in raw:
                in_asm = False
                continue
            mk = re.search(r"; written wait vmcnt\((\d+)\)", raw)
            if mk:
                marked = int(mk.group(1))
                continue
            lm = _LABEL.match(raw)
            if lm:
                labels[lm.group(1)] = len(body)
                hm = re.search(r"Header=(BB\d+_\d+)", raw)
                if "Loop Header" in raw:
                    headers[lm.group(1)] = lm.group(1)
                elif hm:
                    headers[lm.group(1)] = ".L" + hm.group(1)
                continue
            im = _INSTR.match(raw.split(";")[0].rstrip())
            if im and not im.group(1).startswith("."):
                op, arg = im.group(1), im.group(2).strip()
                written = in_asm
                if marked is not None and not in_asm:
                    vm = re.search(r"vmcnt\((\d+)\)", arg)
                    written = op == "s_waitcnt" and (vm is None or int(vm.group(1)) >= marked)
                    marked = None
                body.append((op, arg, written))
        out[name] = (body, labels, headers)
    return out


def _drain(ins):
    op, arg, written = ins
    return op == "s_waitcnt" and not written and "vmcnt(0)" in arg


def analyse(body, labels, headers):
    """the three wait counts of one kernel (see the module text)"""
    mf = [k for k, (op, _, _) in enumerate(body) if op.startswith("v_mfma")]
    # a loop: the blocks the compiler's comments assign to one header (a block runs from its label to the next)
    order = sorted(labels.items(), key=lambda kv: kv[1])
    loops = {}
    for n, (lab, start) in enumerate(order):
        if lab in headers:
            end = order[n + 1][1] if n + 1 < len(order) else len(body)
            lo, hi = loops.get(headers[lab], (start, end))
            loops[headers[lab]] = (min(lo, start), max(hi, end))
    res = {"epi_stores": 0, "epi_wait0": 0, "loop_wait0": -1, "loop": "none", "copy_waits": "no loop"}
    if not mf:
        return res
    main = None
    for t, k in loops.values():  # the loop that holds the most MFMAs
        n = sum(1 for m in mf if t <= m < k)
        if n and (main is None or n > main[2]):
            main = (t, k, n)
    res["loop"] = "loop" if main else "span"
    if main is None:
        main = (mf[0], mf[-1] + 1, len(mf))
    res["loop_wait0"] = sum(1 for ins in body[main[0]:main[1]] if _drain(ins))
    end = max(main[1], mf[-1] + 1)
    stores = [k for k in range(end, len(body)) if _STORE16.match(body[k][0])]
    res["epi_stores"] = len(stores)
    if stores:
        res["epi_wait0"] = sum(1 for ins in body[stores[0]:stores[-1] + 1] if _drain(ins))
    pre = [(t, k) for t, k in loops.values() if k <= mf[0]]
    if pre:
        waits = any(any(_drain(ins) for ins in body[t:k]) and any(i[0].startswith("ds_write") for i in body[t:k])
                    for t, k in pre)
        res["copy_waits"] = "yes" if waits else "no"
    return res


def unit_report(src, kernel, csrc, inc, tmp):
    asm = os.path.join(tmp, os.path.basename(src).replace(".hip", ".s"))
    flags = [f for f in build_lib.CFLAGS if not f.startswith("-I")] + [f"-I{csrc}", f"-I{inc}"]
    cmd = [build_lib.HIPCC, *flags, "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    rem = parse_remarks(r.stderr)
    rows = []
    for name, (body, labels, headers) in kernel_bodies(open(asm).read()).items():
        targs = template_args(name, kernel)
        if targs is not None:
            rows.append((kernel, targs, rem.get(name, {}), analyse(body, labels, headers)))
    return sorted(rows, key=lambda r: r[1])


def describe(kernel, t):
    if kernel != "mlp_kernel":
        return f"{kernel}<{','.join(map(str, t))}>"
    C, waves, ring, hs, kind, one, split = t[:7]
    return (f"mlp_kernel<{C},{waves},{ring},{'hs' if hs else 'whole'},{KINDS.get(kind, kind)},"
            f"{'one' if one else 'split3'},{split}>")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=build_lib.CSRC)
    ap.add_argument("--include", default=os.path.join(ROOT, "include"))
    a = ap.parse_args()
    print("# kernel <C,waves,ring,tile,kind,products,split> | VGPRs | AGPRs | scratch B/lane | LDS B | occupancy waves/SIMD |"
          " epilogue 16-B stores | vmcnt(0) between first and last epilogue store | main loop (loop / one-chunk span) |"
          " vmcnt(0) in main loop | table copy waits per iteration")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(len(UNITS)) as ex:
        reps = ex.map(lambda u: unit_report(os.path.join(a.csrc, u[0]), u[1], a.csrc, a.include, tmp), UNITS)
        for rows in reps:
            for kernel, targs, rem, ana in rows:
                ok = ""
                if kernel == "mlp_kernel":
                    good = (rem.get("ScratchSize [bytes/lane]", 0) == 0 and ana["epi_wait0"] == 0
                            and ana["loop_wait0"] == 0 and ana["copy_waits"] != "yes")
                    ok = " ok" if good else " FAIL"
                    bad += 0 if good else 1
                print(f"{describe(kernel, targs)} | {rem.get('VGPRs', -1)} | {rem.get('AGPRs', -1)} | "
                      f"{rem.get('ScratchSize [bytes/lane]', -1)} | {rem.get('LDS Size [bytes/block]', -1)} | "
                      f"{rem.get('Occupancy [waves/SIMD]', -1)} | {ana['epi_stores']} | {ana['epi_wait0']} | "
                      f"{ana['loop']} | {ana['loop_wait0']} | {ana['copy_waits']}{ok}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
