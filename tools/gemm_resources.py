"""Static resource report of the gemm_kernel instantiations (no GPU): compiles the gemm_k*.hip units for the device
only with the library's flags plus -Rpass-analysis=kernel-resource-usage, and reads the generated assembly.  Per
kernel: VGPRs, VGPR spills, scratch bytes per lane, SGPR spills, instruction count (llvm-objdump of the assembled
code object), the number of `s_waitcnt vmcnt(0)` between the first and the last global store of the kernel (its
epilogue: nothing else stores to memory), and the v_readlane + v_writelane count of the main K-loop body (the
innermost loop that holds MFMAs).
    python tools/gemm_resources.py [--csrc DIR] [--include DIR] [--units k08,k38] [--spl 2] > table.txt"""
import argparse
import concurrent.futures as cf
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from splatformer_amd import build_lib  # noqa: E402

ROCM_LLVM = os.path.join(os.path.dirname(os.path.dirname(build_lib.HIPCC)), "lib", "llvm", "bin")
EPI_NAMES = {0: "general", 1: "lin", 2: "lin_gelu", 3: "pair_store"}


def template_args(mangled):
    """integer / bool template arguments of a mangled gemm_kernel<...> instantiation, or None"""
    m = re.search(r"gemm_kernelI((?:L[ib]n?\d+E)+)E", mangled)
    if not m:
        return None
    return [-int(v[1:]) if v.startswith("n") else int(v) for v in re.findall(r"L[ib](n?\d+)E", m.group(1))]


def parse_remarks(text):
    """-Rpass-analysis=kernel-resource-usage remarks -> {mangled name: {field: int}}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


_INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_STORE = re.compile(r"^(buffer_store_dword|buffer_atomic_)")  # the epilogue's forms (the amax publish is a global atomic)


def analyse_asm(text):
    """assembly text -> {mangled kernel name: {"wait0": n, "lanes": n, "stores": n}}"""
    res = {}
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        body, labels = [], {}
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            code = lines[i].split(";")[0].rstrip()
            lm = _LABEL.match(code)
            if lm:
                labels[lm.group(1)] = len(body)
            else:
                im = _INSTR.match(code)
                if im and not im.group(1).startswith("."):
                    body.append((im.group(1), im.group(2).strip()))
            i += 1
        stores = [k for k, (op, _) in enumerate(body) if _STORE.match(op)]
        wait0 = 0
        if stores:
            wait0 = sum(1 for op, arg in body[stores[0]:stores[-1] + 1] if op == "s_waitcnt" and "vmcnt(0)" in arg)
        # loops: a branch back to an earlier label; the K loop is the smallest one that holds MFMAs
        best = None
        for k, (op, arg) in enumerate(body):
            if op.startswith("s_cbranch") or op == "s_branch":
                t = labels.get(arg.split()[0] if arg else "")
                if t is not None and t <= k and any(o.startswith("v_mfma") for o, _ in body[t:k + 1]):
                    if best is None or k - t < best[1] - best[0]:
                        best = (t, k)
        lanes = loop_len = mfma = -1
        if best:
            seg = body[best[0]:best[1] + 1]
            lanes = sum(1 for o, _ in seg if o.startswith("v_readlane") or o.startswith("v_writelane"))
            loop_len = len(seg)
            mfma = sum(1 for o, _ in seg if o.startswith("v_mfma"))
        res[name] = {"wait0": wait0, "lanes": lanes, "stores": len(stores), "loop": loop_len, "loop_mfma": mfma}
    return res


def count_instructions(asm_path, tmp):
    """{mangled name: instruction count} from llvm-objdump of the assembled code object"""
    obj = os.path.join(tmp, os.path.basename(asm_path) + ".o")
    clang = os.path.join(ROCM_LLVM, "clang")
    r = subprocess.run([clang, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", f"-mcpu={build_lib.ARCH}", "-c",
                        asm_path, "-o", obj], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    d = subprocess.run([os.path.join(ROCM_LLVM, "llvm-objdump"), "-d", obj], capture_output=True, text=True).stdout
    counts, cur = {}, None
    for line in d.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
            counts[cur] = 0
        elif cur and line[:1] in ("\t", " ") and "//" in line:
            counts[cur] += 1
    return counts


def unit_report(src, csrc, inc, tmp):
    asm = os.path.join(tmp, os.path.basename(src).replace(".hip", ".s"))
    flags = [f for f in build_lib.CFLAGS if not f.startswith("-I")] + [f"-I{csrc}", f"-I{inc}"]
    cmd = [build_lib.HIPCC, *flags, "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    rem = parse_remarks(r.stderr)
    ana = analyse_asm(open(asm).read())
    cnt = count_instructions(asm, tmp)
    return [(k, rem.get(k, {}), ana[k], cnt.get(k, -1)) for k in ana]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=build_lib.CSRC)
    ap.add_argument("--include", default=os.path.join(ROOT, "include"))
    ap.add_argument("--units", default="", help="comma list of unit suffixes (k08,k38); default: every gemm_k*.hip")
    ap.add_argument("--spl", type=int, default=2, help="operand precision to list (-1: all)")
    a = ap.parse_args()
    srcs = sorted(glob.glob(os.path.join(a.csrc, "gemm_k*.hip")))
    if a.units:
        want = {f"gemm_{u}.hip" for u in a.units.split(",")}
        srcs = [s for s in srcs if os.path.basename(s) in want]
    rows = []
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(min(8, len(srcs) or 1)) as ex:
        for rep in ex.map(lambda s: unit_report(s, a.csrc, a.include, tmp), srcs):
            rows += rep
    rows = [(template_args(r[0]),) + r[1:] for r in rows]
    rows = sorted((r for r in rows if r[0] is not None), key=lambda r: r[0])
    print("# kernel <BM,BN,WGM,NW,VEC,MODE,SPL[,EPI]> | VGPRs | VGPR spill | scratch B/lane | SGPR spill | instructions |"
          " vmcnt(0) between first and last store | stores | K-loop readlane+writelane | K-loop instr / MFMAs")
    bad = 0
    for targs, rem, ana, n in rows:
        spl = targs[6]
        epi = targs[7] if len(targs) > 7 else 0
        if a.spl >= 0 and spl != a.spl:
            continue
        ok = ""
        if epi != 0:
            good = rem.get("ScratchSize [bytes/lane]", 0) == 0 and rem.get("VGPRs Spill", 0) == 0 and ana["wait0"] == 0
            ok = " ok" if good else " FAIL"
            bad += 0 if good else 1
        print(f"gemm_kernel<{','.join(map(str, targs))}> {EPI_NAMES.get(epi, epi)} | {rem.get('VGPRs', -1)} | "
              f"{rem.get('VGPRs Spill', -1)} | {rem.get('ScratchSize [bytes/lane]', -1)} | {rem.get('SGPRs Spill', -1)} | "
              f"{n} | {ana['wait0']} | {ana['stores']} | {ana['lanes']} | {ana['loop']} / {ana['loop_mfma']}{ok}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
