"""Same bits from two builds of libsfx: the image loss, the fused evaluation metrics and the LPIPS input stage on
identical seeded inputs, one process per library (SFX_LIB), then compared with torch.equal.
    SFX_LIB=/path/parent.so python tools/image_same_bits.py dump a.pt
    SFX_LIB=/path/new.so    python tools/image_same_bits.py dump b.pt
    python tools/image_same_bits.py compare a.pt b.pt
Dumped under "same/": sfx_image_loss terms and d_pred over the shapes, input kinds and weight pairs of
tests/test_gpu_image_loss.py, with and without view_scale, forward only and with gradient; sfx_eval_metrics_u8 sums,
maxes and ssim over the cases of tests/test_gpu_eval_masked.py in the RGBA, RGB + dense mask and RGB no-mask forms,
and on 9 views of 800 x 800; sfx_lpips_input with and without quantisation and mask.
Dumped under "moved/": the SSIM metrics.ssim returns for 3-channel quantised and for unquantised inputs over the same
shapes and at 9 x 800 x 800.  A library that still exports the 121-tap entry (the parent of the change that retired
it) is called through that entry, as metrics.ssim did then; compare reports max |a - b| per group instead of
equality.  That branch (`_ssim`'s hand-written binding) serves the comparison with that one parent only and can go
once no such library is compared any more."""
import ctypes
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _ssim(a, b, quantize):
    """metrics.ssim, or the retired 121-tap entry where the library still has it."""
    from splatformer_amd import _lib, metrics
    lib = _lib.lib()
    if not hasattr(lib, "sfx_ssim"):
        return metrics.ssim(a, b, quantize_u8=quantize)
    I, P, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.sfx_ssim_workspace_bytes.argtypes, lib.sfx_ssim_workspace_bytes.restype = [I, I, I, I], Z
    lib.sfx_ssim.argtypes = [I, I, I, I, P, P, P, I, P, P, Z, P]
    V, H, W, C = a.shape
    a, b = a.float().contiguous(), b.float().contiguous()
    win = metrics.ssim_window().reshape(-1).to(a.device)
    ws = torch.empty(max(int(lib.sfx_ssim_workspace_bytes(V, H, W, C)), 4), dtype=torch.uint8, device=a.device)
    out = torch.empty(V, dtype=torch.float32, device=a.device)
    rc = lib.sfx_ssim(V, H, W, C, a.data_ptr(), b.data_ptr(), win.data_ptr(), int(quantize), out.data_ptr(),
                      ws.data_ptr(), ws.numel(), _lib.stream())
    assert rc == 0, lib.sfx_last_error()
    return out


def dump(path):
    from splatformer_amd import losses, lpips, metrics
    host = _module("test_image_loss_host")
    masked = _module("test_gpu_eval_masked")
    dev = torch.device("cuda:0")
    out = {}
    for shape in host.SHAPES + [(2, 64, 64, 3)]:
        for kind in ("noise", "indep", "flat"):
            pred, gt = (t.to(dev) for t in host.make_inputs(shape, kind))
            tag = "x".join(map(str, shape)) + "/" + kind
            out[f"moved/ssim/{tag}"] = _ssim(pred, gt, False).cpu()
            for l1w, sw in ((0.0, 1.0), (0.75, 0.25), (1.0, 0.0)):
                out[f"same/loss/{tag}/{l1w}-{sw}/fwd_terms"] = losses.image_loss_terms(pred, gt, l1w, sw).cpu()
                for scale in (None, host.upstream(shape[0], torch.float32).to(dev)):
                    terms, d = losses.image_loss_and_grad(pred, gt, l1w, sw, scale)
                    s = "scaled" if scale is not None else "unscaled"
                    out[f"same/loss/{tag}/{l1w}-{sw}/{s}/terms"] = terms.cpu()
                    out[f"same/loss/{tag}/{l1w}-{sw}/{s}/d_pred"] = d.cpu()

    def metrics_forms(tag, pred, rgba):
        gt3, m = rgba[..., :3].contiguous(), rgba[..., 3].contiguous()
        for clamp in (True, False):
            forms = {"rgba": (rgba, None), "rgb_mask": (gt3, m), "rgb": (gt3, None)}
            for form, (gt, mask) in forms.items():
                r = metrics.eval_stats_u8(pred, gt, mask, clamp_pred=clamp)
                for nm, t in zip(("sums", "maxes", "ssim"), r):
                    out[f"same/eval/{tag}/clamp{int(clamp)}/{form}/{nm}"] = t.cpu()
        out[f"moved/ssim_u8/{tag}"] = _ssim(pred, gt3, True).cpu()

    for shape, kind in masked.CASES:
        c = masked.case(shape, kind)
        metrics_forms("x".join(map(str, shape)) + "/" + kind, c["pred"].to(dev), c["rgba"].to(dev))
    g = torch.Generator().manual_seed(0)
    V, H, W = 9, 800, 800
    gt = torch.rand(V, H, W, 3, generator=g)
    pred = (gt + 0.05 * torch.randn(V, H, W, 3, generator=g)).clamp(0, 1).to(dev)
    m = masked.blob_mask(V, H, W)
    rgba = torch.cat([gt * m[..., None], m[..., None]], -1).contiguous().to(dev)
    metrics_forms("9x800x800", pred, rgba)
    gt = gt.to(dev)
    out["moved/ssim_u8/9x800x800/rgb"] = _ssim(pred, gt, True).cpu()
    out["moved/ssim/9x800x800x3"] = _ssim(pred, gt, False).cpu()
    terms, d = losses.image_loss_and_grad(pred, gt, 0.8, 0.2)
    out["same/loss/9x800x800x3/terms"], out["same/loss/9x800x800x3/d_pred"] = terms.cpu(), d.cpu()

    x = (torch.rand(2, 37, 50, 3, generator=g) * 1.1).to(dev)
    mask = torch.randint(0, 256, (2, 37, 50), generator=g).float().div(255).to(dev)
    for q in (False, True):
        for nm, mk in (("nomask", None), ("mask", mask)):
            out[f"same/lpips_input/q{int(q)}/{nm}"] = lpips.lpips_input(x, mask=mk, quantize_u8=q).cpu()
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"{len(out)} tensors -> {path} (library {os.environ.get('SFX_LIB', 'in-tree')})")


def compare(pa, pb):
    A, B = torch.load(pa), torch.load(pb)
    assert set(A) == set(B), sorted(set(A) ^ set(B))
    eq = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and (  # noqa: E731
        torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y))
    same = [k for k in sorted(A) if k.startswith("same/")]
    bad = [k for k in same if not eq(A[k], B[k])]
    groups = {}
    for k in same:
        groups[k.split("/")[1]] = groups.get(k.split("/")[1], 0) + 1
    print(f"{len(same)} tensors that must not move ({', '.join(f'{v} {k}' for k, v in sorted(groups.items()))}): "
          f"{'all bit-identical' if not bad else f'{len(bad)} DIFFER: {bad[:10]}'}")
    moved = {}
    for k in sorted(A):
        if k.startswith("moved/"):
            grp = k.split("/")[1] + (" at 9 x 800 x 800" if "9x800x800" in k else " over the test shapes")
            d = float((A[k].double() - B[k].double()).abs().max())
            n, worst, at = moved.get(grp, (0, -1.0, ""))
            moved[grp] = (n + 1, max(worst, d), k if d > worst else at)
    for grp, (n, worst, at) in sorted(moved.items()):
        print(f"the SSIM that may move, {grp}: {n} tensors, max |a - b| = {worst:.3e} (at {at})")
    for k in sorted(A):  # the unquantised SSIM per input kind: the fp32 121-tap sum cancels on flat inputs
        if k.startswith("moved/ssim/") and "9x800x800" not in k:
            print(f"  {k}: |a - b| = {float((A[k].double() - B[k].double()).abs().max()):.3e}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
