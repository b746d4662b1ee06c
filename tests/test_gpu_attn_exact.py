"""The exact fp32-MFMA attention kernels (SFX_ATTN_PREC=fp32: window_attn_kernel, window_attn_flash_kernel,
window_attn_bwd_kernel) vs the fp64 reference math.

The switch is read once per process, so the check runs in one fresh child process with SFX_ATTN_PREC=fp32 added to
the inherited environment (this file's __main__ block); the test asserts on the child's exit status and on the
figures it prints.  Bars: the ones the default kernels are held to -- forward relative L2 < 2e-6
(test_window_attention_vs_reference_padding), backward < 1e-5 (test_window_attention_bwd).

Shapes: n = 77 (one short window, K = n) and n = 129 (K = 128, a ragged second window whose keys are shared with
the first) for the windowed forward and backward; key counts [5, 1, 130, 259] at K = 128 for the varlen forward (one
tiny window, a single key, two batches that need a second, ragged window); head dims 16, 24 and 32."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_BAR, BWD_BAR = 2e-6, 1e-5
SHAPES = [(2, 32), (4, 96), (4, 128)]  # (heads, C): head dims 16, 24, 32
WINDOW_N = [77, 129]
VARLEN_COUNTS, VARLEN_K = [5, 1, 130, 259], 128


def _child():
    sys.path.insert(0, ROOT)
    import torch

    from oracle import ptv3_ref
    from splatformer_amd import _lib
    from splatformer_amd import ptv3_ops as ops
    from splatformer_amd import train_ops as tops

    _lib.load()
    dev = torch.device("cuda:0")

    def rel_l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).norm() / b.norm().clamp_min(1e-30))

    res = []
    for heads, C in SHAPES:
        for n in WINDOW_N:
            g = torch.Generator().manual_seed(n + C)
            qkv = torch.randn(n, 3 * C, generator=g)
            order = torch.randperm(n, generator=g)
            inverse = torch.empty_like(order)
            inverse[order] = torch.arange(n)
            K = min(n, 128)
            pad, unpad = ptv3_ref.get_padding_and_inverse(torch.tensor([n]), K)
            q64 = qkv.double().requires_grad_()
            q, k, v = q64[order[pad]].reshape(-1, K, 3, heads, C // heads).permute(2, 0, 3, 1, 4).unbind(0)
            att = torch.softmax((q * (C // heads) ** -0.5) @ k.transpose(-2, -1), -1)
            ref = (att @ v).transpose(1, 2).reshape(-1, C)[unpad[inverse]]
            dout = torch.randn(n, C, generator=g)
            ref.backward(dout.double())
            tab = ops.window_table([n], K)
            win = torch.tensor(tab, dtype=torch.int32).to(dev)
            qd, od = qkv.to(dev), order.int().to(dev)
            out = ops.window_attention(qd, od, win, len(tab), K, heads, C)
            res.append({"case": f"fwd n={n} heads={heads} C={C}", "err": rel_l2(out, ref), "bar": FWD_BAR})
            dqkv = tops.window_attention_bwd(qd, od, win, len(tab), K, heads, C, dout.to(dev))
            res.append({"case": f"bwd n={n} heads={heads} C={C}", "err": rel_l2(dqkv, q64.grad), "bar": BWD_BAR})
        counts, K = VARLEN_COUNTS, VARLEN_K
        n = sum(counts)
        offset = torch.tensor(counts).cumsum(0)
        g = torch.Generator().manual_seed(K + C)
        qkv = torch.randn(n, 3 * C, generator=g).double()  # fp32 values: the kernel and the reference see the same
        batch = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
        order = torch.cat([torch.randperm(c, generator=g) + (int(offset[i]) - c) for i, c in enumerate(counts)])
        inverse = torch.empty_like(order)
        inverse[order] = torch.arange(n)
        point = ptv3_ref.Point(offset=offset, serialized_order=order[None], serialized_inverse=inverse[None],
                               batch=batch)
        ref = ptv3_ref.serialized_attention_flash(qkv, point, C, heads, K, 0)
        tab = ops.window_table_varlen_np(offset.tolist(), K)
        win3 = torch.from_numpy(tab).to(dev)
        out = ops.window_attention_varlen(qkv.float().to(dev), order.int().to(dev), win3, tab.shape[0], K, heads, C)
        res.append({"case": f"varlen counts={counts} K={K} heads={heads} C={C}", "err": rel_l2(out, ref),
                    "bar": FWD_BAR})
    for r in res:
        print(f"[attn exact] {r['case']}: rel L2 {r['err']:.3e} (bar {r['bar']:.0e})")
    ok = all(r["err"] < r["bar"] for r in res)  # (a NaN fails)
    print("ATTN_EXACT_RESULT " + json.dumps({"ok": ok, "cases": res}))
    return 0 if ok else 1


@pytest.mark.gpu
def test_attention_exact_fp32_kernels(device):
    env = dict(os.environ)
    env["SFX_ATTN_PREC"] = "fp32"
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=180)
    print(p.stdout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ATTN_EXACT_RESULT ")]
    assert lines, f"child printed no result (exit status {p.returncode}):\n{p.stdout}\n{p.stderr}"
    result = json.loads(lines[-1][len("ATTN_EXACT_RESULT "):])
    assert len(result["cases"]) == len(SHAPES) * (2 * len(WINDOW_N) + 1)
    bad = [c for c in result["cases"] if not c["err"] < c["bar"]]
    assert not bad, bad
    assert p.returncode == 0 and result["ok"], p.stderr


if __name__ == "__main__":
    sys.exit(_child())
