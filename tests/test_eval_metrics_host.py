"""sfx_eval_metrics_u8 / metrics.eval_metrics_u8 without a GPU: the library loads, every refusal the header lists
returns rc < 0 with a message naming the entry point (nothing is launched), an empty batch is fine, the workspace
query is monotone, and the Python wrapper rejects wrong shapes before it asks for a device."""
import ctypes

import pytest
import torch

V, H, W = 2, 20, 40
P = 4096  # a non-null, 16-byte aligned pointer value; every case below is refused before anything reads it
NAME = b"sfx_eval_metrics_u8"


def _lib():
    from splatformer_amd import _lib
    return _lib.load()


def _call(lib, **over):
    a = dict(num_images=V, height=H, width=W, pred=P, gt=P, gt_pixel_stride=4, mask=P + 12, mask_pixel_stride=4,
             clamp_pred=1, window=P, sums=P, maxes=P, ssim=P, ws=P,
             ws_bytes=lib.sfx_eval_metrics_workspace_bytes(V, H, W), stream=None)
    a.update(over)
    return lib.sfx_eval_metrics_u8(*a.values())


def test_signatures_are_bound_from_the_header():
    from splatformer_amd import _lib as L
    I, Z, Pv = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
    assert L.SIGNATURES["sfx_eval_metrics_workspace_bytes"] == [I, I, I]
    assert L.SIGNATURES["sfx_eval_metrics_u8"] == [I, I, I, Pv, Pv, I, Pv, I, I, Pv, Pv, Pv, Pv, Pv, Z, Pv]
    lib = _lib()
    assert lib.sfx_eval_metrics_workspace_bytes.restype is Z
    assert lib.sfx_abi_version() == 17


@pytest.mark.parametrize("over,word", [
    (dict(num_images=-1), b"sizes"),
    (dict(height=0), b"sizes"),
    (dict(width=0), b"sizes"),
    (dict(width=-3), b"sizes"),
    (dict(gt_pixel_stride=5), b"gt_pixel_stride"),
    (dict(gt_pixel_stride=1), b"gt_pixel_stride"),
    (dict(mask_pixel_stride=3), b"mask_pixel_stride"),
    (dict(mask_pixel_stride=0), b"mask_pixel_stride"),
    (dict(pred=None), b"null"),
    (dict(gt=None, mask=None), b"null"),
    (dict(window=None), b"null"),
    (dict(sums=None), b"null"),
    (dict(maxes=None), b"null"),
    (dict(ssim=None), b"null"),
    (dict(ws=None), b"null"),
    (dict(ws_bytes=7), b"workspace"),
    (dict(ws=P + 4), b"aligned"),
    (dict(num_images=65536, height=1, width=1, ws_bytes=1 << 30), b"65535"),
])
def test_refusals_name_the_entry_point(over, word):
    lib = _lib()
    rc = _call(lib, **over)
    msg = lib.sfx_last_error()
    assert rc < 0
    assert msg.startswith(NAME) and word in msg, msg


def test_short_workspace_is_refused_by_one_byte():
    lib = _lib()
    need = lib.sfx_eval_metrics_workspace_bytes(V, H, W)
    assert need >= 8
    assert _call(lib, ws_bytes=need - 1) < 0
    assert b"workspace too small" in lib.sfx_last_error()


def test_no_mask_ignores_the_mask_stride():
    """mask == NULL: the stride is not looked at; the call gets as far as the next check (a null buffer here)."""
    lib = _lib()
    rc = _call(lib, mask=None, mask_pixel_stride=0, pred=None)
    assert rc < 0 and b"null buffer" in lib.sfx_last_error()


def test_empty_batch_is_ok():
    lib = _lib()
    assert _call(lib, num_images=0, pred=None, gt=None, mask=None, window=None, sums=None, maxes=None, ssim=None,
                 ws=None, ws_bytes=0) == 0
    assert lib.sfx_eval_metrics_workspace_bytes(0, H, W) == 0


def test_workspace_query_is_monotone():
    lib = _lib()
    q = lib.sfx_eval_metrics_workspace_bytes
    for fixed in (1, 7, 33):
        for k in range(3):
            sizes = [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 130, 800, 4096]
            got = []
            for s in sizes:
                a = [fixed] * 3
                a[k] = s
                got.append(q(*a))
            assert got == sorted(got), (fixed, k, got)
            assert got[0] >= 8 and got[-1] > got[0]
    assert q(-1, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, 0) == 0  # the sizes the call refuses


def test_python_wrapper_rejects_shapes_before_it_needs_a_device():
    from splatformer_amd import metrics
    pred = torch.zeros(2, 8, 8, 3)
    with pytest.raises(ValueError):
        metrics.eval_metrics_u8(pred, torch.zeros(2, 8, 8, 5))
    with pytest.raises(ValueError):
        metrics.eval_metrics_u8(pred, torch.zeros(2, 8, 9, 3))
    with pytest.raises(ValueError):
        metrics.eval_metrics_u8(pred, torch.zeros(3, 8, 8, 4))
    with pytest.raises(ValueError):
        metrics.eval_metrics_u8(torch.zeros(2, 8, 8, 4), torch.zeros(2, 8, 8, 4))
    with pytest.raises(ValueError):
        metrics.eval_metrics_u8(pred, torch.zeros(2, 8, 8, 3), mask=torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError):
        metrics.eval_metrics_u8(pred, torch.zeros(2, 8, 8, 4), mask=torch.zeros(2, 8))


def test_retired_entries_are_gone():
    """ABI v17: the uint8-moments entry and the 121-tap SSIM pair are neither declared nor bound nor exported."""
    import os
    from splatformer_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfx.h")).read()
    lib = _lib()
    for name in ("sfx_ssim", "sfx_ssim_workspace_bytes", "sfx_image_stats_u8"):
        assert name not in L.SIGNATURES
        assert name + "(" not in header and name + " " not in header
        assert not hasattr(lib, name)
    assert lib.sfx_abi_version() == 17


def test_thin_callers_reject_shapes_before_they_need_a_device():
    from splatformer_amd import metrics
    rgb, rgba, flat = torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 4), torch.zeros(2, 192)
    for a, b in ((rgba, rgba), (flat, flat), (rgb, rgba), (rgb, torch.zeros(2, 8, 9, 3)), (rgb[0], rgb[0])):
        with pytest.raises(ValueError):
            metrics.psnr_u8(a, b)
        with pytest.raises(ValueError):
            metrics.image_stats_u8(a, b)
        with pytest.raises(ValueError):
            metrics.ssim(a, b, quantize_u8=True)
    with pytest.raises(ValueError):
        metrics.ssim(rgb, rgba)
    with pytest.raises(ValueError):
        metrics.ssim(rgb[0], rgb[0])
