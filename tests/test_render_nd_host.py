"""Host side of the N-channel rasterizer (no GPU needed): the two C-ABI entries are exported, validate their
arguments before any launch, and the Python shim has no CPU fallback for C != 3."""
import pytest
import torch

FWD_ARGS = [None] * 12   # gids_sorted .. out_alpha, stream
BWD_ARGS = [None] * 17   # gids_sorted .. v_opacity, stream


def _load():
    from splatformer_amd import _lib, gsplat_compat  # noqa: F401  (gsplat_compat registers the signatures)
    return _lib.load()


def test_entries_exported_and_bound():
    from splatformer_amd import _lib
    lib = _load()
    for name in ("sfx_rasterize_fwd_nd", "sfx_rasterize_bwd_nd"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sfx_rasterize_fwd_nd"]) == 6 + len(FWD_ARGS)
    assert len(_lib.SIGNATURES["sfx_rasterize_bwd_nd"]) == 6 + len(BWD_ARGS)
    assert lib.sfx_abi_version() == 17


@pytest.mark.parametrize("channels", [0, 33, -1])
def test_channel_range_is_validated_before_any_launch(channels):
    lib = _load()
    # 32 x 32 image, 2 x 2 tiles of 16: everything valid but the channel count (and the null buffers behind it)
    rc = lib.sfx_rasterize_fwd_nd(2, 2, 16, 32, 32, channels, *FWD_ARGS)
    assert rc == -1
    msg = lib.sfx_last_error()
    assert b"sfx_rasterize_fwd_nd" in msg and b"channels" in msg and b"[1,32]" in msg
    rc = lib.sfx_rasterize_bwd_nd(2, 2, 16, 32, 32, channels, *BWD_ARGS)
    assert rc == -1
    msg = lib.sfx_last_error()
    assert b"sfx_rasterize_bwd_nd" in msg and b"channels" in msg and b"[1,32]" in msg


@pytest.mark.parametrize("tx,ty,bw,h,w", [(2, 2, 1, 32, 32), (2, 2, 17, 32, 32), (2, 2, 16, -32, 32),
                                          (2, 2, 16, 32, -32), (3, 2, 16, 32, 32)])
def test_bad_block_width_or_size(tx, ty, bw, h, w):
    lib = _load()
    assert lib.sfx_rasterize_fwd_nd(tx, ty, bw, h, w, 4, *FWD_ARGS) == -1
    assert b"sfx_rasterize_fwd_nd" in lib.sfx_last_error()
    assert lib.sfx_rasterize_bwd_nd(tx, ty, bw, h, w, 4, *BWD_ARGS) == -1
    assert b"sfx_rasterize_bwd_nd" in lib.sfx_last_error()


def test_null_buffers_are_refused():
    lib = _load()
    assert lib.sfx_rasterize_fwd_nd(2, 2, 16, 32, 32, 4, *FWD_ARGS) == -1
    assert b"null buffer" in lib.sfx_last_error()
    assert lib.sfx_rasterize_bwd_nd(2, 2, 16, 32, 32, 4, *BWD_ARGS) == -1
    assert b"null buffer" in lib.sfx_last_error()


def test_no_cpu_fallback_for_n_channels():
    from splatformer_amd import gsplat_compat
    n = 4
    with pytest.raises(RuntimeError) as e:
        gsplat_compat.rasterize_gaussians(torch.rand(n, 2), torch.rand(n), torch.ones(n, dtype=torch.int32),
                                          torch.rand(n, 3), torch.ones(n, dtype=torch.int32), torch.rand(n, 5),
                                          torch.rand(n, 1), 16, 16, 16)
    assert not isinstance(e.value, NotImplementedError)
