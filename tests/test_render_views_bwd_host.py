"""Host side of the batched training render's two backward entries (no GPU needed): they are exported with the
pinned signatures, and every invalid argument is refused before any launch with a message that names it."""
import ctypes

import pytest

I, L, F, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p
RAST = "sfx_rasterize_bwd_views_quad"
PREP = "sfx_render_prep_project_views_bwd"
X = 1 << 20  # a non-null "pointer": validation never dereferences it.  Every call below is invalid: the scalar
# cases leave the buffers checked last null as well, so no argument list here could ever reach a launch


def _lib():
    from splatformer_amd import _lib
    return _lib, _lib.load()


def test_pinned_signatures():
    mod, lib = _lib()
    assert mod.SIGNATURES[RAST] == [I] * 6 + [P] * 17
    assert mod.SIGNATURES[PREP] == ([I, I, I] + [P, L] * 6 + [P, F, F] + [P] * 6 + [P, L] * 6 + [P])
    for name in (RAST, PREP):
        assert getattr(lib, name).argtypes == mod.SIGNATURES[name]
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.sfx_abi_version() == 17


def _rast(views=2, tx=2, ty=2, bw=16, h=32, w=32, bufs=None):
    bufs = [None] * 16 if bufs is None else bufs  # gids_sorted .. v_opacity
    return [views, tx, ty, bw, h, w, *bufs, None]


def _prep(n=8, views=2, nb=4, attrs=None, cams=X, per_view=None, grads=None):
    attrs = [X, 3, X, 3, X, 4, X, 1, X, 3, X, 9] if attrs is None else attrs
    per_view = [X] * 6 if per_view is None else per_view
    grads = [None, 3, None, 3, None, 4, None, 1, None, 3, None, 9] if grads is None else grads
    return [n, views, nb, *attrs, cams, 100.0, 100.0, *per_view, *grads, None]


def _refused(lib, name, args, *words):
    assert getattr(lib, name)(*args) == -1  # SFX_ERR_INVALID
    msg = lib.sfx_last_error()
    assert name.encode() in msg
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("views", [0, -1, 65536])
def test_views_are_validated(views):
    _, lib = _lib()
    _refused(lib, RAST, _rast(views=views), b"views")
    _refused(lib, PREP, _prep(views=views), b"views")


@pytest.mark.parametrize("bw", [8, 15, 17, 0])
def test_block_width_must_be_16(bw):
    _, lib = _lib()
    _refused(lib, RAST, _rast(bw=bw), b"block_width must be 16")


@pytest.mark.parametrize("tx,ty,h,w", [(3, 2, 32, 32), (2, 2, 33, 32), (2, 2, -32, 32), (2, 2, 32, 0)])
def test_tile_bounds_must_match_the_image(tx, ty, h, w):
    _, lib = _lib()
    _refused(lib, RAST, _rast(tx=tx, ty=ty, h=h, w=w), b"tile bounds")


@pytest.mark.parametrize("nb", [0, 2, 3, 5, 24, 36, -1])
def test_num_bases_is_validated(nb):
    _, lib = _lib()
    _refused(lib, PREP, _prep(nb=nb), b"num_bases", b"{1,4,9,16,25}")


def test_negative_n_and_int32_overflow():
    _, lib = _lib()
    _refused(lib, PREP, _prep(n=-1), b"n < 0")
    _refused(lib, PREP, _prep(n=1 << 30, views=4), b"views * n")


# v_out_alpha (index 10) and v_xy_abs (index 12) are the nullable buffers of the rasterizer entry
@pytest.mark.parametrize("k", [k for k in range(16) if k not in (10, 12)])
def test_rasterizer_required_pointers(k):
    _, lib = _lib()
    bufs = [X] * 16
    bufs[k] = None
    _refused(lib, RAST, _rast(bufs=bufs), b"null buffer")


def test_prep_required_pointers():
    _, lib = _lib()
    _refused(lib, PREP, _prep(cams=None), b"null cameras")
    for k in range(0, 12, 2):  # means .. features_rest (required at num_bases 4)
        attrs = [X, 3, X, 3, X, 4, X, 1, X, 3, X, 9]
        attrs[k] = None
        _refused(lib, PREP, _prep(attrs=attrs), b"null input buffer")
        grads = [X, 3, X, 3, X, 4, X, 1, X, 3, X, 9]
        grads[k], attrs[k] = None, X
        _refused(lib, PREP, _prep(attrs=attrs, grads=grads), b"null gradient buffer")
    for k in range(6):  # radii, conics, v_xys, v_conics, v_rgbs, v_opacities
        pv = [X] * 6
        pv[k] = None
        _refused(lib, PREP, _prep(per_view=pv), b"null per-view buffer")


def test_python_surface():
    """The public wrappers and the Trainer argument exist; an unknown render mode is refused by name."""
    from splatformer_amd import gs_render, train
    assert callable(gs_render.rasterize_gaussians_to_multiimgs_batched)
    assert callable(gs_render.rasterize_packed_to_multiimgs_batched)
    assert train.RENDER_MODES == ("per_view", "batched")
