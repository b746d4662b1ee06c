"""The rasterizer forward entry points driven directly, at their edges (oracle/render_cases.py RASTER_CASES: partial
tiles, 1x1 .. 17x17 images, lists of 8 .. 513 records in one tile, saturated and early-stopping pixels, empty tiles,
indefinite conics, one Gaussian over every tile).

Every entry is handed the same list -- the oracle's gids / bins of raster_state(name, bw) -- so at equal block width
out_img, out_alpha, final_Ts and final_idx (a list position) have to agree bit for bit between
sfx_rasterize_fwd, sfx_rasterize_fwd_views, sfx_pack_raster_records + sfx_rasterize_fwd_views_packed,
sfx_rasterize_fwd_views_quad (block width 16 only) and sfx_rasterize_fwd_nd with 3 channels.  The three _views
entries run two views: the case, then a view whose bins are all empty, which has to come out as exactly the
background, T = 1, alpha 0.  Their clamp_max1 = 1 image has to equal torch.clamp(unclamped, max=1); the cases' own
colours and background stay below 1, so that comparison runs a second time on the same lists with the colours
times 3 and the background times 4 (red 1.2), where the clamp has to change pixels.  Output buffers are pre-filled with
NaN (-1 for final_idx) and no element may keep the fill.  Image and 1 - final_Ts are compared with the oracle's
rasterize_forward at atol 2e-4 (the bar of test_render_fused_matches_oracle); final_idx is not: the 1e-4 stop is a
discontinuity that near_threshold_pairs does not clear.
"""
import pytest
import torch

from oracle import render_cases as rc
from splatformer_amd import _lib

pytestmark = pytest.mark.gpu

f32 = torch.float32
OUTS = ["out_img", "out_alpha", "final_Ts", "final_idx"]


def _bufs(device, H, W, views=None):
    v = () if views is None else (views,)
    nan = lambda *s: torch.full(s, float("nan"), device=device, dtype=f32)
    return dict(out_img=nan(*v, H, W, 3), out_alpha=nan(*v, H, W), final_Ts=nan(*v, H, W),
                final_idx=torch.full((*v, H, W), -1, device=device, dtype=torch.int32))


def _tail(o):
    return (o["final_Ts"].data_ptr(), o["final_idx"].data_ptr(), o["out_img"].data_ptr(), o["out_alpha"].data_ptr(),
            _lib.stream())


BRIGHT = (3.0, 4.0)  # colour and background gains of the clamp test: red background 1.2, colours up to 3


def forward_entries(name, bw, device, gains=(1.0, 1.0)):
    """{entry tag: {output name: CPU tensor}} of every forward entry that takes block width bw, on the oracle's
    list of the case, colours and background multiplied by `gains`.  Tags ending in "+clamp" ran with
    clamp_max1 = 1; the _views entries return [2, H, W, ...]."""
    c, s = rc.raster_case(name), rc.raster_state(name, bw)
    H, W, n, tx, ty = c["H"], c["W"], c["n"], s["tx"], s["ty"]
    t = lambda x: x.to(device).contiguous()
    gids, xys, conics, colors, op, bg = (t(x) for x in (s["gids"], c["xys"], c["conics"], c["colors"] * gains[0],
                                                        c["opacities"], c["background"] * gains[1]))
    bins = t(s["bins"])
    bins2 = t(torch.cat([s["bins"], torch.zeros_like(s["bins"])]))  # second view: every bin empty
    arrays = (xys.data_ptr(), conics.data_ptr(), colors.data_ptr(), op.data_ptr())
    records = torch.full((n, 16), float("nan"), device=device, dtype=f32)
    _lib.call("sfx_pack_raster_records", n, *arrays, records.data_ptr(), _lib.stream())
    res = {}

    o = res["fwd"] = _bufs(device, H, W)
    _lib.call("sfx_rasterize_fwd", tx, ty, bw, H, W, gids.data_ptr(), bins.data_ptr(), *arrays, bg.data_ptr(),
              *_tail(o))
    o = res["nd3"] = _bufs(device, H, W)
    _lib.call("sfx_rasterize_fwd_nd", tx, ty, bw, H, W, 3, gids.data_ptr(), bins.data_ptr(), *arrays, bg.data_ptr(),
              *_tail(o))
    for clamp in (0, 1):
        sfx = "+clamp" if clamp else ""
        o = res["views" + sfx] = _bufs(device, H, W, 2)
        _lib.call("sfx_rasterize_fwd_views", 2, tx, ty, bw, H, W, gids.data_ptr(), bins2.data_ptr(), *arrays,
                  bg.data_ptr(), clamp, *_tail(o))
        for entry in ["packed"] + (["quad"] if bw == 16 else []):
            o = res[entry + sfx] = _bufs(device, H, W, 2)
            _lib.call(f"sfx_rasterize_fwd_views_{entry}", 2, tx, ty, bw, H, W, gids.data_ptr(), bins2.data_ptr(),
                      records.data_ptr(), bg.data_ptr(), clamp, *_tail(o))
    torch.cuda.synchronize()
    return {k: {nm: v[nm].cpu() for nm in OUTS} for k, v in res.items()}


_CACHE = {}


def _entries(device, name, bw, gains=(1.0, 1.0)):
    """forward_entries, run once per (case, block width, gains) and shared by the tests below"""
    key = (name, bw, gains)
    if key not in _CACHE:
        _CACHE[key] = forward_entries(name, bw, device, gains)
    return _CACHE[key]


@pytest.mark.parametrize("bw", [16, 8])
@pytest.mark.parametrize("name", rc.RASTER_CASES)
def test_forward_entries_agree_bitwise(device, name, bw):
    res = _entries(device, name, bw)
    assert set(res) == {"fwd", "nd3", "views", "views+clamp", "packed", "packed+clamp"} | (
        {"quad", "quad+clamp"} if bw == 16 else set())
    base = res["fwd"]
    for tag, o in res.items():
        for nm in OUTS:
            fill = (o[nm] == -1) if nm == "final_idx" else torch.isnan(o[nm])
            assert not bool(fill.any()), f"{name}@{bw} {tag}: {int(fill.sum())} elements of {nm} keep the fill"
        if tag == "fwd":
            continue
        first = {nm: (o[nm][0] if o[nm].dim() == base[nm].dim() + 1 else o[nm]) for nm in OUTS}
        for nm in OUTS:
            want = torch.clamp(base[nm], max=1) if (tag.endswith("+clamp") and nm == "out_img") else base[nm]
            assert torch.equal(first[nm], want), f"{name}@{bw} {tag}: {nm} differs from sfx_rasterize_fwd"


@pytest.mark.parametrize("bw", [16, 8])
@pytest.mark.parametrize("name", rc.RASTER_CASES)
def test_forward_clamp_changes_bright_pixels(device, name, bw):
    """clamp_max1 on inputs that exceed 1: every _views entry equals torch.clamp(unclamped, max=1) bit for bit, in
    both views (the empty one: the clamped background), the clamp changes at least one element of the case's view,
    and nothing but the image depends on it."""
    res = _entries(device, name, bw, BRIGHT)
    base = res["fwd"]
    want = torch.clamp(base["out_img"], max=1)
    assert int((want != base["out_img"]).sum()) > 0, f"{name}@{bw}: no pixel above 1, the clamp is not exercised"
    bg = torch.clamp(rc.raster_case(name)["background"] * BRIGHT[1], max=1)
    for tag in ["views", "packed"] + (["quad"] if bw == 16 else []):
        plain, clamped = res[tag], res[tag + "+clamp"]
        assert torch.equal(plain["out_img"][0], base["out_img"]), f"{name}@{bw} {tag}: unclamped image"
        assert torch.equal(clamped["out_img"][0], want), f"{name}@{bw} {tag}: clamped image"
        assert torch.equal(clamped["out_img"], torch.clamp(plain["out_img"], max=1)), f"{name}@{bw} {tag}"
        assert torch.equal(clamped["out_img"][1], bg.expand_as(want)), f"{name}@{bw} {tag}: empty view"
        for nm in ("out_alpha", "final_Ts", "final_idx"):
            assert torch.equal(clamped[nm], plain[nm]), f"{name}@{bw} {tag}: {nm} depends on the clamp"


@pytest.mark.parametrize("bw", [16, 8])
@pytest.mark.parametrize("name", rc.RASTER_CASES)
def test_forward_empty_second_view(device, name, bw):
    """A view whose bins are all empty: exactly the background (below 1: the clamp changes nothing), T = 1, alpha 0."""
    c = rc.raster_case(name)
    for tag, o in _entries(device, name, bw).items():
        if o["out_img"].dim() != 4:
            continue
        assert torch.equal(o["out_img"][1], c["background"].expand(c["H"], c["W"], 3)), f"{name}@{bw} {tag}"
        assert torch.equal(o["final_Ts"][1], torch.ones(c["H"], c["W"])), f"{name}@{bw} {tag}"
        assert torch.equal(o["out_alpha"][1], torch.zeros(c["H"], c["W"])), f"{name}@{bw} {tag}"
        assert torch.equal(o["final_idx"][1], torch.zeros(c["H"], c["W"], dtype=torch.int32)), f"{name}@{bw} {tag}"


@pytest.mark.parametrize("bw", [16, 8])
@pytest.mark.parametrize("name", rc.RASTER_CASES)
def test_forward_matches_oracle(device, name, bw):
    """sfx_rasterize_fwd against the oracle; the other entries are tied to it bit for bit by
    test_forward_entries_agree_bitwise."""
    s, o = rc.raster_state(name, bw), _entries(device, name, bw)["fwd"]
    torch.testing.assert_close(o["out_img"], s["img"], rtol=0, atol=2e-4)
    torch.testing.assert_close(o["out_alpha"], 1 - s["final_Ts"], rtol=0, atol=2e-4)
    torch.testing.assert_close(1 - o["final_Ts"], 1 - s["final_Ts"], rtol=0, atol=2e-4)
