"""Plain, differentiable, dtype-generic references of the render operators, for pinning the hand-written vjp
restatements of oracle/gsplat_ref.py (and through them the HIP backward kernels) to autograd of the forward.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Nothing here culls, clamps to the frustum, or produces integers: these are the smooth functions whose
derivatives gsplat's backward kernels state by hand.  Evaluate them in float64.
"""
from __future__ import annotations

import torch

BLUR = 0.3


def rotmat_raw(q: torch.Tensor) -> torch.Tensor:
    """R(w,x,y,z) of gsplat's quat_to_rotmat WITHOUT the normalisation: the function gsplat's quat_to_rotmat_vjp
    differentiates (it evaluates that derivative at q/|q|).  Equal to the rotation of q only where |q| = 1."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def unpack_sym3(c: torch.Tensor) -> torch.Tensor:
    return torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]],
                       -1).reshape(-1, 3, 3)


def project_smooth(means, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, frustum_lim=None):
    """The smooth part of project_gaussians: returns (xys, depths, conics, compensation, cov2d, cov3d).
    frustum_lim = (lim_x, lim_y) puts the forward's clamp of tx/tz, ty/tz in the EWA Jacobian back (only for
    showing that gsplat's vjp ignores it).

    Pixel centre with rw = 1/(tz + 1e-6); EWA Jacobian with 1/tz and no frustum clamp; blur 0.3 on the diagonal;
    rotation from the quaternion as given (rotmat_raw -- pass unit quaternions).  cov3d [n,6] and cov2d [n,3]
    (blurred) are graph nodes in gsplat's packing: everything downstream reads both off-diagonal entries from
    the one packed value, so torch.autograd.grad w.r.t. them gives gsplat's v_cov3d / v_cov2d (off-diagonal
    entries summed)."""
    dt = means.dtype
    vm = viewmat.reshape(-1)[:12].to(dt).reshape(3, 4)
    W, t0 = vm[:, :3], vm[:, 3]
    t = means @ W.T + t0[None]
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    R = rotmat_raw(quats)
    M = R * (glob_scale * scales)[:, None, :]
    Vfull = M @ M.transpose(1, 2)
    cov3d = torch.stack([Vfull[:, 0, 0], Vfull[:, 0, 1], Vfull[:, 0, 2], Vfull[:, 1, 1], Vfull[:, 1, 2],
                         Vfull[:, 2, 2]], -1)
    V = unpack_sym3(cov3d)
    rz = 1.0 / tz
    zero = torch.zeros_like(tz)
    jx, jy = tx, ty
    if frustum_lim is not None:
        jx = tz * torch.clamp(tx / tz, min=-frustum_lim[0], max=frustum_lim[0])
        jy = tz * torch.clamp(ty / tz, min=-frustum_lim[1], max=frustum_lim[1])
    J = torch.stack([fx * rz, zero, -fx * jx * rz * rz, zero, fy * rz, -fy * jy * rz * rz], -1).reshape(-1, 2, 3)
    T = J @ W
    C = T @ V @ T.transpose(1, 2)
    cov2d = torch.stack([C[:, 0, 0] + BLUR, C[:, 0, 1], C[:, 1, 1] + BLUR], -1)
    a, b, c = cov2d[:, 0], cov2d[:, 1], cov2d[:, 2]
    det = a * c - b * b
    det_orig = (a - BLUR) * (c - BLUR) - b * b
    compensation = torch.sqrt(torch.clamp(det_orig / det, min=0.0))
    conics = torch.stack([c / det, -b / det, a / det], -1)
    rw = 1.0 / (tz + 1e-6)
    xys = torch.stack([tx * rw * fx + cx, ty * rw * fy + cy], -1)
    return xys, tz, conics, compensation, cov2d, cov3d


def composite_masked(pix, xys, conics, colors, opacity, background, g, valid, pos, final_idx, alpha_clamp=0.99,
                     include_final=True, with_background=True, pair_offset=None):
    """Front-to-back composite of the list `g` (Gaussian ids, list order) at the pixel centres pix[P,2]:
    rgb = sum_i alpha_i T_i c_i + T_last bg, alpha_out = 1 - T_last, alpha_i = min(alpha_clamp, o_i exp(-sigma_i)).

    Record j (list position pos[j]) contributes to pixel p where valid[p,j] and pos[j] <= final_idx[p]
    (include_final=False: <); all other records are transparent for that pixel.  The mask is data, not part of
    the differentiated function.  The three keyword parameters are gsplat's choices; other values give the wrong
    variants tests/test_oracle_render_grad.py shows the bars reject.  pair_offset [P,m,2] (zeros) is added to the
    Gaussian centre per (pixel, record): its gradient is the per-pixel v_xy, whose absolute sum is v_xy_abs.
    Returns (rgb[P,3], alpha_out[P], T_last[P])."""
    dt = xys.dtype
    g = g.long()
    dx = xys[g, 0][None] - pix[:, 0:1].to(dt)
    dy = xys[g, 1][None] - pix[:, 1:2].to(dt)
    if pair_offset is not None:
        dx, dy = dx + pair_offset[..., 0], dy + pair_offset[..., 1]
    con = conics[g]
    sigma = 0.5 * (con[:, 0][None] * dx * dx + con[:, 2][None] * dy * dy) + con[:, 1][None] * dx * dy
    op = opacity.reshape(-1)[g][None]
    alpha = torch.clamp(op * torch.exp(-torch.where(valid, sigma, torch.zeros_like(sigma))), max=alpha_clamp)
    fi = final_idx.long()[:, None]
    mask = valid & ((pos[None] <= fi) if include_final else (pos[None] < fi))
    a = torch.where(mask, alpha, torch.zeros_like(alpha))
    one_m = 1.0 - a
    Tin = torch.cumprod(torch.cat([torch.ones_like(one_m[:, :1]), one_m[:, :-1]], 1), 1)
    T_last = Tin[:, -1] * one_m[:, -1]
    rgb = (a * Tin) @ colors[g]
    if with_background:
        rgb = rgb + T_last[:, None] * background[None].to(dt)
    return rgb, 1.0 - T_last, T_last


def sh_colors(degree: int, viewdirs: torch.Tensor, coeffs: torch.Tensor) -> torch.Tensor:
    """spherical_harmonics forward in the dtype of `coeffs` (the basis of oracle/gsplat_ref.py, dirs re-normalised)."""
    from .gsplat_ref import _sh_basis
    b = _sh_basis(degree, viewdirs.to(coeffs.dtype), coeffs.dtype)
    return sum(b[k][:, None] * coeffs[:, k, :] for k in range(len(b)))
