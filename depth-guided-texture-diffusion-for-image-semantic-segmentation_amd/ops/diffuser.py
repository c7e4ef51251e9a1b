from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L

LAT, P = 24, 144
GRID, K, STEPS = 12, 7, 4
# domain of the run-time parameterised kernels (csrc/diffuser_cfg.hip)
MAX_GRID, MAX_K, MAX_STEPS, MAX_LAT = 64, 11, 64, 64


def uses_generic(grid: int, k: int, steps: int, latent: int) -> bool:
    """False exactly for the reference configuration (12, 7, 4, 24): that one runs the kernels specialised for it
    (csrc/diffuser.hip); every other point runs the run-time parameterised family (csrc/diffuser_cfg.hip)."""
    return (grid, k, steps, latent) != (GRID, K, STEPS, LAT)


def resolve_steps(max_step: int, grid: int) -> int:
    """MessagePassing's rule (cod.py:1203): a negative ``max_step`` means max(h, w) = ``grid`` steps."""
    return grid if max_step < 0 else max_step


def _check_state(x_hp, depth, rw, rb, ew, eb, grid, k, steps):
    lat = ew.numel()
    if not (2 <= grid <= MAX_GRID and 3 <= k <= MAX_K and k % 2 == 1 and 0 <= steps <= MAX_STEPS and 1 <= lat <= MAX_LAT):
        raise L.DgtdError(f"diffuser_state: outside the domain 2 <= grid <= {MAX_GRID}, odd 3 <= k <= {MAX_K}, 0 <= steps <= {MAX_STEPS}, "
                          f"1 <= latent <= {MAX_LAT}: grid={grid} k={k} steps={steps} latent={lat}")
    if x_hp.dim() != 4 or x_hp.shape[1] != 3 or x_hp.shape[2] != x_hp.shape[3] or x_hp.shape[0] < 1 or x_hp.shape[2] % 4 or x_hp.shape[2] < 4:
        raise L.DgtdError(f"diffuser_state: x_hp must be [B,3,S,S] with S a positive multiple of 4, got {tuple(x_hp.shape)}")
    if tuple(depth.shape) != (x_hp.shape[0], 1, x_hp.shape[2], x_hp.shape[3]):
        raise L.DgtdError(f"diffuser_state: depth must be [B,1,S,S] = {(x_hp.shape[0], 1, *x_hp.shape[2:])}, got {tuple(depth.shape)}")
    if tuple(rw.shape) != (lat * k * k, 3) or rb.numel() != lat * k * k or eb.numel() != lat:
        raise L.DgtdError(f"diffuser_state: latent={lat}, k={k} need reg_w [{lat * k * k},3], reg_b [{lat * k * k}], enc_b [{lat}]; got "
                          f"reg_w {tuple(rw.shape)}, reg_b {tuple(rb.shape)}, enc_b {tuple(eb.shape)}")


def _workspace(nbytes: int, device) -> torch.Tensor:
    if nbytes < 0:
        raise L.DgtdError("diffuser: workspace query outside the kernels' domain")
    return torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=device)


class _DiffuserFn(Function):
    """x_hp [B,3,S,S], depth [B,1,S,S] + the regressor / depth-embedding parameters -> propagated state
    x4 [B,LAT,G,G] (twig/model/cod.py:1295-1298 + MessagePassing steps cod.py:1193-1205)."""

    @staticmethod
    def forward(ctx, x_hp, depth, reg_w, reg_b, enc_w, enc_b, grid, k, steps, generic):
        x_hp, depth = x_hp.float().contiguous(), depth.float().contiguous()
        rw, rb = reg_w.float().reshape(-1, 3).contiguous(), reg_b.float().contiguous()
        ew, eb = enc_w.float().reshape(-1).contiguous(), enc_b.float().contiguous()
        L.check_cuda(x_hp, depth, rw, rb, ew, eb)
        _check_state(x_hp, depth, rw, rb, ew, eb, grid, k, steps)
        B, _, S, _ = x_hp.shape
        lat = ew.numel()
        generic = generic or uses_generic(grid, k, steps, lat)
        x4 = torch.empty(B, lat, grid, grid, dtype=torch.float32, device=x_hp.device)
        if generic:
            ws = _workspace(L.load().dgtd_diffuser_cfg_workspace(B, S, grid, k, steps, lat, 0), x_hp.device)
            L.call("dgtd_diffuser_cfg_fwd", L.ptr(x_hp), L.ptr(depth), L.ptr(rw), L.ptr(rb), L.ptr(ew), L.ptr(eb), L.ptr(x4), L.ptr(ws),
                   B, S, grid, k, steps, lat, L.stream_ptr())
        else:
            L.call("dgtd_diffuser_fwd", L.ptr(x_hp), L.ptr(depth), L.ptr(rw), L.ptr(rb), L.ptr(ew), L.ptr(eb), L.ptr(x4), B, S, L.stream_ptr())
        ctx.save_for_backward(x_hp, depth, rw, rb, ew, eb)
        ctx.shapes = (reg_w.shape, enc_w.shape)
        ctx.cfg = (grid, k, steps, lat, generic)
        return x4

    @staticmethod
    @once_differentiable
    def backward(ctx, g4):
        x_hp, depth, rw, rb, ew, eb = ctx.saved_tensors
        grid, k, steps, lat, generic = ctx.cfg
        B, _, S, _ = x_hp.shape
        g4 = g4.float().contiguous()
        d_rw, d_rb, d_ew, d_eb = (torch.zeros_like(t) for t in (rw, rb, ew, eb))
        if generic:
            ws = _workspace(L.load().dgtd_diffuser_cfg_workspace(B, S, grid, k, steps, lat, 1), x_hp.device)
            L.call("dgtd_diffuser_cfg_bwd", L.ptr(x_hp), L.ptr(depth), L.ptr(rw), L.ptr(rb), L.ptr(ew), L.ptr(eb), L.ptr(g4),
                   L.ptr(d_rw), L.ptr(d_rb), L.ptr(d_ew), L.ptr(d_eb), L.ptr(ws), B, S, grid, k, steps, lat, L.stream_ptr())
        else:
            L.call("dgtd_diffuser_bwd", L.ptr(x_hp), L.ptr(depth), L.ptr(rw), L.ptr(rb), L.ptr(ew), L.ptr(eb), L.ptr(g4),
                   L.ptr(d_rw), L.ptr(d_rb), L.ptr(d_ew), L.ptr(d_eb), B, S, L.stream_ptr())
        return None, None, d_rw.view(ctx.shapes[0]), d_rb, d_ew.view(ctx.shapes[1]), d_eb, None, None, None, None


class _DiffuseTailFn(Function):
    """fused = bilinear_{G->S}(conv1x1_{LAT->3}(x4)) + image (cod.py:1206-1207, :1302)."""

    @staticmethod
    def forward(ctx, x4, cw, cb, image, generic):
        x4, image = x4.float().contiguous(), image.float().contiguous()
        if x4.dim() != 4 or x4.shape[2] != x4.shape[3] or not (2 <= x4.shape[2] <= MAX_GRID and 1 <= x4.shape[1] <= MAX_LAT):
            raise L.DgtdError(f"diffuse_tail: x4 must be [B,LAT,G,G] with 2 <= G <= {MAX_GRID}, 1 <= LAT <= {MAX_LAT}, got {tuple(x4.shape)}")
        lat, grid = x4.shape[1], x4.shape[2]
        if cw.numel() != 3 * lat or cb.numel() != 3:
            raise L.DgtdError(f"diffuse_tail: LAT={lat} needs conv_w [3,{lat}] and conv_b [3], got {tuple(cw.shape)}, {tuple(cb.shape)}")
        if image.dim() != 4 or image.shape[0] != x4.shape[0] or image.shape[1] != 3 or image.shape[2] != image.shape[3] \
                or image.shape[2] % 4 or image.shape[2] < 4:
            raise L.DgtdError(f"diffuse_tail: image must be [{x4.shape[0]},3,S,S] with S a positive multiple of 4, got {tuple(image.shape)}")
        w, b = cw.float().reshape(3, lat).contiguous(), cb.float().contiguous()
        L.check_cuda(x4, image, w, b)
        B, _, S, _ = image.shape
        generic = generic or (grid, lat) != (GRID, LAT)
        out = torch.empty_like(image)
        if generic:
            L.call("dgtd_diffuse_tail_cfg_fwd", L.ptr(x4), L.ptr(w), L.ptr(b), L.ptr(image), L.ptr(out), B, S, grid, lat, L.stream_ptr())
        else:
            L.call("dgtd_diffuse_tail_fwd", L.ptr(x4), L.ptr(w), L.ptr(b), L.ptr(image), L.ptr(out), B, S, L.stream_ptr())
        ctx.save_for_backward(x4, w)
        ctx.meta = (B, S, cw.shape, grid, lat, generic)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x4, w = ctx.saved_tensors
        B, S, wshape, grid, lat, generic = ctx.meta
        gout = gout.float().contiguous()
        g4 = torch.empty_like(x4)
        d_w = torch.zeros_like(w)
        d_b = torch.zeros(3, dtype=torch.float32, device=x4.device)
        if generic:
            ws = _workspace(L.load().dgtd_diffuse_tail_cfg_bwd_workspace(B, grid), x4.device)
            L.call("dgtd_diffuse_tail_cfg_bwd", L.ptr(gout), L.ptr(x4), L.ptr(w), L.ptr(g4), L.ptr(d_w), L.ptr(d_b), L.ptr(ws), B, S, grid,
                   lat, L.stream_ptr())
        else:
            ws = torch.empty(L.load().dgtd_diffuse_tail_bwd_workspace(B), dtype=torch.uint8, device=x4.device)
            L.call("dgtd_diffuse_tail_bwd", L.ptr(gout), L.ptr(x4), L.ptr(w), L.ptr(g4), L.ptr(d_w), L.ptr(d_b), L.ptr(ws), B, S, L.stream_ptr())
        return g4, d_w.view(wshape), d_b, None, None


def diffuser_state(x_hp, depth, reg_w, reg_b, enc_w, enc_b, grid=GRID, k=K, steps=STEPS, _generic=False):
    """Propagated state x4 [B,LAT,grid,grid]; LAT is ``enc_w``'s size.  ``steps < 0`` means ``grid`` steps (cod.py:1203).
    ``_generic=True`` (tests) runs the run-time parameterised kernels at the reference configuration too."""
    grid, k = int(grid), int(k)
    return _DiffuserFn.apply(x_hp, depth, reg_w, reg_b, enc_w, enc_b, grid, k, resolve_steps(int(steps), grid), bool(_generic))


def diffuse_tail(x4, conv_w, conv_b, image, _generic=False):
    """bilinear_{G->S}(conv1x1_{LAT->3}(x4)) + image; G and LAT are ``x4``'s."""
    return _DiffuseTailFn.apply(x4, conv_w, conv_b, image, bool(_generic))
