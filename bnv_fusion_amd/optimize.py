"""Global optimisation of the fused feature volume against the depth frames -- the second level of
the reference's bi-level fusion (src/run_e2e.py:111-162, src/utils/render_utils.py:461-590,
src/datasets/fusion_inference_dataset.py:308-420).

``render_with_rays`` and ``calculate_loss`` keep the reference's signatures so a maintainer can swap
``from src.utils.render_utils import calculate_loss`` for this one.  They run on the fused ray kernels
(csrc/rays.hip: sampling, L1 target and loss) and ``SparseVolume.decode_pts``, whose backward into
``volume.features`` is ``bnv_decode_pts_backward``.  ``ray_split_step`` (one split) and ``ray_batch_step`` (all
splits of a step at once) are the optimiser's step on the same kernels without autograd.  The torch formulation of
render_utils.py is not part of the package: it is the tests' checker (camera_rays ... calculate_loss), pinned to the
reference's golden vectors.

Randomness: pass ``generator=`` (a CPU or device ``torch.Generator``) for reproducible draws; a CPU
generator reproduces the reference's CPU stream bit for bit (used by the parity tests).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _uniforms(n, n_fine, n_coarse, dev, generator, per=None):
    """The uniforms of the stratified draws of n rays -> ([1, n, n_fine], [1, n, n_coarse]) on ``dev``.  A CPU generator
    draws split by split (``per`` rays; default one split), a split's fine strata and then its coarse ones: the
    reference's stream, bit for bit.  Any other generator draws each tensor in one call."""
    if generator is None or generator.device.type != "cpu":
        return (torch.rand((1, n, n_fine), device=dev, generator=generator),
                torch.rand((1, n, n_coarse), device=dev, generator=generator))
    per = per or n
    uf, uc = [], []
    for lo in range(0, n, per):
        k = min(per, n - lo)
        uf.append(torch.rand(1, k, n_fine, generator=generator))
        uc.append(torch.rand(1, k, n_coarse, generator=generator))
    return torch.cat(uf, 1).to(dev), torch.cat(uc, 1).to(dev)


def _ray_samples(rays, u_f, u_c, n_fine, n_coarse, truncated_dist):
    """The sampling kernel on the rays of batch entry 0 (render_utils.py:461-549 up to the decode) -> (pts [n, S, 3],
    L1 target [n, S], sample weight [n, S] (valid sample x ray mask), ray mask [n]); S = n_fine + n_coarse."""
    uv = rays["uv"][0].float().contiguous()
    n, dev, S = int(uv.shape[0]), uv.device, n_fine + n_coarse
    T = rays["T_wc_host"] if rays.get("T_wc_host") is not None else rays["T_wc"].detach().cpu().numpy()
    K = rays["intr_host"] if rays.get("intr_host") is not None else rays["intr_mat"].detach().cpu().numpy()
    T = (C.c_float * 16)(*np.asarray(T, dtype=np.float32).reshape(-1)[:16].tolist())
    K = (C.c_float * 9)(*np.asarray(K, dtype=np.float32).reshape(-1)[:9].tolist())
    gt = rays["gt_pts"][0].float().contiguous()
    rm = rays["mask"][0].float().contiguous()
    nb = rays["neighbor_pts"][0].float().contiguous()
    nbm = rays["neighbor_masks"][0].float().contiguous()
    u_f, u_c = u_f.contiguous(), u_c.contiguous()
    pts = torch.empty((n, S, 3), dtype=torch.float32, device=dev)
    target = torch.empty((n, S), dtype=torch.float32, device=dev)
    weight = torch.empty((n, S), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().bnv_ray_samples(
        _lib.ptr(uv), _lib.ptr(gt), _lib.ptr(rm), _lib.ptr(nb), _lib.ptr(nbm), int(nb.shape[1]), T, K, _lib.ptr(u_f),
        _lib.ptr(u_c), n, n_fine, n_coarse, float(truncated_dist), _lib.ptr(pts), _lib.ptr(target), _lib.ptr(weight),
        _lib.stream_ptr()), "bnv_ray_samples")
    return pts, target, weight, rm


def _sample_split(volume, rays, truncated_units, truncated_dist, ray_max_dist, generator):
    """One split's samples on fresh uniforms, with count_optim of their corner voxels before any decode
    (render_utils.py:488-493) -> what ``_ray_samples`` returns."""
    n_fine, n_coarse = int(truncated_units * 2), int(ray_max_dist * 5)
    uv = rays["uv"]
    u_f, u_c = _uniforms(int(uv.shape[1]), n_fine, n_coarse, uv.device, generator)
    out = _ray_samples(rays, u_f, u_c, n_fine, n_coarse, truncated_dist)
    volume.count_optim_pts(out[0])
    return out


def _ray_loss(pred, target, weight, n_valid):
    """bnv_ray_loss on flat float32 tensors: -> (sum weight |pred - target| / n_valid [1], d loss / d pred)."""
    loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
    g = torch.empty_like(pred)
    _lib.check(_lib.load().bnv_ray_loss(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(n_valid),
                                        int(pred.numel()), 0, _lib.ptr(loss), _lib.ptr(g), _lib.stream_ptr()),
               "bnv_ray_loss")
    return loss, g


class _RayLoss(torch.autograd.Function):
    """The L1 ray loss (render_utils.py:508-549) as an autograd node: its forward yields d loss / d pred as well."""

    @staticmethod
    def forward(ctx, pred, target, weight, n_valid):
        loss, g = _ray_loss(pred.detach().reshape(-1).float().contiguous(), target, weight, n_valid)
        ctx.save_for_backward(g.view(pred.shape))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        return grad_out * g, None, None, None


def render_with_rays(volume, rays, nerf, sdf_delta, truncated_units, truncated_dist, ray_max_dist,
                     generator=None):
    """render_utils.py:461-505: sample every ray, bump the optimisation counter of the touched voxels and decode the SDF
    at the samples (differentiable w.r.t. ``volume.features``) -> {"cam_loc" [1, 3], "sdf_on_rays" [1, n, S],
    "pts_on_rays" [1, n, S, 3]} (the reference's "ray_dirs" is not returned)."""
    pts = _sample_split(volume, rays, truncated_units, truncated_dist, ray_max_dist, generator)[0][None]
    pred = volume.decode_pts(pts, nerf, sdf_delta=sdf_delta)[..., 0]
    return {"cam_loc": rays["T_wc"][:, :3, 3], "sdf_on_rays": pred, "pts_on_rays": pts}


def calculate_loss(volume, rays, nerf, truncated_units, truncated_dist, ray_max_dist, sdf_delta=None,
                   generator=None):
    """render_utils.py:551-590 -> {"depth_bce_loss": 0-dim tensor}; its backward reaches ``volume.features``."""
    pts, target, weight, mask = _sample_split(volume, rays, truncated_units, truncated_dist, ray_max_dist, generator)
    pred = volume.decode_pts(pts[None], nerf, sdf_delta=sdf_delta)
    n_valid = (mask.sum() + 1e-4).reshape(1)                          # render_utils.py:553
    return {"depth_bce_loss": _RayLoss.apply(pred, target, weight, n_valid)}


def key_frame_points(depth, intr_mat, T_wc, ray_max_dist, conf=None, conf_level=0):
    """The part of _sample_key_frame that depends on the frame alone: every pixel's world point (float64 arithmetic of
    geometry.py:150-171, rounded to float32 as the sampler's ``.float()`` does after its gather) and validity
    (common.py:110-113).  -> (pts [H * W, 3] f32, mask [H * W] f32, H, W, host copies of T_wc / intr_mat).
    ``conf`` [H, W] (an ARKit confidence map): the validity also requires ``conf >= conf_level``
    (fusion_inference_dataset.py:388-389); the points stay those of the range-masked depth."""
    dev = depth.device
    intr_mat, T_wc = torch.as_tensor(intr_mat), torch.as_tensor(T_wc)
    depth = depth.to(torch.float64)
    mask = (depth > 0) & (depth < ray_max_dist)                       # common.py:110-113
    depth = depth * mask
    if conf is not None:
        mask = mask & (torch.as_tensor(conf, device=dev).reshape(depth.shape).to(torch.int32) >= int(conf_level))
    elif int(conf_level) > 0:
        raise _lib.BnvError("key_frame_points: conf_level > 0 needs a confidence map")
    H, W = depth.shape
    K = intr_mat.to(dev, torch.float32)
    T = T_wc.to(dev, torch.float32).to(torch.float64)
    # geometry.py:163-168 forms the normalised pixel coordinates in float32 before the float64 product
    u = ((torch.arange(W, device=dev, dtype=torch.float32) - K[0, 2]) / K[0, 0]).to(torch.float64)
    v = ((torch.arange(H, device=dev, dtype=torch.float32) - K[1, 2]) / K[1, 1]).to(torch.float64)
    pts_c = torch.stack([u[None, :].expand(H, W), v[:, None].expand(H, W), torch.ones_like(depth)], -1)
    pts_c = pts_c * depth[..., None]                                  # geometry.py:150-171
    pts_w = pts_c.reshape(-1, 3) @ T[:3, :3].T + T[:3, 3]
    r = torch.arange(-1, 2, device=dev)
    oy, ox = torch.meshgrid(r, r, indexing="ij")                      # np.meshgrid(range_, range_) order: x fastest
    return {"pts": pts_w.float(), "mask": mask.reshape(-1).float(), "H": H, "W": W,
            "oy": oy.reshape(1, -1), "ox": ox.reshape(1, -1), "zero_rgb": {},
            "intr_mat": intr_mat.to(dev).float().reshape(1, 3, 3), "T_wc": T_wc.to(dev).float().reshape(1, 4, 4),
            "T_wc_host": T_wc.detach().cpu().numpy().astype(np.float32).reshape(4, 4),
            "intr_host": intr_mat.detach().cpu().numpy().astype(np.float32).reshape(3, 3)}


def random_subset(n, k, device, generator=None):
    """``torch.randperm(n)[:k]`` in distribution -- k indices out of n without replacement, in random order
    (fusion_inference_dataset.py:383) -- without permuting all n on the device: a full permutation of a 640x480 image is a
    sort of 307,200 keys (18 merge passes, 135 us per optimiser step) to pick 5,000 rays.  2 k indices are drawn WITH
    replacement and every repeat of an earlier draw is dropped, which is sequential sampling with rejection -- the same
    distribution; the first k survivors are kept, in draw order.  With k <= n / 8 the expected number of repeats among the
    2 k draws is <= k / 4 and fewer than k survivors would need more than k of them (never seen; such a slot would hold
    index 0).  Larger k: the permutation."""
    if k * 8 > n:
        return torch.randperm(n, device=device, generator=generator)[:k]
    m = 2 * k
    draws = torch.randint(n, (m,), device=device, generator=generator)
    s, order = torch.sort(draws, stable=True)                  # equal values stay in draw order
    rep_sorted = torch.zeros(m, dtype=torch.bool, device=device)
    rep_sorted[1:] = s[1:] == s[:-1]                           # a later draw of a value already drawn
    rep = torch.empty_like(rep_sorted)
    rep[order] = rep_sorted
    pos = torch.cumsum(~rep, 0) - 1                            # rank among the survivors, in draw order
    out = torch.zeros(k + 1, dtype=draws.dtype, device=device)
    out.scatter_(0, torch.where(~rep & (pos < k), pos, torch.full_like(pos, k)), draws)     # (slot k: the rest)
    return out[:k]


def sample_key_frame(depth, intr_mat, T_wc, sampling_size, ray_max_dist, generator=None, points=None):
    """IterableInferenceDataset._sample_key_frame (fusion_inference_dataset.py:373-420) for a depth map
    already on the device: ``sampling_size`` random pixels with their back-projected world points, validity
    and 3x3 neighbourhoods.  depth [H, W] metres; intr_mat [3, 3]; T_wc [4, 4] -> rays dict (batch 1).
    ``points``: the frame's ``key_frame_points`` when the caller keeps them (NeuralMap.optimize does, per key frame:
    the reference re-reads the depth image in DataLoader workers beside the optimiser, off its critical path);
    depth, intr_mat and T_wc are not read then."""
    if points is None:
        points = key_frame_points(depth, intr_mat, T_wc, ray_max_dist)
    dev = points["pts"].device
    H, W = points["H"], points["W"]
    if generator is not None and generator.device.type == "cpu":
        idx = torch.randperm(H * W, generator=generator)[:sampling_size].to(dev)
    else:
        idx = random_subset(H * W, sampling_size, dev, generator)
    px, py = idx % W, idx // W
    nidx = (py[:, None] + points["oy"]).clamp(0, H - 1) * W + (px[:, None] + points["ox"]).clamp(0, W - 1)
    rgb = points["zero_rgb"].get(len(idx))        # (all zeros, read-only downstream: one tensor per batch size)
    if rgb is None:
        rgb = points["zero_rgb"][len(idx)] = torch.zeros(1, len(idx), 3, device=dev)
    return {"uv": torch.stack([px, py], -1).float().unsqueeze(0),
            "rgb": rgb,
            "gt_pts": points["pts"][idx].unsqueeze(0),
            "intr_mat": points["intr_mat"], "T_wc": points["T_wc"],
            "T_wc_host": points["T_wc_host"], "intr_host": points["intr_host"],
            "mask": points["mask"][idx].unsqueeze(0),
            "neighbor_pts": points["pts"][nidx].unsqueeze(0),
            "neighbor_masks": points["mask"][nidx].unsqueeze(0)}


def ray_split_step(volume, rays, nerf, truncated_units, truncated_dist, ray_max_dist, sdf_delta=None,
                   generator=None, grad=None, return_pred=False):
    """calculate_loss + backward of one ray split without autograd: sampling, count_optim, decode_pts forward,
    bnv_ray_loss and decode_pts backward, 6 launches, the uniforms drawn as calculate_loss draws them.  ``d loss / d
    features`` is ACCUMULATED into ``grad`` ([M, 8], e.g. ``volume.features.grad``); returns (loss [1] device tensor,
    pts [n, S, 3][, pred [n, S]])."""
    pts, target, weight, mask = _sample_split(volume, rays, truncated_units, truncated_dist, ray_max_dist, generator)
    pred = volume._decode_pts_forward(pts, nerf, sdf_delta, False, True).reshape(-1).contiguous()
    loss, g = _ray_loss(pred, target, weight, (mask.sum() + 1e-4).reshape(1))
    if grad is not None:
        volume.decode_pts_backward(pts, nerf, g, grad)
    return (loss, pts, pred.view(pts.shape[:2])) if return_pred else (loss, pts)


def ray_batch_step(volume, rays, nerf, truncated_units, truncated_dist, ray_max_dist, sdf_delta=None,
                   generator=None, grad=None, train_ray_splits=1000, return_pred=False):
    """ALL ray splits of one optimiser step at once (include/bnv_fusion.h: bnv_optim_step) -- what
    ``for lo in range(0, n_rays, train_ray_splits): ray_split_step(...)`` computes (run_e2e.py:127-153), in 5 launches
    instead of 6 per split: one sampling launch for every ray, count_optim of all splits recorded as per-row split masks,
    ONE forward + loss + backward kernel whose mask decisions see exactly the weights the split-by-split sequence would
    (weights[row] + 1 per split up to the query's own that touches the row), then the +1s applied.  The uniforms are drawn
    split by split in the reference's order when the generator is a CPU generator (bit-for-bit the reference's stream);
    with a device generator (or none) in two calls for the whole step.  ``d loss / d features`` of the SUM of the splits'
    losses is ACCUMULATED into ``grad``; returns (sum of the splits' losses [1], pts [n, S, 3][, pred [n, S]]).  If
    anything fails once the splits are counted, the split masks are cleared and the weights left as they were."""
    n = int(rays["uv"].shape[1])
    n_fine, n_coarse = int(truncated_units * 2), int(ray_max_dist * 5)
    S = n_fine + n_coarse
    per = int(train_ray_splits)
    n_splits = -(-n // per)
    if n_splits > 31:
        raise ValueError(f"{n_splits} ray splits in one step (at most 31: raise train_ray_splits)")
    u_f, u_c = _uniforms(n, n_fine, n_coarse, rays["uv"].device, generator, per)
    pts, target, weight, rm = _ray_samples(rays, u_f, u_c, n_fine, n_coarse, truncated_dist)
    dev = pts.device
    # per split: sum of its ray masks + 1e-4 (render_utils.py:553)
    if n % per == 0:
        n_valid = rm.view(n_splits, per).sum(1) + 1e-4
    else:
        n_valid = torch.stack([rm[lo: lo + per].sum() for lo in range(0, n, per)]) + 1e-4
    n_valid = n_valid.float().contiguous()
    split_samples = per * S
    try:
        volume.count_optim_splits(pts, split_samples)
        loss2 = torch.zeros(2, dtype=torch.float32, device=dev)
        pred = torch.empty((n, S), dtype=torch.float32, device=dev) if return_pred else None
        if grad is None:
            grad = torch.zeros_like(volume.features.detach())        # (the kernel needs somewhere to accumulate)
        if _lib.model_mode(nerf) == 2 or not hasattr(nerf, "sdf_bwd_pack"):
            # tiny-cuda-nn decoder: its own forward / backward kernels, all splits per launch
            p = volume.decode_pts_splits(pts, nerf, sdf_delta, split_samples)
            g = torch.empty_like(p)
            _lib.check(_lib.load().bnv_ray_loss(
                _lib.ptr(p), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(n_valid), n * S, split_samples,
                _lib.ptr(loss2), _lib.ptr(g), _lib.stream_ptr()), "bnv_ray_loss")
            volume.decode_pts_backward_splits(pts, nerf, g, grad, split_samples)
            if pred is not None:
                pred.copy_(p.view(n, S))
        else:
            volume.optim_step(pts, nerf, sdf_delta, split_samples, target, weight, n_valid, loss2, grad, pred)
        volume.apply_split_counts()
    except BaseException:
        volume._split_mask().zero_()          # no stale +1s for the next step's apply_split_counts
        raise
    out = (loss2[:1], pts)
    return out + (pred,) if return_pred else out


def optimize_volume(volume, nerf, ray_batches, truncated_units, truncated_dist, ray_max_dist, sdf_delta=None,
                    train_ray_splits=1000, lr=0.001, generator=None, batched=True):
    """NeuralMap.optimize (run_e2e.py:111-162): Adam on ``volume.features`` over an iterable of ray
    batches, ``train_ray_splits`` rays per backward, then the optimised features are written back into the
    hash volume.  Returns the list of per-iteration losses (device scalars).  ``batched``: all splits of a step per
    launch (ray_batch_step) instead of split by split (ray_split_step) -- same decisions, same weights, gradients equal
    up to the order of float atomics."""
    volume.to_tensor()
    volume.features = torch.nn.Parameter(volume.features)
    # (one fused update kernel on the device instead of the foreach implementation's eight: the same formula)
    optimizer = torch.optim.Adam([volume.features], lr=lr, **({"fused": True} if volume.features.is_cuda else {}))
    history = []
    whole = ("T_wc", "intr_mat", "T_wc_host", "intr_host")
    for rays in ray_batches:
        optimizer.zero_grad(set_to_none=False)
        if rays.get("T_wc_host") is not None:
            if np.isnan(rays["T_wc_host"]).any():
                continue
        elif torch.isnan(rays["T_wc"]).any():
            continue
        if volume.features.grad is None:
            volume.features.grad = torch.zeros_like(volume.features)
        n_rays = rays["uv"].shape[1]
        if batched and -(-n_rays // train_ray_splits) <= 31:
            # every split of the step in one set of launches (same mask decisions, same count_optim as split by split)
            total = ray_batch_step(volume, rays, nerf, truncated_units, truncated_dist, ray_max_dist,
                                   sdf_delta=sdf_delta, generator=generator, grad=volume.features.grad,
                                   train_ray_splits=train_ray_splits)[0][0]
        else:
            total = None
            for lo in range(0, n_rays, train_ray_splits):
                part = {k: (v[:, lo: lo + train_ray_splits] if k not in whole else v) for k, v in rays.items()}
                loss = ray_split_step(volume, part, nerf, truncated_units, truncated_dist, ray_max_dist,
                                      sdf_delta=sdf_delta, generator=generator, grad=volume.features.grad)[0][0]
                total = loss if total is None else total + loss
        optimizer.step()
        history.append(total)
    feats = volume.features.detach()
    volume.features = feats
    volume.insert(volume.active_coordinates, feats, volume.weights, volume.num_hits)
    return history
