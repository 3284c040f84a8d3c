"""Float32 torch restatement of the render semantics of include/bnv_fusion.h ("Rendering"): camera rays, the sample
box and schedule, the domain rules, the hit rule and its interpolation.  Every step is one float32 torch operation on
the CPU (IEEE, one rounding each, no contraction), in the order the header writes, so sample positions and depths can
be compared with the kernels bit for bit.  The field is the caller's: an analytic function, the HIP volume's own
``decode_pts`` or the checker's."""
import numpy as np
import torch

F32 = torch.float32
NORMAL_EPS = 0.5          # BNV_RENDER_NORMAL_EPS


def f32(x):
    return torch.tensor(float(np.float32(x)), dtype=F32)


def sqrt32(x):
    """Correctly rounded float32 sqrt (torch's CPU kernel is not): the float64 root rounded once to float32."""
    return torch.sqrt(x.double()).float()


def box(lo, n, voxel):
    """Sample box of a grid with origin ``lo`` [3], ``n`` [3] points per axis: (lo, lo + (n - 1) * voxel)."""
    lo = torch.as_tensor(np.asarray(lo, dtype=np.float32), dtype=F32).reshape(3)
    v = f32(voxel)
    hi = torch.stack([lo[a] + f32(int(n[a]) - 1) * v for a in range(3)])
    return lo, hi


def ray_setup(T_wc, K, H, W, lo, hi, near, max_depth):
    T = torch.from_numpy(np.asarray(T_wc, dtype=np.float64).astype(np.float32))
    Km = torch.from_numpy(np.asarray(K, dtype=np.float64).astype(np.float32))
    u = torch.arange(W, dtype=F32)[None, :].expand(H, W).reshape(-1)
    v = torch.arange(H, dtype=F32)[:, None].expand(H, W).reshape(-1)
    x = (u - Km[0, 2]) / Km[0, 0]
    y = (v - Km[1, 2]) / Km[1, 1]
    w = [(T[a, 0] * x + T[a, 1] * y) + T[a, 2] for a in range(3)]
    nrm = sqrt32((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    d = [w[a] / nrm for a in range(3)]
    o = T[:3, 3].clone()
    n = H * W
    tin = torch.zeros(n, dtype=F32)
    tout = torch.full((n,), float("inf"), dtype=F32)
    miss = torch.zeros(n, dtype=torch.bool)
    for a in range(3):
        zero = d[a] == 0
        safe = torch.where(zero, torch.ones_like(d[a]), d[a])
        t1 = (lo[a] - o[a]) / safe
        t2 = (hi[a] - o[a]) / safe
        tin = torch.where(zero, tin, torch.maximum(tin, torch.minimum(t1, t2)))
        tout = torch.where(zero, tout, torch.minimum(tout, torch.maximum(t1, t2)))
        if bool(((o[a] < lo[a]) | (o[a] > hi[a]))):
            miss |= zero
    t0 = torch.maximum(tin, f32(near) * nrm)
    t1 = torch.minimum(tout, f32(max_depth) * nrm)
    t1 = torch.where(miss, torch.full_like(t1, -1.0), t1)
    return {"o": o, "d": torch.stack(d, 1), "nrm": nrm, "t0": t0, "t1": t1}


def schedule(ray, step_world):
    """t [R, S] of samples k = 0..S-1 and their validity (t_k <= t1)."""
    s = f32(step_world) if not isinstance(step_world, torch.Tensor) else step_world
    span = (ray["t1"] - ray["t0"]).clamp(min=0)
    n_max = int(torch.floor(span.max() / s).item()) + 3 if span.numel() else 1
    k = torch.arange(n_max, dtype=F32)
    t = ray["t0"][:, None] + k[None, :] * s
    return t, t <= ray["t1"][:, None]


def positions(ray, t):
    return torch.stack([ray["o"][a] + t * ray["d"][:, a][:, None] for a in range(3)], -1)


def lead_ins(valid, dom):
    """Samples right before a run of in-domain samples that are not in the domain themselves."""
    lead = torch.zeros_like(dom)
    lead[:, :-1] = valid[:, :-1] & ~dom[:, :-1] & dom[:, 1:]
    return lead


def first_hit(ray, t, dom, f, step_world, evaluated=None):
    """Hit rule + interpolation -> (depth [R], t_hit [R], hit [R]).  ``evaluated``: samples with a value (the
    in-domain ones and the runs' lead-ins; default: the in-domain ones)."""
    s = f32(step_world) if not isinstance(step_world, torch.Tensor) else step_world
    ev = dom if evaluated is None else evaluated
    f = torch.where(ev, f, torch.zeros_like(f))
    cross = ev[:, :-1] & dom[:, 1:] & (f[:, :-1] > 0) & (f[:, 1:] <= 0)
    hit = cross.any(1)
    k1 = torch.argmax(cross.to(torch.int8), 1)          # first crossing: index of sample k - 1
    rows = torch.arange(t.shape[0])
    f0, f1 = f[rows, k1], f[rows, k1 + 1]
    k_prev = k1.to(F32)
    t_prev = ray["t0"] + k_prev * s
    den = torch.where(hit, f0 - f1, torch.ones_like(f0))
    th = t_prev + (f0 / den) * s
    depth = torch.where(hit, th / ray["nrm"], torch.zeros_like(th))
    return depth, torch.where(hit, th, torch.full_like(th, -1.0)), hit


def render(ray, step_world, field, domain, masked=None, lead_in=True):
    """field(p [N, 3]) -> f32 [N], called on the in-domain samples and on each run's lead-in (the out-of-domain sample
    right before it; ``masked(p)`` gives those instead when set -- the HIP volume's decode_pts returns its masked
    constant there by itself); domain(p [N, 3]) -> bool [N].  ``lead_in=False``: the TSDF rule, in-domain samples
    only."""
    t, valid = schedule(ray, step_world)
    p = positions(ray, t)
    dom = valid.clone()
    dom[valid] = domain(p[valid])
    lead = lead_ins(valid, dom) if lead_in else torch.zeros_like(dom)
    ev = dom | lead
    f = torch.zeros_like(t)
    if masked is None:
        if bool(ev.any()):
            f[ev] = field(p[ev]).to(F32)
    else:
        if bool(dom.any()):
            f[dom] = field(p[dom]).to(F32)
        if bool(lead.any()):
            f[lead] = masked(p[lead]).to(F32)
    return first_hit(ray, t, dom, f, step_world, ev)


def hit_points(ray, t_hit):
    return ray["o"][None, :] + t_hit[:, None] * ray["d"]


def normalise(g):
    l = sqrt32((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    safe = torch.where(l > 0, l, torch.ones_like(l))
    return torch.where((l > 0)[:, None], g / safe[:, None], torch.zeros_like(g))


def central_difference_normals(ray, t_hit, hit, field, voxel):
    """Neural normals: g_a = f(p + e e_a) - f(p - e e_a), e = NORMAL_EPS * voxel, normalised; 0 without a hit."""
    p = hit_points(ray, t_hit)[hit]
    e = f32(NORMAL_EPS) * f32(voxel)
    pts = []
    for a in range(3):
        for sgn in (0, 1):
            q = p.clone()
            q[:, a] = p[:, a] - e if sgn else p[:, a] + e
            pts.append(q)
    vals = field(torch.stack(pts, 1).reshape(-1, 3)).to(F32).reshape(-1, 6)
    g = torch.stack([vals[:, 2 * a] - vals[:, 2 * a + 1] for a in range(3)], 1)
    out = torch.zeros((hit.shape[0], 3), dtype=F32)
    out[hit] = normalise(g)
    return out


# ---- neural volume domain -------------------------------------------------------------------------------------------

def occupancy(coords, n_xyz):
    """Dense bool grid of the volume's rows from its voxel coordinates [M, 3]."""
    occ = torch.zeros(tuple(int(v) for v in n_xyz), dtype=torch.bool)
    c = torch.as_tensor(coords).cpu().long()
    if c.numel():
        occ[c[:, 0], c[:, 1], c[:, 2]] = True
    return occ


def neural_domain(occ, bound_min, voxel):
    bmin = torch.as_tensor(np.asarray(bound_min, dtype=np.float32), dtype=F32).reshape(3)
    v = f32(voxel)
    dims = torch.tensor(occ.shape)

    def dom(p):
        c = (p - bmin[None, :]) / v
        fl, ce = torch.floor(c), torch.ceil(c)
        ok = torch.ones(p.shape[0], dtype=torch.bool)
        for b in range(8):
            idx = torch.stack([(ce if (b >> a) & 1 else fl)[:, a] for a in range(3)], 1).long()
            inside = ((idx >= 0) & (idx < dims[None, :])).all(1)
            cl = torch.minimum(idx.clamp(min=0), dims[None, :] - 1)
            ok &= inside & occ[cl[:, 0], cl[:, 1], cl[:, 2]]
        return ok
    return dom


# ---- TSDF volume ------------------------------------------------------------------------------------------------

def _lerp(a, b, f):
    return a + f * (b - a)


def _tsdf_cell(tsdf, origin, voxel, p, clamp):
    org = torch.as_tensor(np.asarray(origin, dtype=np.float32), dtype=F32).reshape(3)
    dims = torch.tensor(tsdf.shape)
    c = (p - org[None, :]) / f32(voxel)
    fl = torch.floor(c)
    if clamp:
        fl = torch.minimum(torch.clamp(fl, min=0.0), (dims - 2).to(F32)[None, :])
    inside = ((fl >= 0) & (fl < (dims - 1).to(F32)[None, :])).all(1)
    i = torch.where(inside[:, None], fl, torch.zeros_like(fl)).long()
    fr = c - fl
    corners = [(i[:, 0] + (b & 1), i[:, 1] + ((b >> 1) & 1), i[:, 2] + ((b >> 2) & 1)) for b in range(8)]
    return inside, fr, corners


def tsdf_field(tsdf, weight, origin, voxel):
    """(domain(p), field(p)) of the trilinear TSDF on CPU float32 grids [X, Y, Z]."""
    def dom(p):
        inside, _, corners = _tsdf_cell(tsdf, origin, voxel, p, False)
        ok = inside.clone()
        for c in corners:
            ok &= weight[c] > 0
        return ok

    def field(p):
        _, f, corners = _tsdf_cell(tsdf, origin, voxel, p, False)
        v = [tsdf[c] for c in corners]
        y0 = _lerp(_lerp(v[0], v[1], f[:, 0]), _lerp(v[2], v[3], f[:, 0]), f[:, 1])
        y1 = _lerp(_lerp(v[4], v[5], f[:, 0]), _lerp(v[6], v[7], f[:, 0]), f[:, 1])
        return _lerp(y0, y1, f[:, 2])
    return dom, field


def tsdf_normals(tsdf, origin, voxel, p):
    _, f, corners = _tsdf_cell(tsdf, origin, voxel, p, True)
    v = [tsdf[c] for c in corners]
    gx = _lerp(_lerp(v[1] - v[0], v[3] - v[2], f[:, 1]), _lerp(v[5] - v[4], v[7] - v[6], f[:, 1]), f[:, 2])
    gy = _lerp(_lerp(v[2] - v[0], v[3] - v[1], f[:, 0]), _lerp(v[6] - v[4], v[7] - v[5], f[:, 0]), f[:, 2])
    gz = _lerp(_lerp(v[4] - v[0], v[5] - v[1], f[:, 0]), _lerp(v[6] - v[2], v[7] - v[3], f[:, 0]), f[:, 1])
    return normalise(torch.stack([gx, gy, gz], 1))
