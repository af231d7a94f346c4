"""Shared by tests/test_penetration_ref.py (CPU) and tests/test_penetration_gpu.py (MI355X): the multi-person penetration term of DESIGN.md 18
RESTATED in torch (float64 = the reference, float32 = the rounding floor), the generated meshes and cases, the mutations of the restatement,
the screening of the piecewise-constant gradient and the recorded floors the tolerances come from.

There is no oracle for this term: the reference's SDFLoss lives in a third-party package that is neither part of it nor installed.  The
restatement follows the definition and is deliberately NOT the kernels' arithmetic: the distance is Ericson's closest point with its seven
regions (the kernels take the minimum over edges and the plane), the solid angle uses torch.atan2 (the kernels a polynomial), and the sampling
is F.grid_sample itself with autograd (the kernels differentiate by hand)."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

OUTPUTS = ('phi', 'boxes', 'overlap', 'loss', 'g_verts')
MULTIPLE = 16                     # bounds = 16 x the fp32 floor, the project's multiple
SCREEN = 1e-4                     # grid units: a sampled vertex this close to a cell boundary is left out of the gradient comparison
SCREEN_CAP = 0.02                 # of the sampled vertices of a case


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------------
def icosphere(level):
    """Unit icosahedron subdivided `level` times, outward orientation: level 1 = 42 vertices / 80 faces, level 2 = 162 / 320."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


def is_closed_and_oriented(faces):
    """Every directed edge appears once and its reverse once."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    fwd = e[:, 0] * (faces.max() + 1) + e[:, 1]
    rev = e[:, 1] * (faces.max() + 1) + e[:, 0]
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(rev))


def signed_volume(verts, faces):
    a, b, c = (np.asarray(verts, np.float64)[faces[:, k]] for k in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


def _body(rng, unit, radius, aniso, centre, perturb=0.2):
    """A radially perturbed (x (1 + perturb . randn)), anisotropically scaled copy of the unit mesh."""
    r = 1.0 + perturb * np.clip(rng.standard_normal(len(unit)), -2.5, 2.5)
    return (unit * r[:, None] * radius * np.asarray(aniso) + np.asarray(centre)).astype(np.float32)


def _two_lobes(rng, unit, faces, radius, centre, gap):
    """One mesh of two lobes pushed through each other (the region inside both has winding number 2)."""
    a = _body(rng, unit, radius, (1.0, 0.9, 1.1), np.asarray(centre) - np.asarray([gap, 0, 0]), 0.1)
    b = _body(rng, unit, radius, (1.1, 1.0, 0.9), np.asarray(centre) + np.asarray([gap, 0, 0]), 0.1)
    return np.concatenate([a, b])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(verts (F, P, V, 3) fp32 as the kernel gets them (NaN for inactive persons), verts_full (the same with finite values
    everywhere, what the `exist` mutation reads), active (F, P) uint8, faces (NF, 3) int32, G, scale_factor, rho)."""
    u1, f1 = icosphere(1)
    u2, f2 = icosphere(2)
    out = {}

    def add(name, bodies, active, faces, G, seed, scale_factor=0.2, rho=1.0):
        full = np.asarray(bodies, np.float32)
        active = np.asarray(active, np.uint8)
        verts = full.copy()
        verts[active == 0] = np.nan
        out[name] = dict(verts=verts, verts_full=full, active=active, faces=np.ascontiguousarray(faces, np.int32), G=G, scale_factor=scale_factor,
                         rho=rho, seed=seed)

    rng = np.random.default_rng(11)
    two = [[_body(rng, u1, 0.5, (1.0, 0.8, 1.3), (0, 0, 0)), _body(rng, u1, 0.45, (1.2, 1.0, 0.7), (0.45, 0.1, -0.2))],
           [_body(rng, u1, 0.5, (0.9, 1.1, 1.0), (0.1, 0, 0)), _body(rng, u1, 0.6, (1.0, 0.7, 1.0), (-0.3, 0.35, 0.3))]]
    add('two_overlap', two, [[1, 1], [1, 1]], f1, 8, 11)
    add('two_overlap_linear', two, [[1, 1], [1, 1]], f1, 8, 11, rho=0.0)

    rng = np.random.default_rng(12)
    three = [[_body(rng, u1, 0.5, (1.0, 0.8, 1.3), (0, 0, 0)), _body(rng, u1, 0.45, (1.2, 1.0, 0.7), (0.5, 0.1, -0.2)), _body(rng, u1, 0.5, (1, 1, 1), (5.0, 4.0, 0))],
             [_body(rng, u1, 0.5, (1.0, 1.0, 1.2), (0, 0, 0)), _body(rng, u1, 0.5, (1.1, 1.0, 0.8), (0.5, 0.2, 0)), _body(rng, u1, 0.5, (0.8, 1.2, 1), (0.2, -0.4, 0.3))]]
    add('third_isolated', three, [[1, 1, 1], [1, 1, 1]], f1, 8, 12)

    rng = np.random.default_rng(13)
    a = _body(rng, u1, 0.5, (1.0, 0.9, 1.1), (0, 0, 0))
    b0 = _body(rng, u1, 0.5, (1.1, 1.0, 0.9), (0, 0.1, 0.1))
    hi = a[:, 0].max()

    def shifted(delta):
        b = b0.copy()
        b[:, 0] = (b0[:, 0] - b0[:, 0].min()) + np.float32(hi)          # the smallest x is exactly the other box's largest
        if delta:
            b[:, 0] = b[:, 0] + np.float32(delta)
        return b
    add('touch', [[a, shifted(1e-3)], [a, shifted(-1e-3)], [a, shifted(0.0)], [a, shifted(-0.4)]], [[1, 1]] * 4, f1, 8, 13)

    rng = np.random.default_rng(14)
    g = [[_body(rng, u1, 0.5, (1, 1, 1), (0, 0, 0)), _body(rng, u1, 0.5, (1, 1, 1), (0.4, 0, 0)), _body(rng, u1, 0.5, (1, 1, 1), (0.2, 0.3, 0))] for _ in range(3)]
    add('gates', g, [[0, 1, 0], [0, 0, 0], [1, 0, 1]], f1, 8, 14)

    rng = np.random.default_rng(15)
    pad = [[_body(rng, u1, 0.5, (1.0, 0.95, 1.05), (0, 0, 0), 0.03), _body(rng, u1, 0.75, (1.0, 1.1, 0.9), (0.55, 0.25, -0.1), 0.05)],
           [_body(rng, u1, 0.5, (1.05, 1.0, 0.95), (0, 0, 0), 0.03), _body(rng, u1, 0.8, (1.0, 1.0, 1.0), (-0.3, -0.6, 0.35), 0.05)]]
    add('padding', pad, [[1, 1], [1, 1]], f1, 8, 15, scale_factor=0.0)

    rng = np.random.default_rng(16)
    fl = np.concatenate([f1, f1 + len(u1)])
    lobes = [[_two_lobes(rng, u1, f1, 0.4, (0, 0, 0), 0.2), _two_lobes(rng, u1, f1, 0.4, (0.25, 0.3, 0.1), 0.25)]]
    add('lobes', lobes, [[1, 1]], fl, 8, 16)

    rng = np.random.default_rng(17)
    big = [[_body(rng, u2, 0.5, (1.0, 0.8, 1.3), (0, 0, 0), 0.1), _body(rng, u2, 0.45, (1.2, 1.0, 0.7), (0.4, 0.15, -0.2), 0.1)]]
    add('g32', big, [[1, 1]], f2, 32, 17)
    return out


CASE_NAMES = ('two_overlap', 'two_overlap_linear', 'third_isolated', 'touch', 'gates', 'padding', 'lobes', 'g32')


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def point_triangle_distance(p, a, b, c, planes_only=False):
    """p (M, 1, 3), a / b / c (1, NF, 3) -> (M, NF) distances to the triangles: Ericson's closest point over the seven regions (three corners,
    three edges, the interior)."""
    ab, ac, ap = b - a, c - a, p - a
    if planes_only:
        n = torch.cross(ab, ac, dim=-1)
        return _dot(ap, n).abs() / n.norm(dim=-1)
    bp, cp = p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4

    def safe(num, den):
        return num / torch.where(den == 0, torch.ones_like(den), den)
    den = va + vb + vc
    q = a + ab * safe(vb, den)[..., None] + ac * safe(vc, den)[..., None]                                                    # interior
    q = torch.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + (c - b) * safe(d4 - d3, (d4 - d3) + (d5 - d6))[..., None], q)      # edge bc
    q = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * safe(d2, d2 - d6)[..., None], q)                 # edge ac
    q = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c.expand_as(q), q)                                                    # corner c
    q = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * safe(d1, d1 - d3)[..., None], q)                 # edge ab
    q = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b.expand_as(q), q)                                                    # corner b
    q = torch.where(((d1 <= 0) & (d2 <= 0))[..., None], a.expand_as(q), q)                                                     # corner a
    return (p - q).norm(dim=-1)


def winding_number(p, a, b, c):
    """Generalised winding number (1 / 4 pi) sum of the Van Oosterom-Strackee solid angles -> (M,)."""
    A, B, C = a - p, b - p, c - p
    la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
    det = _dot(A, torch.cross(B, C, dim=-1))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    return (2.0 * torch.atan2(det, den)).sum(-1) / (4.0 * np.pi)


def sdf_grid(xn, faces, G, planes_only=False, chunk=2048):
    """phi[kz][ky][kx] of one mesh given in normalised coordinates (V, 3)."""
    k = -1.0 + (2.0 * torch.arange(G, dtype=xn.dtype) + 1.0) / G
    pts = torch.stack(torch.meshgrid(k, k, k, indexing='ij'), -1).reshape(-1, 3).flip(-1)          # [kz][ky][kx] -> (x, y, z)
    f = torch.as_tensor(faces, dtype=torch.long)
    a, b, c = xn[f[:, 0]][None], xn[f[:, 1]][None], xn[f[:, 2]][None]
    phi = []
    for s in range(0, len(pts), chunk):
        p = pts[s:s + chunk, None]
        d = point_triangle_distance(p, a, b, c, planes_only).min(-1).values
        phi.append(torch.where(winding_number(p, a, b, c) > 0.5, d, torch.zeros_like(d)))
    return torch.cat(phi).reshape(G, G, G)


MUTATIONS = ('align_corners', 'no_nf2', 'self_sample', 'open_overlap', 'no_scale_factor', 'grad_through_centre', 'swap_xz', 'plane_distance',
             'metres', 'exist')


def restate(case, dtype, mut=None):
    """The definition of DESIGN.md 18 in torch at `dtype` -> dict of numpy arrays: phi (F, P, G, G, G), boxes (F, P, 2, 3), overlap (F, P),
    loss (F,), g_verts (F, P, V, 3), and frac (F, P, V): the sampled vertices' smallest distance (grid units) to a cell boundary over axes
    and sources (inf where nothing is sampled).  `mut`: one of MUTATIONS."""
    assert mut is None or mut in MUTATIONS
    G, sf, rho = case['G'], case['scale_factor'], case['rho']
    src = case['verts_full'] if mut == 'exist' else case['verts']
    active = np.ones_like(case['active']) if mut == 'exist' else case['active']
    x = torch.tensor(src, dtype=dtype).requires_grad_(True)
    F_, P, V = x.shape[:3]
    phi_all, boxes = torch.zeros((F_, P, G, G, G), dtype=dtype), torch.zeros((F_, P, 2, 3), dtype=dtype)
    overlap, frac = np.zeros((F_, P), np.int32), np.full((F_, P, V), np.inf)
    losses = []
    for f in range(F_):
        act = [p for p in range(P) if active[f, p]]
        loss = torch.zeros((), dtype=dtype)
        for p in act:
            boxes[f, p, 0], boxes[f, p, 1] = x[f, p].detach().amin(0), x[f, p].detach().amax(0)
        if len(act) >= 2:
            def meets(p, q):
                lo_p, hi_p, lo_q, hi_q = boxes[f, p, 0], boxes[f, p, 1], boxes[f, q, 0], boxes[f, q, 1]
                return bool(((lo_p < hi_q) & (lo_q < hi_p)).all()) if mut == 'open_overlap' else bool(((lo_p <= hi_q) & (lo_q <= hi_p)).all())
            O = [p for p in act if any(meets(p, q) for q in act if q != p)]
            overlap[f, O] = 1
            n = len(O)
            for p in O:
                lo, hi = (x[f, p].amin(0), x[f, p].amax(0)) if mut == 'grad_through_centre' else (boxes[f, p, 0], boxes[f, p, 1])
                c = (lo + hi) / 2
                s = (1.0 if mut == 'no_scale_factor' else 1.0 + sf) * 0.5 * (boxes[f, p, 1] - boxes[f, p, 0]).max()
                with torch.no_grad():
                    phi = sdf_grid((x[f, p].detach() - c.detach()) / s, case['faces'], G, planes_only=(mut == 'plane_distance'))
                    if mut == 'metres':
                        phi = phi * s
                phi_all[f, p] = phi
                for q in O:
                    if q == p and mut != 'self_sample':
                        continue
                    u = (x[f, q] - c) / s
                    if mut == 'swap_xz':
                        u = u.flip(-1)
                    val = Fn.grid_sample(phi[None, None], u[None, None, None], mode='bilinear', padding_mode='zeros', align_corners=(mut == 'align_corners'))[0, 0, 0, 0]
                    loss = loss + (val * val / (val * val + rho * rho) if rho else val).sum()
                    fx = ((u.detach().double() + 1) * G - 1) / 2
                    d = (fx - fx.round()).abs().amin(-1)
                    inside = ((fx > -1) & (fx < G)).all(-1)
                    frac[f, q] = np.minimum(frac[f, q], torch.where(inside, d, torch.full_like(d, np.inf)).numpy())
            if n and mut != 'no_nf2':
                loss = loss / (n * n)
        losses.append(loss)
    total = torch.stack(losses)
    g = torch.autograd.grad(total.sum(), x)[0] if total.requires_grad else torch.zeros_like(x)
    g = torch.nan_to_num(g, nan=0.0) * torch.tensor(active, dtype=dtype)[..., None, None]           # (inactive persons: NaN inputs, zero gradient)
    return dict(phi=phi_all.numpy(), boxes=boxes.numpy(), overlap=overlap, loss=total.detach().numpy(), g_verts=g.numpy(), frac=frac)


def frame_term(x, faces, G=32, scale_factor=0.2, rho=1.0):
    """L_f of one frame for the stacked vertices x (N, V, 3) of its visible persons, differentiable with respect to x: the definition without
    the mutations, for the end-to-end reference (tests/penetration_e2e.py).  restate() on an all-active frame gives the same value."""
    N = x.shape[0]
    if N < 2:
        return x.new_zeros(())
    lo, hi = x.detach().amin(1), x.detach().amax(1)
    O = [p for p in range(N) if any(bool(((lo[p] <= hi[q]) & (lo[q] <= hi[p])).all()) for q in range(N) if q != p)]
    loss = x.new_zeros(())
    for p in O:
        c, s = (lo[p] + hi[p]) / 2, (1.0 + scale_factor) * 0.5 * (hi[p] - lo[p]).max()
        with torch.no_grad():
            phi = sdf_grid((x[p].detach() - c) / s, faces, G)
        for q in O:
            if q != p:
                val = Fn.grid_sample(phi[None, None], ((x[q] - c) / s)[None, None, None], mode='bilinear', padding_mode='zeros', align_corners=False)[0, 0, 0, 0]
                loss = loss + (val * val / (val * val + rho * rho) if rho else val).sum()
    return loss / (len(O) ** 2) if O else loss


@functools.lru_cache(maxsize=None)
def ref64(name):
    return restate(cases()[name], torch.float64)


@functools.lru_cache(maxsize=None)
def ref32(name):
    return restate(cases()[name], torch.float32)


def screen(name):
    """(F, P, V) bool: the vertices kept in the gradient comparison, and the screened share of the sampled ones (judged on the fp64 reference)."""
    frac = ref64(name)['frac']
    sampled = np.isfinite(frac)
    keep = ~(sampled & (frac < SCREEN))
    return keep, float((sampled & ~keep).sum()) / max(1, int(sampled.sum()))


def errors(name, got, ref=None):
    """Worst absolute error per output of `got` against the fp64 reference (phi over the whole grid, in normalised units; g_verts over the
    vertices that pass the screening)."""
    ref = ref64(name) if ref is None else ref
    keep = screen(name)[0]
    e = {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()) for k in ('phi', 'boxes', 'loss')}
    e['overlap'] = float(np.abs(np.asarray(got['overlap'], np.int64) - ref['overlap']).max())
    e['g_verts'] = float(np.abs(np.asarray(got['g_verts'], np.float64) - ref['g_verts'])[keep].max())
    return e


def measure_floors(name):
    return errors(name, ref32(name))


# fp32 restatement against fp64, per case and output (re-measured by tests/test_penetration_ref.py, which fails outside [1/2, 2] x these).
# boxes and flags are exact: their bound is 0.
FLOORS = {
    'two_overlap': dict(phi=1.08e-07, boxes=0.0, overlap=0.0, loss=1.24e-08, g_verts=5.10e-08),
    'two_overlap_linear': dict(phi=1.08e-07, boxes=0.0, overlap=0.0, loss=1.90e-08, g_verts=1.09e-07),
    'third_isolated': dict(phi=9.00e-08, boxes=0.0, overlap=0.0, loss=2.22e-08, g_verts=4.07e-08),
    'touch': dict(phi=1.32e-07, boxes=0.0, overlap=0.0, loss=1.29e-08, g_verts=5.99e-08),
    'gates': dict(phi=1.33e-07, boxes=0.0, overlap=0.0, loss=2.90e-08, g_verts=6.09e-08),
    'padding': dict(phi=1.12e-07, boxes=0.0, overlap=0.0, loss=2.79e-08, g_verts=1.11e-07),
    'lobes': dict(phi=7.26e-08, boxes=0.0, overlap=0.0, loss=1.93e-08, g_verts=5.84e-08),
    'g32': dict(phi=9.60e-08, boxes=0.0, overlap=0.0, loss=4.07e-08, g_verts=1.72e-07),
}


def tol(name):
    return {k: MULTIPLE * FLOORS[name][k] for k in OUTPUTS}


# which cases a mutation must move (every case, unless the mutated piece is not exercised by it; the 32^3 case repeats the code of the others at
# a size that costs seconds per restatement and is kept to the two mutations that change phi itself)
def touched(mut):
    small = tuple(n for n in CASE_NAMES if n != 'g32')
    if mut not in ('plane_distance', 'metres'):
        return tuple(n for n in _touched(mut) if n in small)
    return _touched(mut)


def _touched(mut):
    if mut == 'open_overlap':
        return ('touch',)                                   # only boxes that touch exactly tell the intervals apart
    if mut == 'no_scale_factor':
        return tuple(n for n in CASE_NAMES if cases()[n]['scale_factor'] != 0.0)
    if mut == 'exist':
        return ('gates',)                                   # the only case with inactive persons
    return CASE_NAMES
