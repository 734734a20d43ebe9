"""The definitions of ``lightplane_amd.distortion_loss`` and ``lightplane_amd.interlevel_loss`` in fp64, their inputs and their bars:
tests/test_ray_losses_host.py checks them without a GPU, tests/test_gpu_ray_losses.py holds the kernels (csrc/lp_ray_losses.hip) to them.

The oracles are written from the text of the ops (include/lightplane_hip_losses.h), not from the kernels: the distortion loss as the
sum over ordered pairs, O(S^2), with autograd for its gradients; the interlevel loss with its cell edges in fp32 (so that every
comparison is the one the kernel makes) and everything else in fp64, autograd for the gradient.  The O(S) forms the kernels use are
restated here too (``distortion_scan``, ``interlevel_scan``), in the dtype they are asked for: the host test holds them to autograd of
the definitions in fp64 and, in fp32, to the bars the kernels are held to.

Bars, against fp64 of the same fp32 inputs: ``TOL`` = 1e-4 of the tensor's max for every result and gradient; where ``w, delta >= 0``
every ray's distortion loss and every entry of its gradient to ``w`` is a sum of non-negative terms and is additionally held to
``bar_sum(S) = 4 S 2^-24`` relative (the summation bound of tests/importance_cases.py).
Inputs are built once per process and never modified.
"""
import torch

from tests.points_cases import TOL  # noqa: F401  (the project's bar, re-exported)

RS = (1, 63, 130)
EPS24 = 2.0 ** -24
EPS = 1e-7  # interlevel_loss's default

DIST_SS = (1, 2, 3, 63, 64, 65, 131)
DIST_REGIMES = ("transparent", "opaque", "mixed", "duplicates")
NONNEG = ("transparent", "opaque", "duplicates")  # the regimes with w, delta >= 0
DIST_CASES = [(RS[i % 3], S) for i, S in enumerate(DIST_SS)]
DIST_LIMIT = (3, 2048)

INTER_SS = (2, 3, 63, 64, 65, 131)
INTER_REGIMES = ("covered", "violating", "disjoint", "contains", "duplicates")
# a covering subset of the (S, P) pairs: every size on either side, S < P, S = P and S > P
INTER_PAIRS = [(2, 2), (2, 3), (3, 2), (3, 65), (63, 3), (63, 64), (64, 63), (64, 64), (64, 131), (65, 65), (65, 131), (131, 65),
               (131, 64), (131, 131), (2, 131), (131, 2), (3, 3), (63, 63)]
INTER_CASES = [(RS[i % 3], S, P) for i, (S, P) in enumerate(INTER_PAIRS)]
INTER_LIMIT = (3, 2048, 2048)
_CACHE = {}


def bar_sum(S):
    return 4 * S * EPS24


# ------------------------------------------------------------------------------------------------------------------------------
# distortion
# ------------------------------------------------------------------------------------------------------------------------------

def distortion_pairs(w, d, delta):
    """THE definition: ``2 sum_{i>j} w_i w_j (d_i - d_j) + (1/3) sum_i w_i^2 delta_i`` per ray, in the dtype of its arguments
    (differentiable).  Rays go in blocks so that the ``[r, S, S]`` pair tensor stays small."""
    R, S = w.shape
    lower = torch.tril(torch.ones(S, S, dtype=w.dtype), -1)  # i > j
    out = []
    for r0 in range(0, R, max(1, (1 << 23) // (S * S))):
        r1 = min(R, r0 + max(1, (1 << 23) // (S * S)))
        ww, dd = w[r0:r1], d[r0:r1]
        pairs = (ww[:, :, None] * ww[:, None, :] * (dd[:, :, None] - dd[:, None, :]) * lower).sum((1, 2))
        out.append(2 * pairs + (ww * ww * delta[r0:r1]).sum(-1) / 3)
    return torch.cat(out) if out else w.new_zeros(0)


def distortion_oracle(w, d, delta, g=None):
    """(loss [R], d weights, d depths, d deltas) of the definition in fp64 of the fp32 inputs; ``g``: the loss's gradient (ones)"""
    leaves = [t.double().clone().requires_grad_(True) for t in (w, d, delta)]
    loss = distortion_pairs(*leaves)
    (loss.sum() if g is None else (loss * g.double()).sum()).backward()
    return (loss.detach(),) + tuple(t.grad for t in leaves)


def _excl(x, reverse=False):
    """exclusive prefix (suffix) sums along the ray, as a shifted inclusive scan"""
    if reverse:
        return torch.flip(_excl(torch.flip(x, (1,))), (1,))
    return torch.cat([torch.zeros_like(x[:, :1]), torch.cumsum(x, 1)[:, :-1]], 1)


def distortion_scan(w, d, delta, dtype=torch.float64):
    """(loss, d weights, d depths, d deltas) by the O(S) forms the kernel uses, every operation in ``dtype``"""
    w, d, delta = (t.to(dtype) for t in (w, d, delta))
    gap = torch.cat([d[:, 1:] - d[:, :-1], torch.zeros_like(d[:, :1])], 1)  # gap_k = d_{k+1} - d_k, 0 for the last sample
    A = torch.cumsum(w, 1)
    A_before, R_after = _excl(w), _excl(w, reverse=True)
    D = _excl(gap * A)  # sum_{k < i} gap_k A_k
    E = torch.flip(torch.cumsum(torch.flip(gap * R_after, (1,)), 1), (1,))  # sum_{k >= i} gap_k R_{k+1}
    loss = 2 * (w * D).sum(-1) + (w * w * delta).sum(-1) / 3
    return loss, 2 * (D + E) + 2 * (w * delta) / 3, 2 * w * (A_before - R_after), w * w / 3


def distortion_inputs(R, S, regime):
    """fp32 inputs of one case.  deltas in [0.01, 0.06], depths their running sum from 0.5.
    transparent: weights about 1e-4; opaque: one sample per ray holds 0.97, the rest 1e-6; mixed: moderate weights, every third row all
    zero, row 0 zero from its middle on, in every third row a negative weight; duplicates: moderate weights over depths of which two runs
    of three are equal (S < 8: all depths of a ray equal)."""
    gen = torch.Generator().manual_seed(77000 * R + 10 * S + DIST_REGIMES.index(regime))
    deltas = torch.rand(R, S, generator=gen) * 0.05 + 0.01
    depths = 0.5 + torch.cumsum(deltas, -1)
    u = torch.rand(R, S, generator=gen)
    if regime == "transparent":
        weights = u * 2e-4
    elif regime == "opaque":
        weights = torch.full((R, S), 1e-6)
        weights.scatter_(1, torch.randint(0, S, (R, 1), generator=gen), 0.97)
    elif regime == "mixed":
        weights = u * 0.1
        weights[2::3, S // 3] = -0.05
        weights[1::3] = 0.0
        weights[0, S // 2:] = 0.0
    else:
        weights = u * 0.1
        if S >= 8:
            depths[:, 1:4] = depths[:, 1:2]
            depths[:, S - 4:S - 1] = depths[:, S - 4:S - 3]
        else:
            depths[:, :] = depths[:, :1]
    return dict(weights=weights, depths=depths, deltas=deltas, g=torch.rand(R, generator=gen) + 0.5)


def distortion_case(R, S, regime):
    """the inputs and their oracle (loss, three gradients; ones as the loss's gradient), computed once"""
    key = ("d", R, S, regime)
    if key not in _CACHE:
        c = distortion_inputs(R, S, regime)
        c["ref"] = distortion_oracle(c["weights"], c["depths"], c["deltas"])
        _CACHE[key] = c
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------------
# interlevel
# ------------------------------------------------------------------------------------------------------------------------------

def edges(depths):
    """[R, S + 1] in fp32: the ends of the ray's span and the midpoints in between"""
    assert depths.dtype == torch.float32
    return torch.cat([depths[:, :1], 0.5 * (depths[:, :-1] + depths[:, 1:]), depths[:, -1:]], dim=1)


def touching(d, pd):
    """(lo [R, S], hi [R, S]): proposal cells lo_k .. hi_k - 1 touch target cell k"""
    P = pd.shape[1]
    n = torch.searchsorted(edges(pd).contiguous(), edges(d).contiguous(), right=True)  # proposal edges <= target edge k
    return (n[:, :-1] - 1).clamp(min=0), n[:, 1:].clamp(max=P)


def interlevel_def(w, d, pw, pd, eps=EPS):
    """THE definition, (loss [R], bound [R, S]): ``pw`` in fp64 (differentiable), the comparisons on the fp32 edges, ``eps`` the fp32
    number the kernel is handed"""
    lo, hi = touching(d, pd)
    C = torch.cat([torch.zeros_like(pw[:, :1]), torch.cumsum(pw, 1)], 1)
    bound = C.gather(1, hi) - C.gather(1, lo)
    w64 = w.double()
    x = (w64 - bound).clamp(min=0)
    return (x * x / (w64 + float(torch.tensor(eps, dtype=torch.float32)))).sum(-1), bound


def interlevel_oracle(w, d, pw, pd, eps=EPS, g=None):
    """(loss [R], d proposal_weights [R, P], violated [R, S]: the cells with w_k > bound_k) in fp64 of the fp32 inputs"""
    leaf = pw.double().clone().requires_grad_(True)
    loss, bound = interlevel_def(w, d, leaf, pd, eps)
    (loss.sum() if g is None else (loss * g.double()).sum()).backward()
    return loss.detach(), leaf.grad, w.double() > bound.detach()


def interlevel_scan(w, d, pw, pd, eps=EPS, dtype=torch.float64):
    """(loss, d proposal_weights) by the forms the kernel uses -- the gradient as G[#{k : lo_k <= j}] - G[#{k : hi_k <= j}] -- with the
    prefix sums in ``dtype``"""
    R, P = pw.shape
    lo, hi = touching(d, pd)
    pw, w = pw.to(dtype), w.to(dtype)
    C = torch.cat([torch.zeros_like(pw[:, :1]), torch.cumsum(pw, 1)], 1)
    x = (w - (C.gather(1, hi) - C.gather(1, lo))).clamp(min=0)
    den = w + torch.tensor(eps, dtype=torch.float32).to(dtype)
    G = torch.cat([torch.zeros_like(w[:, :1]), torch.cumsum(-2 * x / den, 1)], 1)
    j = torch.arange(P)[None, :].expand(R, P).contiguous()
    n_lo = torch.searchsorted(lo.contiguous(), j, right=True)
    n_hi = torch.searchsorted(hi.contiguous(), j, right=True)
    return (x * x / den).sum(-1), G.gather(1, n_lo) - G.gather(1, n_hi)


def _sorted_depths(R, S, gen, first=None, last=None):
    """[R, S] ascending; with ``first`` / ``last`` ([R, 1]) stretched onto that span, ends included"""
    d = 0.5 + torch.cumsum(torch.rand(R, S, generator=gen) * 0.05 + 0.01, -1)
    if first is not None:
        d = first + (d - d[:, :1]) / (d[:, -1:] - d[:, :1]) * (last - first)
        d[:, :1], d[:, -1:] = first, last
    return d


def _duplicate(d):
    S = d.shape[1]
    if S >= 8:
        d[:, 1:4] = d[:, 1:2]
        d[:, S - 4:S - 1] = d[:, S - 4:S - 3]
    else:
        d[:, :] = d[:, :1]
    return d


def interlevel_possible(S, P, regime):
    """fine-contains-coarse needs more target samples than proposal samples; every other regime exists at every shape"""
    return regime != "contains" or S > P


def interlevel_inputs(R, S, P, regime):
    """fp32 inputs of one case: target weights in [0, 0.1] over depths with deltas in [0.01, 0.06] from 0.5.
    covered: the proposal is the target's own samples (S = P; otherwise P samples over the same span) and every proposal weight is 1.01 x
    the largest target weight whose cell it touches: the loss and its gradient are exactly 0; violating: a random proposal over the same
    span whose cells hold about a third of what the target cells they touch hold; disjoint: the same with the proposal's span strictly
    inside the target's; contains: target depths = sort(cat(proposal depths, S - P more strictly inside the span)), the include_coarse
    layout with shared end edges; duplicates: violating with two runs of three equal depths on both sides (all equal below 8)."""
    assert interlevel_possible(S, P, regime)
    gen = torch.Generator().manual_seed(91000 * R + 300 * S + P + 7 * INTER_REGIMES.index(regime))
    d = _sorted_depths(R, S, gen)
    w = torch.rand(R, S, generator=gen) * 0.1
    pw = torch.rand(R, P, generator=gen) * 0.03 * min(1.0, S / P)
    first, last = d[:, :1].clone(), d[:, -1:].clone()
    if regime == "covered":
        pd = d.clone() if S == P else _sorted_depths(R, P, gen, first, last)
        lo, hi = touching(d, pd)
        j = torch.arange(P)[None, None, :]
        touch = (lo[:, :, None] <= j) & (j < hi[:, :, None])  # [R, S, P]
        pw = 1.01 * (w[:, :, None] * touch).amax(1)
    elif regime in ("violating", "duplicates"):
        pd = _sorted_depths(R, P, gen, first, last)
        if regime == "duplicates":
            d, pd = _duplicate(d), _duplicate(pd)
    elif regime == "disjoint":
        span = last - first
        pd = _sorted_depths(R, P, gen, first + 0.2 * span, last - 0.25 * span)
    else:
        pd = _sorted_depths(R, P, gen)
        extra = pd[:, :1] + (0.02 + 0.96 * torch.rand(R, S - P, generator=gen)) * (pd[:, -1:] - pd[:, :1])
        d = torch.sort(torch.cat([pd, extra], 1), 1).values
    return dict(weights=w, depths=d.contiguous(), proposal_weights=pw.contiguous(), proposal_depths=pd.contiguous(),
                g=torch.rand(R, generator=gen) + 0.5)


def interlevel_case(R, S, P, regime):
    """the inputs and their oracle (loss, gradient, violated cells; ones as the loss's gradient), computed once"""
    key = ("i", R, S, P, regime)
    if key not in _CACHE:
        c = interlevel_inputs(R, S, P, regime)
        c["ref"] = interlevel_oracle(c["weights"], c["depths"], c["proposal_weights"], c["proposal_depths"])
        _CACHE[key] = c
    return _CACHE[key]
