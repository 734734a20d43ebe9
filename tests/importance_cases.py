"""The definition of ``lightplane_amd.importance_samples`` in fp64, its inputs and its accuracy bar: tests/test_importance_host.py
checks them without a GPU, tests/test_gpu_importance.py holds the kernel (csrc/lp_importance.hip) to them.

The definition is written from the text of the op (lightplane_amd/importance.py, include/lightplane_hip_importance.h), in the dtype it
is asked for: fp64 is the oracle, fp32 the operation-by-operation restatement the host test holds to the same bar as the kernel.

The bar.  The inverse CDF has slope (bin width) / (bin mass), unbounded in a near-empty bin, so "max |err| / max |t|" is no bar a correct
fp32 implementation meets (the fp32 restatement is at 1.2e-4 of max in the opaque regime).  Every new depth is instead held to a mixed
forward-backward bound that leaves no sample out: with F the fp64 CDF of the same fp32 inputs (piecewise linear through
``(e_j, C_j / W)``; where duplicate depths make a zero-width bin it jumps, and has a lower and an upper limit there),

    F_lower(t (1 - B)) - A  <=  u_k  <=  F_upper(t (1 + B)) + A,        A = 4 S 2^-24,   B = 4 2^-24

``A``: any-order fp32 summation of ``S`` positive terms, twice (``C_j`` and ``W``), with margin; ``B``: the roundings of ``t`` itself (the
edge's midpoint, the product, the sum).  Where a bin holds real mass the bar bounds the depth error by ``A (bin width) / (p_j / W)``.
Inputs are built once per process and never modified.
"""
import torch

from tests.points_cases import TOL  # noqa: F401  (the bar of the points and of the gradients, re-exported)

RS = (1, 63, 130)
SS = (2, 3, 63, 64, 65, 131)
NS = (1, 2, 63, 64, 65, 130)
REGIMES = ("transparent", "opaque", "mixed", "duplicates")
PAD = 1e-5
EPS24 = 2.0 ** -24
B = 4 * EPS24
# the shapes of the bar's own check on the CPU (the fp32 restatement)
HOST_SS = (2, 3, 63, 64, 65, 131, 200, 1024)
HOST_NS = (1, 2, 63, 64, 65, 128, 257)
HOST_R = 33
# every (S, N) pair, with the three batch sizes going round; the LDS limit on its own
CASES = [(RS[(i + j) % len(RS)], S, N) for i, S in enumerate(SS) for j, N in enumerate(NS)]
LIMIT_CASE = (3, 2048, 2048)
_CACHE = {}


def bar_a(S):
    return 4 * S * EPS24


def edges(depths):
    """[R, S + 1]: the ends of the ray's span and the midpoints in between, in the dtype of ``depths``"""
    return torch.cat([depths[:, :1], 0.5 * (depths[:, :-1] + depths[:, 1:]), depths[:, -1:]], dim=1)


def masses(weights, pad, dtype):
    """(p [R, S], C [R, S + 1]); ``pad`` enters as the fp32 number the kernel is handed"""
    w = weights.to(dtype)
    p = torch.where(w > 0, w, torch.zeros_like(w)) + torch.tensor(pad, dtype=torch.float32).to(dtype)  # (a NaN is not > 0)
    return p, torch.cat([torch.zeros_like(p[:, :1]), torch.cumsum(p, dim=1)], dim=1)


def targets(R, N, jitter, dtype):
    """u [R, N] = (k + xi) / N"""
    k = torch.arange(N, dtype=dtype)[None, :].expand(R, N)
    xi = torch.full((R, N), 0.5, dtype=dtype) if jitter is None else jitter.to(dtype)
    return (k + xi) / N


def new_depths(depths, weights, N, pad=PAD, jitter=None, dtype=torch.float64):
    """(t [R, N], bin [R, N]) of the definition, computed in ``dtype``"""
    d = depths.to(dtype)
    R, S = d.shape
    e = edges(d)
    _, C = masses(weights, pad, dtype)
    x = targets(R, N, jitter, dtype) * C[:, -1:]
    j = (torch.searchsorted(C.contiguous(), x.contiguous(), right=True) - 1).clamp(0, S - 1)  # the last bin with C_j <= x
    c0, c1 = C.gather(1, j), C.gather(1, j + 1)
    den = c1 - c0
    a = torch.where(den > 0, (x - c0) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den)).clamp(0, 1)
    e0, e1 = e.gather(1, j), e.gather(1, j + 1)
    return torch.minimum(torch.maximum(e0 + a * (e1 - e0), e0), e1), j


def resample(origins, directions, depths, weights, N, pad=PAD, jitter=None, include_coarse=True, dtype=torch.float64):
    """(points, depths', deltas') of the definition in ``dtype``"""
    t, _ = new_depths(depths, weights, N, pad, jitter, dtype)
    return assemble(origins, directions, depths, t, include_coarse, dtype)


def assemble(origins, directions, depths, t, include_coarse, dtype):
    """merge, deltas and points for given new depths ``t``: values are copied, never recomputed"""
    out = torch.sort(torch.cat([depths.to(dtype), t.to(dtype)], dim=1), dim=1, stable=True).values if include_coarse else t.to(dtype)
    if out.shape[1] > 1:
        diff = out[:, 1:] - out[:, :-1]
        deltas = torch.cat([diff[:, :1], diff], dim=1)
    else:
        deltas = torch.ones_like(out)
    points = out[..., None] * directions.to(dtype)[:, None] + origins.to(dtype)[:, None]
    return points, out, deltas


def cdf_limit(depths, weights, pad, q, upper):
    """the lower (``upper=False``) or upper limit at ``q [R, N]`` (fp64) of the fp64 CDF of the fp32 inputs"""
    e = edges(depths.double())
    p, C = masses(weights, pad, torch.float64)
    S = p.shape[1]
    m = torch.searchsorted(e.contiguous(), q.contiguous(), right=upper)  # edges < q (lower) / <= q (upper)
    i = (m - 1).clamp(0, S - 1)  # bin [e_i, e_{i+1}] has q inside and a positive width wherever 0 < m <= S
    e0, e1 = e.gather(1, i), e.gather(1, i + 1)
    width = torch.where(e1 > e0, e1 - e0, torch.ones_like(e0))
    inside = (C.gather(1, i) + ((q - e0) / width).clamp(0, 1) * p.gather(1, i)) / C[:, -1:]
    return torch.where(m == 0, torch.zeros_like(inside), torch.where(m == S + 1, torch.ones_like(inside), inside))


def bar_excess(t, depths, weights, N, pad=PAD, jitter=None):
    """How far the worst sample of ``t [R, N]`` is outside the ``B`` window, in units of ``S 2^-24`` (the bar: <= 4), and the same
    per sample.  Every sample counts."""
    R, S = depths.shape
    t64 = t.detach().double().cpu()
    u = targets(R, N, jitter, torch.float64)
    lo = cdf_limit(depths, weights, pad, t64 * (1 - B), upper=False)
    hi = cdf_limit(depths, weights, pad, t64 * (1 + B), upper=True)
    excess = torch.maximum(lo - u, u - hi) / (S * EPS24)
    return float(excess.max()), excess


def equal_mass_depths(depths, N, jitter=None):
    """what the definition gives a ray of all-zero weights, in fp64 closed form: every bin holds the same mass ``pad``, so
    ``t_k = e_j + (u_k S - j) (e_{j+1} - e_j)`` with ``j = floor(u_k S)``"""
    e = edges(depths.double())
    R, S = depths.shape
    x = targets(R, N, jitter, torch.float64) * S
    j = x.floor().long().clamp(0, S - 1)
    e0, e1 = e.gather(1, j), e.gather(1, j + 1)
    return e0 + (x - j).clamp(0, 1) * (e1 - e0)


def inputs(R, S, N, regime, seed=None):
    """fp32 inputs of one case.  deltas in [0.01, 0.06], depths their running sum from 0.5.
    transparent: weights about 1e-4; opaque: one bin per ray holds 0.97, the rest 1e-6; mixed: moderate weights, every third row all
    zero, row 0 zero from its middle on, and in every third row a negative and a NaN weight (both count as 0); duplicates: moderate
    weights over depths of which two runs of three are equal -- two zero-width bins (S < 8: all depths of a ray equal, every bin)."""
    gen = torch.Generator().manual_seed(100000 * R + 100 * S + N + 7 * REGIMES.index(regime) if seed is None else seed)
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
        weights[2::3, 0] = -1.0
        weights[2::3, S // 3] = float("nan")
        weights[1::3] = 0.0
        weights[0, S // 2:] = 0.0
    else:
        weights = u * 0.1
        if S >= 8:
            depths[:, 1:4] = depths[:, 1:2]
            depths[:, S - 4:S - 1] = depths[:, S - 4:S - 3]
        else:
            depths[:, :] = depths[:, :1]
    origins = torch.randn(R, 3, generator=gen) * 0.3
    directions = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * (0.5 + torch.rand(R, 1, generator=gen))
    jitter = torch.rand(R, N, generator=gen)
    return dict(origins=origins, directions=directions, depths=depths, weights=weights, jitter=jitter,
                g_points=torch.randn(R, S + N, 3, generator=gen))


def case(R, S, N, regime):
    key = (R, S, N, regime)
    if key not in _CACHE:
        _CACHE[key] = inputs(R, S, N, regime)
    return _CACHE[key]
