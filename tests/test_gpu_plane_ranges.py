"""The tuned Renderer kernels march each grid plane only over the samples that reach it (csrc/lp_plane_range.h, WaveRanges in
csrc/lp_mfma_common.h): per wave of 32 rays, one range of samples per plane, outside of which the plane is neither gathered nor
scattered to.  What is left out has to be exact zeros.

One batch of 256 rays (eight waves), S = 32, a 8^2 x 16 triplane or a 8^3 voxel grid -- the slab of an axis is |c| < 1 + 1/8 --
holds every situation the ranges distinguish:

  wave 0  diagonal rays that enter and leave the slabs of x and z: outside ALL planes for a prefix and a suffix of the march
  wave 1  a pinhole image row through the cube (before and behind the cube only the xy plane is reached)
  wave 2  31 rays that miss every plane at every sample + ONE ray inside the yz plane at exactly one sample (s = 1)
  wave 3  rays grazing the face x = 1 inside and just outside the half-texel border 1 < x < 1.125
  wave 4  rays exactly parallel to an axis, inside and outside the slabs they are parallel to (those slabs keep every sample)
  wave 5  a row of a 45 / 30 deg view
  wave 6  random rays with per-ray near / far, every fourth starting inside the cube
  wave 7  another pinhole row, off-centre

* forward: per-ray outputs are BITWISE the same whether the rays are given in this order or permuted so that every wave mixes
  rays of all kinds -- the ranges of a wave depend on its 32 rays, the outputs of a ray must not;
* gradients: the project's forced-oracle proof (tests/test_gpu_parity.py) at its own tolerances, on both orders;
* a call with contraction on takes the "every sample" fallback and has to pass the same checks.
The segment-parallel march (which small batches take by default and which keeps every sample) is switched off so that the
full-batch kernels run; one case leaves it on.  Every call names march_order="rays": left to "auto", the front-end would hand the
permuted (no longer image-coherent) batch to the transposed march, which is another kernel."""
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from tests.synth import grid_sizes_for, pinhole_rays, random_decoder, random_grids
from tests.test_gpu_parity import _dev, forced_oracle_check, run_hip_renderer

gpu = pytest.mark.gpu
S = 32
G = 8  # cells per axis: slab |c| < 1.125


def _norm(v):
    return v / v.norm(dim=-1, keepdim=True)


def edge_case_rays(enc_dim, gen):
    f32 = torch.float32
    k = torch.arange(32, dtype=f32)
    o, d, near, far = [], [], [], []

    def add(origins, dirs, n, f):
        o.append(origins.to(f32)); d.append(dirs.to(f32))
        near.append(torch.as_tensor(n, dtype=f32).expand(32).clone()); far.append(torch.as_tensor(f, dtype=f32).expand(32).clone())

    # wave 0: x = -3 + t / sqrt 2, z = 3 - t / sqrt 2: both inside their slabs for t in (2.65, 5.83) only; near 1, far 7
    add(torch.stack([-3.0 + 0.01 * k, -0.6 + 0.04 * k, 3.0 - 0.005 * k], -1), _norm(torch.tensor([[1.0, 0.02, -1.0]])).expand(32, 3), 1.0, 7.0)
    # wave 1 / 7: pinhole rows (camera at z = 2.7; near / far bracket the bounding sphere)
    pin = pinhole_rays(32, 32)
    row1, row7 = slice(32 * 15, 32 * 16), slice(32 * 3, 32 * 4)
    add(pin.origins[row1], pin.directions[row1], pin.near[row1], pin.far[row1])
    # wave 2: 31 rays beside the cube in x AND y (slightly tilted: not parallel to any slab) ...
    o2 = torch.stack([5.0 + 0.01 * k, 5.0 - 0.01 * k, torch.full((32,), 3.0)], -1)
    d2 = _norm(torch.tensor([[0.01, 0.013, -1.0]])).expand(32, 3).clone()
    n2, f2 = torch.full((32,), 1.0), torch.full((32,), 5.0)
    # ... and one ray along +y beside the cube in x: y = -2 + 2 s at sample s (step 2), z = 0.5: inside the yz plane at s = 1 only
    o2[13] = torch.tensor([5.0, -3.0, 0.5]); d2[13] = _norm(torch.tensor([0.003, 1.0, 0.002])); n2[13] = 1.0; f2[13] = 63.0
    o.append(o2); d.append(d2); near.append(n2); far.append(f2)
    # wave 3: along -z, x from 1.05 (inside the border) to 1.2 (outside), y likewise on a few rays
    o3 = torch.stack([1.05 + 0.15 * k / 31.0, torch.where(k % 4 == 0, -1.12 + 0.0 * k, 0.3 + 0.0 * k), torch.full((32,), 3.0)], -1)
    add(o3, _norm(torch.tensor([[1e-3, -2e-3, -1.0]])).expand(32, 3), 1.0, 5.0)
    # wave 4: exactly axis-parallel rays (-z, +x, +y), origins inside and outside the slabs they run along
    ax = torch.tensor([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])[(torch.arange(32) % 4)]
    side = torch.where(k < 16, 0.4 + 0.0 * k, 1.1 + 0.01 * (k - 16))  # 1.10 .. 1.25: across the slab face
    o4 = torch.stack([side, -side, side], -1) - 3.0 * ax
    add(o4, ax, 1.0, 5.0)
    # wave 5: a row of the 45 / 30 deg view
    el = pinhole_rays(32, 32, azimuth_deg=45.0, elevation_deg=30.0)
    row5 = slice(32 * 20, 32 * 21)
    add(el.origins[row5], el.directions[row5], el.near[row5], el.far[row5])
    # wave 6: random directions through the cube, per-ray brackets; every fourth starts inside the cube
    u = torch.rand(32, 3, generator=gen) * 2 - 1
    dirs6 = _norm(torch.randn(32, 3, generator=gen))
    start = torch.where((torch.arange(32) % 4 == 0)[:, None], 0.8 * u, u * 0.5 - 3.0 * dirs6)
    o.append(start); d.append(dirs6)
    near.append(0.2 + torch.rand(32, generator=gen)); far.append(4.0 + 2.0 * torch.rand(32, generator=gen))
    add(pin.origins[row7], pin.directions[row7], pin.near[row7], pin.far[row7])
    n = 256
    return lp.Rays(directions=torch.cat(d).contiguous(), origins=torch.cat(o).contiguous(), grid_idx=torch.zeros(n, dtype=torch.long),
                   near=torch.cat(near), far=torch.cat(far), encoding=torch.randn(n, enc_dim, generator=gen))


def inputs(triplane=True, contract=False, mask_oob=False, seed=0):
    gen = torch.Generator().manual_seed(seed)
    sizes = grid_sizes_for((1, G, G, G, 16), triplane)
    grids = random_grids(gen, sizes)
    dec = random_decoder(gen, 2, 2, 2, input_chn=16, hidden_chn=32, color_chn=3, std=0.2)
    rays = edge_case_rays(int(dec.n_hidden_color[0]), gen)
    n = rays.n_rays
    cfg = dict(num_samples=S, gain=2.0, num_samples_inf=0, mask_out_of_bounds_samples=mask_oob, contract_coords=contract,
               inject_noise_sigma=0.0, inject_noise_seed=0)
    up = (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen))
    return dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=up)


def permuted(d, seed=1):
    """The same rays dealt over the waves at random: every wave mixes rays inside and outside every plane."""
    perm = torch.randperm(d["rays"].n_rays, generator=torch.Generator().manual_seed(seed))
    p = dict(d)
    p["rays"] = d["rays"][perm]
    p["upstream"] = tuple(u[perm] for u in d["upstream"])
    return p, perm


@pytest.fixture
def full_batch_kernels():
    """Small batches take the segment-parallel march by default; these tests are about the full-batch kernels."""
    assert lp.config.segment_backward and lp.config.segment_forward
    lp.config.segment_forward = lp.config.segment_backward = False
    try:
        yield
    finally:
        lp.config.segment_forward = lp.config.segment_backward = True


def test_batch_holds_the_cases():
    """The batch is what the docstring says (checked on the host with the kernels' float arithmetic): the lone ray of wave 2 has
    weight in the yz plane at sample 1 and nowhere else, its 31 neighbours nowhere at all; wave 0 is outside every plane before
    and behind the cube; wave 3 has rays inside the border 1 < x < 1.125 and rays beyond it."""
    r = inputs()["rays"]
    step = 1.0 / (S - 1)
    i = torch.arange(S, dtype=torch.float32)
    lin = torch.where(i < S // 2, step * i, 1.0 - step * (S - 1 - i))
    depth = r.near[:, None] + lin[None, :] * (r.far - r.near)[:, None]
    p = depth[..., None] * r.directions[:, None, :] + r.origins[:, None, :]   # [ray, sample, xyz]
    inside = p.abs() < 1.0 + 1.0 / G
    plane = torch.stack([inside[..., 0] & inside[..., 1], inside[..., 0] & inside[..., 2], inside[..., 1] & inside[..., 2]], -1)
    w2 = plane[64:96]
    assert w2[13, :, 2].nonzero().flatten().tolist() == [1] and not w2[13, :, :2].any()
    assert not w2[torch.arange(32) != 13].any()
    w0 = plane[0:32].any(dim=(0, 2))  # samples at which any ray of wave 0 reaches any plane
    assert not w0[:5].any() and not w0[-4:].any() and w0[10:20].all()
    x3 = p[96:128, S // 2, 0]
    assert ((x3 > 1.0) & (x3 < 1.125)).sum() >= 8 and (x3 > 1.125).sum() >= 8
    assert (r.directions[128:160] == 0).sum(dim=-1).eq(2).all()  # axis-parallel


@gpu
@pytest.mark.parametrize("mask_oob", [False, True], ids=["", "mask_oob"])
@pytest.mark.parametrize("triplane", [True, False], ids=["triplane", "voxel"])
def test_forward_is_bitwise_independent_of_the_wave(full_batch_kernels, triplane, mask_oob):
    dev = _dev()
    d = inputs(triplane, mask_oob=mask_oob)
    p, perm = permuted(d)
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"]) == 1  # the tuned family
    a = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, march_order="rays")[0]
    b = run_hip_renderer(p, dev, _lib.LP_KERNEL_AUTO, march_order="rays")[0]
    for nm, x, y in zip(("ray_length", "neg_log_t", "feature"), a, b):
        x, y = x.detach().cpu(), y.detach().cpu()
        assert torch.isfinite(x).all()
        assert torch.equal(x[perm], y), f"{nm}: {int((x[perm] != y).sum())} entries differ between the two ray orders"
    assert float(a[1].abs().max()) > 0  # (something was rendered)


@gpu
@pytest.mark.parametrize("order", ["given", "permuted"])
@pytest.mark.parametrize("triplane", [True, False], ids=["triplane", "voxel"])
def test_gradients_forced_oracle(full_batch_kernels, triplane, order):
    d = inputs(triplane)
    if order == "permuted":
        d = permuted(d)[0]
    forced_oracle_check(f"plane ranges {'triplane' if triplane else 'voxel'} {order}", d, _dev(), march_order="rays")


@gpu
def test_contraction_takes_the_fallback(full_batch_kernels):
    """contract_coords bends the rays: no plane ranges (every sample is marched), same checks."""
    dev = _dev()
    d = inputs(True, contract=True)
    p, perm = permuted(d)
    a = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, march_order="rays")[0]
    b = run_hip_renderer(p, dev, _lib.LP_KERNEL_AUTO, march_order="rays")[0]
    for x, y in zip(a, b):
        assert torch.equal(x.detach().cpu()[perm], y.detach().cpu())
    forced_oracle_check("plane ranges: contraction (fallback)", d, dev, march_order="rays")


@gpu
def test_segmented_march_unchanged():
    """The default path of a batch this small (segment-parallel forward and backward, every sample marched)."""
    forced_oracle_check("plane ranges: segmented march", inputs(True), _dev(), march_order="rays")
