"""Host-side selection of the deep hidden-64 FORWARD (lp_renderer_forward_family / _workspace_bytes / _ws): needs no GPU -- the
library loads without one and these entry points answer from shapes alone, or refuse before any launch.

Decoders with hidden width 64 (or 64 grid channels) and 3-4 layers in an MLP keep the shape-generic BACKWARD (kernel_family 0); their
forward runs the layer-looped MFMA forward: family 3 where the weight images fit the 160 KB LDS without the backward's tiles, family 4
(streamed weight images) where they do not."""
import ctypes
import itertools

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from lightplane_amd.renderer import _shape_args, forward_kernel_family, kernel_family
from tests.synth import RENDERER_CASES, grid_sizes_for, random_decoder

LOOP_BLK = 3 * (32 * 64 + 8 * 16)  # bytes of one 32 x 32 block image: three bf16 limbs of rm_bytes(32) (lp_bf3.h, lp_loop.h)
LDS = 160 * 1024


def layer_bytes(rows_in, cols):
    return ((rows_in + 31) // 32) * ((cols + 31) // 32) * LOOP_BLK


def _dec(nt, no, nc, C, hidden=64, color_chn=3, sep=False):
    gen = torch.Generator().manual_seed(0)
    return random_decoder(gen, nt, no, nc, C, hidden, color_chn, use_separate_color_grid=sep)


def _families(dec, C, tri, sep=False, **kw):
    sizes = grid_sizes_for((1, 16, 16, 16, C), tri)
    ckw = dict(color_grid_sizes=sizes, color_grid=[torch.empty(s, device="meta") for s in sizes]) if sep else {}
    return (forward_kernel_family(None, None, dec, grid_sizes=sizes, **ckw, **kw),
            kernel_family(None, None, dec, grid_sizes=sizes, **ckw, **kw))


def test_exported():
    assert "forward_kernel_family" in lp.__all__ and lp.forward_kernel_family is forward_kernel_family


def test_reference_golden_shape_streams():
    d = next(c for c in RENDERER_CASES if c.name == "voxel_deep342_h64_c32").build()
    assert forward_kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"]) == 4
    assert kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"]) == 0


@pytest.mark.parametrize("C,tri,layers", list(itertools.product([16, 32, 64], [False, True], [(3, 3, 3), (4, 4, 4)])))
def test_deep_shapes_stream(C, tri, layers):
    fwd, bwd = _families(_dec(*layers, C), C, tri)
    assert (fwd, bwd) == (4, 0)


@pytest.mark.parametrize("C,tri", list(itertools.product([16, 32], [False, True])))
def test_colour_grid_044_streams(C, tri):
    fwd, bwd = _families(_dec(0, 4, 4, C, sep=True), C, tri, sep=True)
    assert (fwd, bwd) == (4, 0)
    sizes = grid_sizes_for((1, 16, 16, 16, C), tri)
    a = _shape_args(None, _dec(0, 4, 4, C, sep=True), sizes, color_grid=[torch.empty(s, device="meta") for s in sizes])
    assert _lib.lib().lp_renderer_forward_workspace_bytes(ctypes.byref(a)) == _expected_workspace((0, 4, 4), C, sep=True) > 0


def test_resident_and_existing_families():
    assert _families(_dec(3, 2, 2, 32), 32, True) == (3, 0)    # 18 block images: resident without the backward's tiles
    assert _families(_dec(3, 2, 2, 32), 32, False) == (3, 0)
    # wherever the backward's family is 3 or 1, the forward's is the same
    for c in RENDERER_CASES:
        d = c.build()
        kw = dict(color_grid=d["color_grids"], num_samples_inf=d["cfg"]["num_samples_inf"])
        k = kernel_family(d["rays"], d["grids"], d["decoder"], **kw)
        f = forward_kernel_family(d["rays"], d["grids"], d["decoder"], **kw)
        if k in (1, 3):
            assert f == k, c.name
    assert _families(_dec(2, 2, 2, 32), 32, True) == (3, 3)
    assert _families(_dec(2, 2, 2, 16, hidden=32), 16, True) == (1, 1)
    assert _families(_dec(4, 4, 4, 16, hidden=32), 16, True) == (3, 3)


def test_shapes_that_stay_generic():
    for layers in ((3, 3, 3), (4, 4, 4), (3, 4, 2)):
        assert _families(_dec(*layers, 32), 32, False, arithmetic=_lib.LP_ARITH_FP32) == (0, 0)
        assert _families(_dec(*layers, 32), 32, False, kernel=_lib.LP_KERNEL_GENERIC) == (0, 0)
        assert _families(_dec(*layers, 32, hidden=128), 32, False) == (0, 0)
        assert _families(_dec(*layers, 32, color_chn=16), 32, False) == (0, 0)
        assert _families(_dec(*layers, 32), 32, False, num_samples_inf=257) == (0, 0)
    assert _families(_dec(2, 2, 2, 32, color_chn=16), 32, False) == (0, 0)  # 16 colour channels at hidden 64: as before


def test_render_kwargs_forward_to_the_helpers():
    """Every keyword of a render call -- rays_per_row included -- passes through the shape queries; a typo still raises."""
    dec = _dec(4, 4, 4, 32)
    sizes = grid_sizes_for((1, 16, 16, 16, 32), True)
    kw = dict(num_samples=16, gain=1.0, mask_out_of_bounds_samples=True, contract_coords=False, rays_per_row=8, march_order="rays",
              stop_transmittance=0.0)
    assert forward_kernel_family(None, None, dec, grid_sizes=sizes, **kw) == 4
    assert kernel_family(None, None, dec, grid_sizes=sizes, **kw) == 0
    with pytest.raises(TypeError):
        forward_kernel_family(None, None, dec, grid_sizes=sizes, num_sample_inf=1)


def _args(dec, C, tri):
    return _shape_args(None, dec, grid_sizes_for((1, 16, 16, 16, C), tri))


def _expected_workspace(layers, C, H=64, sep=False):
    """The plan the header documents: layers in running order (trunk, opacity hidden, colour hidden); the longest prefix that fits beside a
    two-slot ring of the largest layer stays resident, the rest is streamed; the workspace is the streamed images, no header."""
    nt, no, nc = layers
    hin = H if nt else C  # (no trunk: the heads read the sampled feature)
    dims = [(C if l == 0 else H, H) for l in range(nt)]
    dims += [(hin if l == 0 else H, H) for l in range(no - 1)] + [(hin if l == 0 else H, H) for l in range(nc - 1)]
    sizes = [layer_bytes(*d) for d in dims]
    small = 4 * (64 * len(dims) + 64 + 256 + 8 + 256)  # biases, the heads' output layers, beyond-far table
    votes = 2 * 8 * 4
    if not sep and small + sum(sizes) + votes <= LDS:
        return 0  # (a two-grid decoder always lays the ring out: its resident kernel has no eight-wave form)
    avail = LDS - votes - small - 2 * max(sizes)
    used, i = 0, 0
    while i < len(sizes) and used + sizes[i] <= avail:
        used += sizes[i]
        i += 1
    return sum(sizes[i:])


@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("layers", [(3, 2, 2), (3, 3, 3), (4, 4, 4), (3, 4, 2), (4, 1, 4), (1, 4, 1), (2, 2, 2)])
def test_workspace_bytes(layers, C):
    L = _lib.lib()
    a = _args(_dec(*layers, C), C, False)
    fam = L.lp_renderer_forward_family(ctypes.byref(a))
    ws = L.lp_renderer_forward_workspace_bytes(ctypes.byref(a))
    want = _expected_workspace(layers, C)
    assert ws == want
    assert (ws > 0) == (fam == 4)
    assert ws % LOOP_BLK == 0


def test_workspace_zero_off_family_4():
    L = _lib.lib()
    for dec, C in ((_dec(2, 2, 2, 16, hidden=32), 16), (_dec(4, 4, 4, 32, hidden=32), 32), (_dec(4, 4, 4, 32, hidden=128), 32)):
        assert L.lp_renderer_forward_workspace_bytes(ctypes.byref(_args(dec, C, True))) == 0
    a = _args(_dec(4, 4, 4, 32), 32, True)
    a.arithmetic = _lib.LP_ARITH_FP32
    assert L.lp_renderer_forward_workspace_bytes(ctypes.byref(a)) == 0
    a.arithmetic = _lib.LP_ARITH_DEFAULT
    a.kernel = _lib.LP_KERNEL_GENERIC
    assert L.lp_renderer_forward_workspace_bytes(ctypes.byref(a)) == 0
    assert L.lp_renderer_forward_family(ctypes.byref(a)) == 0


def test_forward_ws_refuses_a_missing_workspace_before_any_launch():
    """A family-4 call with a NULL or short workspace: LP_EINVAL and a message.  Every pointer of the call is a host buffer and there is
    no GPU in this process: a launch would not come back with LP_EINVAL."""
    L = _lib.lib()
    d = next(c for c in RENDERER_CASES if c.name == "voxel_deep342_h64_c32").build()
    from lightplane_amd.grids import make_grid_descs
    dec = d["decoder"]
    a = _shape_args(d["grids"], dec)
    n = d["rays"].directions.shape[0]
    r = d["rays"]
    keep = [r.directions.contiguous(), r.origins.contiguous(), r.grid_idx.to(torch.int32).contiguous(), r.near.contiguous(),
            r.far.contiguous(), r.encoding.contiguous(), dec.mlp_params.contiguous(), torch.cat([g.reshape(-1, g.shape[-1]) for g in d["grids"]]),
            torch.empty(n), torch.empty(n), torch.empty(n, dec.color_chn)]
    a.rays = _lib.make_rays(*keep[:6])
    descs, C, rows = make_grid_descs([list(g.shape) for g in d["grids"]])
    a.grid = _lib.make_grid_list(keep[7], descs, C, rows)
    a.march = _lib.make_march(9, 0, False, False, 1e-5)
    a.mlp_params, a.n_mlp_params = _lib.ptr(keep[6]), keep[6].numel()
    a.gain = 1.0
    a.ray_length, a.neg_log_t, a.feature = _lib.ptr(keep[8]), _lib.ptr(keep[9]), _lib.ptr(keep[10])
    need = L.lp_renderer_forward_workspace_bytes(ctypes.byref(a))
    assert need > 0
    assert L.lp_renderer_forward_ws(ctypes.byref(a), None, 0, None) == -1
    assert "workspace" in L.lp_last_error().decode()
    buf = torch.empty(need, dtype=torch.uint8)
    assert L.lp_renderer_forward_ws(ctypes.byref(a), buf.data_ptr(), need - 1, None) == -1
    assert str(need) in L.lp_last_error().decode()
    assert L.lp_renderer_forward_ws(ctypes.byref(a), None, need, None) == -1


def test_config_switch_is_off_until_the_timing_gate_is_measured():
    """A shape that has not cleared the gate (faster than the shape-generic forward by more than the 2 % spread) keeps the generic
    forward: no shape has been timed yet, so the switch is opt-in."""
    assert lp.config.deep_forward_mfma is False
