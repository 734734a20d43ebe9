"""The launches of the ragged-width tests: layer widths, channel counts and encoding widths that do not fill a tile of the
shape-generic kernels (tests/test_ragged_widths_host.py checks the tables without a GPU, tests/test_gpu_ragged_widths.py holds the
kernels to the fp64 oracle on them).

The C ABI takes every layer width, channel count and encoding width in [1, LP_MAX_WIDTH = 128]; whatever the MFMA families do not take
runs on the shape-generic kernels (csrc/lp_renderer_generic.hip, lp_generic_mlp.h, lp_splatter_mlp.h, lp_column_mlp.h, the LPR / CPL
kernels of lp_splatter.hip, lp_ray_embedding.hip), whose tail handling -- partial blocks of eight, clamped 32-tiles, odd inner
dimensions, scalar grid rows -- only a width that is NOT a multiple of the tile executes.  The tables below choose such widths.

The BRANCH LEDGER (``LEDGER``) restates those device conditions as pure-Python predicates over a case's widths and ray count, one per
piece of tail handling; each predicate's docstring cites the lines it mirrors.  The host test asserts that every predicate is reached
by a case and that every case reaches a predicate no earlier case reaches: when a kernel's thresholds move, a predicate goes
unreachable and that test fails -- the table is then updated, the entry is not deleted.

Shapes: grids of at most 7 cells per axis, 5-9 samples, no beyond-far samples in the Renderer and MLP-Splatter cases (the forced
proof marches every sample of the nearer range only), ray counts 1 / 63 / 65 / 130 (one lane, a block short of a wave, a wave and one
lane, two waves and two lanes).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch

from lightplane_amd import DecoderParams, SplatterParams
from lightplane_amd.params import flatten_decoder_params, flatten_splatter_params, mlp_numel
from tests.synth import SplatterCase, grid_sizes_for, random_grids, random_rays


# ---- decoders with a width of its own per layer -----------------------------------------------------------------------------------
def _chain(gen, dims, std):
    """weights [in, out] and biases of the layers dims[0] -> dims[1] -> ..., N(0, std)"""
    ws = [torch.randn(i, o, generator=gen) * std for i, o in zip(dims[:-1], dims[1:])]
    bs = [torch.randn(o, generator=gen) * std for o in dims[1:]]
    return ws, bs


def ragged_decoder(gen, trunk_dims, opacity_dims, color_dims, color_chn, pad_color=True, std=0.2) -> DecoderParams:
    """A decoder whose layers each have a width of their own, in the flat wire format (``flatten_decoder_params``).  ``*_dims``: input
    width followed by every layer's output width (``trunk_dims`` empty: the two-grid decoder); the opacity head ends in 1, the colour
    head in ``color_chn``, which ``pad_color`` pads to 16 columns as the reference's wire format does."""
    assert opacity_dims[-1] == 1 and color_dims[-1] == color_chn
    wt, bt = _chain(gen, trunk_dims, std) if len(trunk_dims) > 1 else ([], [])
    wo, bo = _chain(gen, opacity_dims, std)
    wc, bc = _chain(gen, color_dims, std)
    flat, nt, no, nc = flatten_decoder_params(wt, bt, wo, bo, wc, bc, pad_color)
    return DecoderParams(flat, nt, no, nc, color_chn)


def ragged_splatter_mlp(gen, dims, std=0.2) -> SplatterParams:
    return SplatterParams(*flatten_splatter_params(*_chain(gen, dims, std)))


@dataclass(frozen=True)
class RaggedRendererCase:
    """One Renderer launch; ``build()`` gives the dictionary of ``tests.synth.RendererCase.build()``."""
    name: str
    seed: int
    n_rays: int
    grid_base: tuple                      # [B, D, H, W, C]
    trunk: tuple                          # () for the two-grid decoder
    opacity: tuple
    color: tuple
    color_chn: int
    pad_color: bool = True
    is_triplane: bool = False
    extra_voxel: bool = False
    num_samples: int = 7
    gain: float = 1.0
    mask_oob: bool = False
    contract: bool = False
    scaffold_size: Optional[tuple] = None
    color_grid_base: Optional[tuple] = None   # two-grid decoder: the colour grid-list (a voxel grid of this size)
    std: float = 0.2

    @property
    def two_grid(self) -> bool:
        return self.color_grid_base is not None

    def build(self):
        gen = torch.Generator().manual_seed(self.seed)
        B, C = self.grid_base[0], self.grid_base[-1]
        sizes = grid_sizes_for(self.grid_base, self.is_triplane)
        if self.extra_voxel:
            sizes = sizes + [[B, 4, 3, 5, C]]
        grids = random_grids(gen, sizes)
        color_grids = random_grids(gen, grid_sizes_for(self.color_grid_base, False)) if self.two_grid else None
        dec = ragged_decoder(gen, self.trunk, self.opacity, self.color, self.color_chn, self.pad_color, self.std)
        rays = random_rays(gen, self.n_rays, B, int(dec.n_hidden_color[0]))
        scaffold = None if self.scaffold_size is None else (torch.rand(B, *self.scaffold_size, generator=gen) > 0.4).float()
        cfg = dict(num_samples=self.num_samples, gain=self.gain, num_samples_inf=0, mask_out_of_bounds_samples=self.mask_oob,
                   contract_coords=self.contract, inject_noise_sigma=0.0, inject_noise_seed=0)
        up = (torch.randn(self.n_rays, generator=gen), torch.randn(self.n_rays, generator=gen),
              torch.randn(self.n_rays, self.color_chn, generator=gen))
        return dict(rays=rays, grids=grids, color_grids=color_grids, decoder=dec, scaffold=scaffold, cfg=cfg, sizes=sizes, upstream=up)


#   widths as in -> ... -> out; what each case aims at is what tests/test_ragged_widths_host.py derives from the ledger
RENDERER_CASES = [
    # every layer per lane (`dense`), the n_out < 4 backward with d_in % 8 != 0, scalar grid rows, staging rows of 17 floats: the
    # per-lane scatter; ACT_CAP 256 with the parameter gradients in LDS
    RaggedRendererCase("narrow", seed=701, n_rays=63, grid_base=(2, 5, 6, 7, 5), trunk=(5, 7, 9), opacity=(9, 6, 1), color=(9, 11, 3),
                       color_chn=3, mask_oob=True, std=0.4),
    # both matrix-core thresholds from either side, d_in = 8, an unpadded colour head (ldw = 3)
    RaggedRendererCase("threshold", seed=702, n_rays=65, grid_base=(1, 6, 5, 7, 8), trunk=(8, 24, 23), opacity=(23, 24, 1),
                       color=(23, 25, 3), color_chn=3, pad_color=False, is_triplane=True, num_samples=5, contract=True, std=0.3),
    # odd d_in, the second tile of one column, dump words for the widths 33 / 47 / 31, more than 16 colour channels
    RaggedRendererCase("odd_mfma", seed=703, n_rays=130, grid_base=(3, 5, 6, 4, 12), trunk=(12, 33, 47), opacity=(47, 31, 1),
                       color=(47, 17, 20), color_chn=20, is_triplane=True, extra_voxel=True, num_samples=6, gain=3.0,
                       scaffold_size=(6, 4, 5), std=0.2),
    # `dense` with full and partial blocks (9, 20, 23, 7), the backward's row and column tails; one ray
    RaggedRendererCase("blocks", seed=704, n_rays=1, grid_base=(1, 7, 5, 6, 20), trunk=(20, 9, 23), opacity=(23, 20, 1),
                       color=(23, 7, 5), color_chn=5, num_samples=9, std=0.3),
    # ACT_CAP 1024, parameters beyond 96 KB: global dW atomics; the second 64 channels of a row; the `more` prefetch
    RaggedRendererCase("wide_ragged", seed=705, n_rays=65, grid_base=(2, 6, 5, 7, 100), trunk=(100, 127, 65), opacity=(65, 100, 1),
                       color=(65, 96, 3), color_chn=3, is_triplane=True, num_samples=8, mask_oob=True, std=0.12),
    # every private array at LP_MAX_WIDTH; the layer widths sum to 897 <= 1024
    RaggedRendererCase("max", seed=706, n_rays=130, grid_base=(1, 4, 5, 6, 128), trunk=(128, 128, 128), opacity=(128, 128, 1),
                       color=(128, 128, 128), color_chn=128, num_samples=9, std=0.12),
    # separate colour grid-list of another size, ReLU on the raw samples
    RaggedRendererCase("two_grid", seed=707, n_rays=63, grid_base=(2, 6, 5, 7, 20), trunk=(), opacity=(20, 24, 1), color=(20, 9, 4),
                       color_chn=4, is_triplane=True, color_grid_base=(2, 4, 3, 7, 20), contract=True, scaffold_size=(5, 4, 6), std=0.3),
    # (beyond the seven above: the one ACT_CAP / LDS pairing they leave out -- widths summing past 256 with parameters that fit LDS)
    RaggedRendererCase("deep_ragged", seed=708, n_rays=65, grid_base=(1, 5, 7, 6, 36), trunk=(36, 41, 39, 42, 40), opacity=(40, 38, 37, 1),
                       color=(40, 43, 40, 3), color_chn=3, is_triplane=True, num_samples=5, std=0.22),
]


@dataclass(frozen=True)
class RaggedMlpSplatterCase:
    """One MLP-Splatter launch; ``build()`` gives the dictionary of ``tests.synth.SplatterCase.build()`` (``use_mlp``)."""
    name: str
    seed: int
    n_rays: int
    dims: tuple                 # feature width -> hidden ... -> output channels
    out_base: tuple             # [B, D, H, W]
    in_base: tuple
    is_triplane: bool = False
    in_triplane: bool = False
    num_samples: int = 7
    mask_oob: bool = False
    contract: bool = False
    std: float = 0.2
    use_mlp: bool = True

    def build(self):
        gen = torch.Generator().manual_seed(self.seed)
        B = self.out_base[0]
        out_sizes = grid_sizes_for(tuple(self.out_base) + (self.dims[-1],), self.is_triplane)
        rays = random_rays(gen, self.n_rays, B, self.dims[0])
        rays.encoding = torch.rand(self.n_rays, self.dims[0], generator=gen)
        in_sizes = grid_sizes_for(tuple(self.in_base) + (self.dims[0],), self.in_triplane)
        in_grids = random_grids(gen, in_sizes)
        mlp = ragged_splatter_mlp(gen, self.dims, self.std)
        cfg = dict(num_samples=self.num_samples, num_samples_inf=0, mask_out_of_bounds_samples=self.mask_oob, contract_coords=self.contract)
        up = [torch.randn(*s, generator=gen) for s in out_sizes]
        return dict(rays=rays, out_sizes=out_sizes, mlp=mlp, in_grids=in_grids, in_sizes=in_sizes, cfg=cfg, upstream=up)


MLP_SPLATTER_CASES = [
    RaggedMlpSplatterCase("f5_h20_o7", seed=711, n_rays=63, dims=(5, 20, 7), out_base=(2, 6, 5, 7), in_base=(2, 4, 6, 5), in_triplane=True,
                          std=0.4),
    RaggedMlpSplatterCase("f33_h47_h24_o100", seed=712, n_rays=65, dims=(33, 47, 24, 100), out_base=(1, 6, 5, 7), in_base=(1, 4, 6, 5),
                          is_triplane=True, num_samples=5, mask_oob=True, std=0.2),
    RaggedMlpSplatterCase("f12_h9_o3", seed=713, n_rays=17, dims=(12, 9, 3), out_base=(2, 5, 4, 6), in_base=(2, 3, 5, 4), num_samples=9,
                          contract=True, std=0.35),
    RaggedMlpSplatterCase("f128_h128_o128", seed=714, n_rays=130, dims=(128, 128, 128), out_base=(1, 5, 4, 6), in_base=(1, 4, 6, 5),
                          in_triplane=True, num_samples=6, std=0.12),
]

# plain Splatter: one case per channel count; voxel and triplane, 1 / 17 / 130 rays, the mask and beyond-far samples spread over them
SPLATTER_CASES = [
    SplatterCase("ragged_c1_voxel", seed=721, n_rays=17, out_base=(2, 6, 5, 7, 1), num_samples=7),
    SplatterCase("ragged_c3_triplane_mask", seed=722, n_rays=130, out_base=(2, 6, 5, 7, 3), is_triplane=True, num_samples=7, mask_oob=True),
    SplatterCase("ragged_c5_voxel_one_ray", seed=723, n_rays=1, out_base=(1, 5, 6, 7, 5), num_samples=9),
    SplatterCase("ragged_c20_triplane_inf", seed=724, n_rays=17, out_base=(2, 6, 5, 7, 20), is_triplane=True, num_samples=7, num_samples_inf=3,
                 contract=True),
    SplatterCase("ragged_c33_voxel", seed=725, n_rays=130, out_base=(1, 6, 5, 7, 33), num_samples=5),
    SplatterCase("ragged_c100_triplane_mask", seed=726, n_rays=17, out_base=(1, 6, 5, 7, 100), is_triplane=True, num_samples=7, mask_oob=True),
    SplatterCase("ragged_c128_voxel", seed=727, n_rays=130, out_base=(2, 4, 5, 6, 128), num_samples=5, num_samples_inf=2, contract=True),
]

# ray embedding (n_harmonics, E, n_rays): tests/test_gpu_modules.py test_ray_embedding_kernel_matches_torch_ops takes them as they are.
# (10, 85): 256 * (63 + 1 + 85 + 1) * 4 bytes = 150 KB exactly, the largest tile the fused path accepts
EMBEDDING_CASES = [(3, 3, 257), (1, 1, 5), (0, 33, 64), (10, 85, 300)]

NORMALIZE_CHANNELS = (3, 100)   # lp_splatter_normalize alone: the scalar and the float4 branch at a width that is not a power of two


# ---- what a launch looks like to the device code ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    """The widths and counts the device conditions of the ledger read.  ``layers``: (d_in, ldw, n_out) of every dense layer in
    evaluation order -- ldw the row stride of its weight matrix, n_out the columns evaluated (1 of the opacity head's last layer,
    color_chn of the colour head's).  ``sites``: widths of the ReLU sites of the dump.  ``total``: floats of the private activation
    array (make_plan).  ``n_params``: floats of mlp_params."""
    kind: str                      # renderer | mlp_splatter | splatter | embedding | points | scaffold
    name: str
    n_rays: int = 0
    C: int = 0                     # channels of the grid-list that is sampled / scattered into
    layers: Tuple[Tuple[int, int, int], ...] = ()
    sites: Tuple[int, ...] = ()
    total: int = 0
    n_params: int = 0
    stage_ld: int = 0
    color_ldw: int = 0
    color_chn: int = 0
    two_grid: bool = False
    n_harmonics: int = 0           # embedding
    E: int = 0

    @property
    def id(self) -> str:
        return f"{self.kind}:{self.name}"


def _mlp_layers(dims, n_out_last=None):
    dims = [int(v) for v in dims]
    out = []
    for l in range(len(dims) - 1):
        last = l == len(dims) - 2
        out.append((dims[l], dims[l + 1], n_out_last if (last and n_out_last is not None) else dims[l + 1]))
    return out


def decoder_shape(kind, name, n_rays, C, dec, two_grid) -> Shape:
    """csrc/lp_generic_decode.h make_plan (:140) and generic_stage_ld (:164) on a decoder's widths"""
    t, o, c = ([int(v) for v in x] for x in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color))
    layers = _mlp_layers(t) + _mlp_layers(o, 1) + _mlp_layers(c, int(dec.color_chn))
    head_w = C if (two_grid or len(t) < 2) else t[-1]
    total = C + (C if two_grid else 0) + sum(t[1:]) + (C if (two_grid or len(t) < 2) else 0) + head_w + sum(o[1:]) + sum(c[1:])
    sites = ([C] + o[1:-1] + [C] + c[1:-1]) if two_grid else (t[1:] + o[1:-1] + c[1:-1])
    return Shape(kind, name, n_rays=n_rays, C=C, layers=tuple(layers), sites=tuple(sites), total=total,
                 n_params=sum(mlp_numel(x) for x in (t, o, c) if len(x) > 1), stage_ld=max([C] + t + o + c) + 1,
                 color_ldw=c[-1], color_chn=int(dec.color_chn), two_grid=two_grid)


def renderer_shape(case: RaggedRendererCase) -> Shape:
    gen = torch.Generator().manual_seed(0)
    dec = ragged_decoder(gen, case.trunk, case.opacity, case.color, case.color_chn, case.pad_color, 1.0)
    return decoder_shape("renderer", case.name, case.n_rays, case.grid_base[-1], dec, case.two_grid)


def mlp_splatter_shape(case: RaggedMlpSplatterCase) -> Shape:
    """csrc/lp_splatter_mlp.h make_plan (:206)"""
    dims = list(case.dims)
    return Shape("mlp_splatter", case.name, n_rays=case.n_rays, C=dims[0], layers=tuple(_mlp_layers(dims)), sites=tuple(dims[1:-1]),
                 total=sum(dims), n_params=mlp_numel(dims), stage_ld=max(dims) + 1)


def splatter_shape(case: SplatterCase) -> Shape:
    return Shape("splatter", case.name, n_rays=case.n_rays, C=case.out_base[-1])


def embedding_shape(t) -> Shape:
    n_h, e, n = t
    return Shape("embedding", f"h{n_h}_e{e}_n{n}", n_rays=n, n_harmonics=n_h, E=e)


def lattice_shape(kind, name, C, n_t, n_o, n_c, hidden, n_rays=0) -> Shape:
    """the uniform-width decoders of tests/points_cases.py and tests/test_gpu_scaffold.py (tests.synth.random_decoder)"""
    two = n_t == 0
    head_in = C if two else hidden
    t = [C] + [hidden] * n_t if n_t else []
    o = [head_in] + [hidden] * (n_o - 1) + [1]
    c = [head_in] + [hidden] * (n_c - 1) + [16]
    return Shape(kind, name, n_rays=n_rays, C=C, layers=tuple(_mlp_layers(t) + _mlp_layers(o, 1) + _mlp_layers(c, 3)), color_ldw=16,
                 color_chn=3)


RAGGED_POINTS_ROWS = ("voxel_c5_222x7_mask", "triplane_c20_222x33_scaffold")
RAGGED_SCAFFOLD_ROWS = ("width7_voxel_c5_22_r1", "width33_triplane_c20_22_r3")


def all_shapes() -> List[Shape]:
    """Every launch of the ragged-width tests in table order: the tables above, then the two ragged rows each of
    tests/points_cases.py and tests/test_gpu_scaffold.py."""
    from tests import points_cases as PC
    from tests.test_gpu_scaffold import CASES as SC
    out = [renderer_shape(c) for c in RENDERER_CASES] + [mlp_splatter_shape(c) for c in MLP_SPLATTER_CASES]
    out += [splatter_shape(c) for c in SPLATTER_CASES] + [embedding_shape(t) for t in EMBEDDING_CASES]
    for name in RAGGED_POINTS_ROWS:
        _, base, (n_t, n_o, n_c, hidden), (R, N), *_ = PC.CASES[name]
        out.append(lattice_shape("points", name, base[4], n_t, n_o, n_c, hidden, R * N))
    for name in RAGGED_SCAFFOLD_ROWS:
        size, _, base, (n_t, n_o, hidden), *_ = SC[name]
        out.append(lattice_shape("scaffold", name, base[4], n_t, n_o, 2, hidden, size[0] * size[1] * size[2] * size[3]))
    return out


# ---- the branch ledger ----------------------------------------------------------------------------------------------------------------
def fwd_on_mfma(d_in, n_out) -> bool:
    """lp_generic_mlp.h:178 dense_on_mfma"""
    return n_out >= 24 and d_in >= 8


def bwd_on_mfma(d_in, n_out) -> bool:
    """lp_generic_mlp.h:260 dense_bwd_on_mfma"""
    return d_in >= 24 and n_out >= 8


def _generic(s: Shape) -> bool:
    return s.kind in ("renderer", "mlp_splatter")


def _lane_dense(s: Shape):
    """the layers `dense` evaluates per lane: in the Renderer kernels and the MLP-Splatter backward's recompute the ones the matrix
    cores do not take (lp_generic_decode.h:40, lp_splatter_mlp.h:52); in the MLP-Splatter FORWARD kernel every layer (Xs = nullptr,
    lp_splatter_mlp.h:82)"""
    if s.kind == "mlp_splatter":
        return list(s.layers)
    return [l for l in s.layers if not fwd_on_mfma(l[0], l[2])] if s.kind == "renderer" else []


def _wave_dense(s: Shape):
    return [l for l in s.layers if fwd_on_mfma(l[0], l[2])] if _generic(s) else []


def _lane_bwd(s: Shape):
    return [l for l in s.layers if not bwd_on_mfma(l[0], l[2])] if _generic(s) else []


def _wave_bwd(s: Shape):
    return [l for l in s.layers if bwd_on_mfma(l[0], l[2])] if _generic(s) else []


def _rows_left(d_in, n_out):
    """rows the four-row loop of dense_bwd_input sees: all of them, or what the eight-row loop of the n_out < 4 path leaves"""
    return d_in % 8 if n_out < 4 else d_in


def dense_partial_block_after_full_blocks(s):
    """lp_generic_mlp.h:19 / :37 `dense`: one or more full blocks of eight outputs, then the partial block (n_out = 9, 20, 23)"""
    return any(n > 8 and n % 8 for _, _, n in _lane_dense(s))


def dense_partial_block_rem_2_6_7(s):
    """lp_generic_mlp.h:40-43 `dense`: a partial block with rem = n_out % 8 other than 1, 3, 4 or 5 (all that the opacity head and the
    colour heads of uniform-width decoders produce): kk[] clamps 6, 2 or 1 spare slots"""
    return any(n % 8 in (2, 6, 7) for _, _, n in _lane_dense(s))


def dense_unpadded_colour_head(s):
    """lp_generic_mlp.h:53 `dense` (`w[kk[k]]`, `w += ldw`): a colour head whose weight rows are color_chn floats long (no padding to
    16 columns) -- a spare slot that was not clamped would read the next row, the last row's past the matrix"""
    return s.kind == "renderer" and s.color_ldw == s.color_chn and s.color_chn % 8 != 0 and s.color_chn < 24


def bwd_input_few_outputs_rows_not_multiple_of_8(s):
    """lp_generic_mlp.h:70 / :80 `dense_bwd_input`: the n_out < 4 path with d_in % 8 != 0 -- the eight-row loop leaves rows to the
    general loops below it"""
    return any(n < 4 and d % 8 for d, _, n in _lane_bwd(s))


def bwd_input_four_row_loop_column_tail(s):
    """lp_generic_mlp.h:96 / :122 `dense_bwd_input`: the four-row loop with n_out % 4 != 0 (the scalar column loop after the blocks of
    four outputs)"""
    return any(_rows_left(d, n) >= 4 and n % 4 for d, _, n in _lane_bwd(s))


def bwd_input_row_tail(s):
    """lp_generic_mlp.h:134 `dense_bwd_input`: d_in % 4 != 0, the one-row loop"""
    return any(d % 4 for d, _, _ in _lane_bwd(s))


def fwd_mfma_at_its_threshold(s):
    """lp_generic_mlp.h:178 `dense_on_mfma`: n_out = 24 or d_in = 8, the first widths the matrix cores take"""
    return any(n == 24 or d == 8 for d, _, n in _wave_dense(s))


def fwd_mfma_just_below_its_threshold(s):
    """lp_generic_mlp.h:178 `dense_on_mfma`: n_out = 23 with d_in >= 8 (or d_in = 7 with n_out >= 24): the last widths `dense` keeps"""
    return any((n == 23 and d >= 8) or (d == 7 and n >= 24) for d, _, n in _lane_dense(s)) and s.kind == "renderer"


def bwd_mfma_at_its_threshold(s):
    """lp_generic_mlp.h:260 `dense_bwd_on_mfma`: d_in = 24 or n_out = 8"""
    return any(d == 24 or n == 8 for d, _, n in _wave_bwd(s))


def bwd_mfma_just_below_its_threshold(s):
    """lp_generic_mlp.h:260 `dense_bwd_on_mfma`: d_in = 23 with n_out >= 8 (or n_out = 7 with d_in >= 24)"""
    return any((d == 23 and n >= 8) or (n == 7 and d >= 24) for d, _, n in _lane_bwd(s))


def mfma_last_tile_clamped(s):
    """lp_generic_mlp.h:188 / :193 / :251 `dense_wave` (n_out % 32 != 0) and :268 / :327 `dense_bwd_input_wave` (d_in % 32 != 0): the
    last 32-tile re-reads the last column / row and stores only what exists"""
    return any(n % 32 for _, _, n in _wave_dense(s)) and any(d % 32 for d, _, _ in _wave_bwd(s))


def mfma_second_tile_of_one_column(s):
    """lp_generic_mlp.h:187 `dense_wave`: n_out = 33 -- a second 32-tile for ONE column, 31 lanes clamped to it"""
    return any(n % 32 == 1 and n > 32 for _, _, n in _wave_dense(s))


def mfma_inner_dimension_8_to_15(s):
    """lp_generic_mlp.h:200 `dense_wave` (d_in in 8..15) / :276 `dense_bwd_input_wave` (n_out in 8..15): the batched prologue is
    skipped, the pair loop does everything"""
    return any(8 <= d < 16 for d, _, _ in _wave_dense(s)) or any(8 <= n < 16 for _, _, n in _wave_bwd(s))


def mfma_pair_loop_after_the_batches(s):
    """lp_generic_mlp.h:236 `dense_wave` / :312 `dense_bwd_input_wave`: an inner dimension >= 16 that is no multiple of 16 -- pairs
    left after the batches of eight"""
    return any(d >= 16 and d % 16 >= 2 for d, _, _ in _wave_dense(s)) and any(n >= 16 and n % 16 >= 2 for _, _, n in _wave_bwd(s))


def mfma_odd_inner_dimension(s):
    """lp_generic_mlp.h:242 `dense_wave` (odd d_in) and :318 `dense_bwd_input_wave` (odd n_out): the k = 1 half of the last
    instruction carries a zero weight"""
    return any(d % 2 for d, _, _ in _wave_dense(s)) and any(n % 2 for _, _, n in _wave_bwd(s))


def mfma_prefetch_true_once_then_false(s):
    """lp_generic_mlp.h:211 `dense_wave`: 32 <= d_in < 48 -- `more` is true in the first batch and false in the second"""
    return any(32 <= d < 48 for d, _, _ in _wave_dense(s))


def wave_outer_clamped_rows_and_columns(s):
    """lp_generic_mlp.h:500 / :502 / :509 / :513 `wave_outer`: dW of a layer whose d_in and n_out are both no multiple of 32, and
    ragged (no multiple of 16 either): rows AND columns of the last tiles are clamped"""
    return _generic(s) and any(d % 16 and n % 16 for d, _, n in s.layers)


def wave_outer_with_lanes_that_are_not_live(s):
    """lp_generic_mlp.h:560 / :562 `mlp_backward` stages zeros for lanes without a ray (n_rays % 64 != 0) under a clamped `wave_outer`"""
    return wave_outer_clamped_rows_and_columns(s) and s.n_rays % 64 != 0


def one_ray_in_the_wave(s):
    """lp_renderer_generic.hip:111-112 / lp_splatter.hip:25: a single ray -- 63 lanes of the only wave stage zeros / leave at once"""
    return s.kind in ("renderer", "splatter") and s.n_rays == 1


def grid_rows_scalar_path(s):
    """lp_generic_mlp.h:384 `sample_list` (C % 4 != 0: no float4 row loads) and :411 `splat_list`'s channel tail"""
    return _generic(s) and s.C % 4 != 0


def grid_rows_float4_tail(s):
    """lp_generic_mlp.h:376 `sample_list`: C % 4 == 0 but C % 16 != 0 -- float4 loads after (or without) the blocks of 16 channels"""
    return _generic(s) and s.C % 4 == 0 and s.C % 16 != 0


def splat_wave_channel_guard(s):
    """lp_generic_mlp.h:458 / :462 `splat_list_wave`: C is not the 16 / 32 / 64 lanes of a row group -- the `c < C` guards"""
    return _generic(s) and s.stage_ld >= 24 and s.C <= 64 and s.C not in (16, 32, 64)


def splat_wave_second_half_partial(s):
    """lp_generic_mlp.h:463 / :468 `splat_list_wave`: 64 < C < 128 -- the `64 + c < C` guard of the second 64 channels"""
    return _generic(s) and s.stage_ld >= 24 and 64 < s.C < 128


def splat_per_lane_fallback_at_a_ragged_width(s):
    """lp_generic_mlp.h:423 `splat_wave_ok` false (staging rows under 24 floats): lp_renderer_generic.hip:228 /
    lp_splatter_mlp.h:187 fall back to the per-lane `splat_list`, at C % 4 != 0"""
    return _generic(s) and s.stage_ld < 24 and s.C % 4 != 0


def relu_dump_partial_word(s):
    """lp_renderer_generic.hip:184 (`c < width`) / lp_splatter_mlp.h:156: a ReLU site whose width is no multiple of 32"""
    return _generic(s) and any(w % 32 for w in s.sites)


def relu_dump_two_words_per_site(s):
    """lp_renderer_generic.hip:381 generic_dump_shape: a widest site of 33..64 units -- two words per site, the second one partial"""
    return s.kind == "renderer" and 32 < max(s.sites, default=0) < 64


def _lds_acc(s):
    """lp_renderer_generic.hip:405-407 / lp_splatter_mlp.h:237-239"""
    return 4 * (128 * s.stage_ld + s.n_params) <= 96 * 1024


def _ragged(s):
    return any(d % 16 or n % 16 for d, _, n in s.layers)


def act_cap_256_params_in_lds(s):
    """lp_renderer_generic.hip:440 renderer_bwd_generic<256, true>: widths summing to <= 256 floats, parameter gradients accumulated in
    LDS (without grad_mlp_params the same launch is <256, false>: tests/test_gpu_ragged_widths.py runs both)"""
    return s.kind == "renderer" and _ragged(s) and s.total <= 256 and _lds_acc(s)


def act_cap_1024_params_in_lds(s):
    """lp_renderer_generic.hip:442 renderer_bwd_generic<1024, true>: widths summing past 256 with parameters that still fit the 96 KB"""
    return s.kind == "renderer" and _ragged(s) and s.total > 256 and _lds_acc(s)


def act_cap_1024_global_atomics(s):
    """lp_renderer_generic.hip:442 / :407 renderer_bwd_generic<1024, false>: widths summing past 256, parameters beyond 96 KB -- dW
    through global atomics"""
    return s.kind == "renderer" and _ragged(s) and s.total > 256 and not _lds_acc(s)


def every_array_at_max_width(s):
    """include/lightplane_hip.h LP_MAX_WIDTH = 128 (lp_api.hip:49 / :59 / :149): channels, encoding and every layer at the bound the
    private arrays `float x[LP_MAX_WIDTH]` are sized for (lp_renderer_generic.hip:47-48, :129-131)"""
    return _generic(s) and s.C == 128 and all(d == 128 for d, _, _ in s.layers) and (s.kind == "mlp_splatter" or s.color_chn == 128)


def two_grid_relu_on_ragged_samples(s):
    """lp_renderer_generic.hip:190 / :194 (dump sites of width C) and :272-274 (the ReLU masks on the raw samples of both grid-lists):
    the two-grid decoder at C % 16 != 0"""
    return s.kind == "renderer" and s.two_grid and s.C % 16 != 0


def mlp_splatter_scatter_fallback(s):
    """lp_splatter_mlp.h:185-188 splat_mlp_bwd_kernel: staging rows under 24 floats -- the input-grid gradient goes through the per-lane
    `splat_list`"""
    return s.kind == "mlp_splatter" and s.stage_ld < 24


def mlp_splatter_forward_keeps_wide_ragged_layers_per_lane(s):
    """lp_splatter_mlp.h:56 / :82 splat_mlp_fwd_kernel (Xs = nullptr): layers the backward's recompute gives to the matrix cores run
    through `dense` here -- full blocks and a partial one at n_out = 47 / 100"""
    return s.kind == "mlp_splatter" and any(fwd_on_mfma(d, n) and n % 8 for d, _, n in s.layers)


def mlp_splatter_fewer_than_four_output_channels(s):
    """lp_splatter_mlp.h:164-179 splat_mlp_bwd_kernel: C_out < 4 -- the gather of dy over three channels and the n_out < 4 path of
    `dense_bwd_input` (lp_generic_mlp.h:70) on an unpadded last layer (ldw = n_out)"""
    return s.kind == "mlp_splatter" and s.layers[-1][2] < 4


def mlp_splatter_act_cap_1024_global_atomics(s):
    """lp_splatter_mlp.h:239 / :251 splat_mlp_bwd_kernel<1024, false>: widths summing past 256, parameters beyond 96 KB"""
    return s.kind == "mlp_splatter" and s.total > 256 and not _lds_acc(s)


def colour_channels_beyond_16(s):
    """lp_renderer_generic.hip:84 / :139 / :234: 16 < color_chn < 128, beyond the padded 16 columns of the reference's wire format"""
    return s.kind == "renderer" and 16 < s.color_chn < 128


def _lpr(C):
    """lp_splatter.hip:524-526 LP_SPLAT_DISPATCH"""
    lpr = 1
    while lpr < C and lpr < 64:
        lpr <<= 1
    return lpr, (C + lpr - 1) // lpr


def splat_one_lane_per_ray(s):
    """lp_splatter.hip:532 KERNEL<1, 1>: C = 1"""
    return s.kind == "splatter" and _lpr(s.C) == (1, 1)


def splat_four_lanes_one_idle(s):
    """lp_splatter.hip:534 KERNEL<4, 1> with `c < C` false in a lane (:52, :327, :336): C = 3"""
    return s.kind == "splatter" and _lpr(s.C)[0] == 4 and s.C < 4


def splat_eight_lanes_some_idle(s):
    """lp_splatter.hip:535 KERNEL<8, 1> with idle lanes: C = 5 .. 7"""
    return s.kind == "splatter" and _lpr(s.C)[0] == 8 and s.C < 8


def splat_32_lanes_some_idle(s):
    """lp_splatter.hip:537 KERNEL<32, 1> with idle lanes: 16 < C < 32"""
    return s.kind == "splatter" and _lpr(s.C)[0] == 32 and s.C < 32


def splat_64_lanes_one_channel_some_idle(s):
    """lp_splatter.hip:539 KERNEL<64, 1> with idle lanes: 32 < C < 64"""
    return s.kind == "splatter" and _lpr(s.C) == (64, 1) and s.C < 64


def splat_two_channels_per_lane_second_partial(s):
    """lp_splatter.hip:540 KERNEL<64, 2> with `c >= C` slots in the second channel of a lane: 64 < C < 128"""
    return s.kind == "splatter" and _lpr(s.C) == (64, 2) and s.C < 128


def splat_two_channels_per_lane_full(s):
    """lp_splatter.hip:540 KERNEL<64, 2>, C = 128 = LP_MAX_WIDTH (:530 refuses cpl > 2)"""
    return s.kind == "splatter" and s.C == 128


def splat_normalize_scalar_branch(s):
    """lp_splatter.hip:507-509 splat_normalize_kernel: C % 4 != 0"""
    return s.kind == "splatter" and s.C % 4 != 0


def embedding_scalar_stores(s):
    """lp_ray_embedding.hip:71-75 ray_embedding_fwd: E % 4 != 0"""
    return s.kind == "embedding" and s.E % 4 != 0


def embedding_min_width(s):
    """lp_api.hip:895 check_ray_embed: out_dim = 1, the lower end of [1, LP_MAX_WIDTH] (one output, one LDS bias, a 4-byte row)"""
    return s.kind == "embedding" and s.E == 1


def embedding_scalar_stores_after_full_groups(s):
    """lp_ray_embedding.hip:59 / :71: E > 4 with E % 4 != 0 -- whole groups of four outputs that still leave through the scalar branch
    before the partial one"""
    return s.kind == "embedding" and s.E > 4 and s.E % 4 != 0


def embedding_largest_lds_tile(s):
    """lp_ray_embedding.hip:125-126 / lightplane_amd/modules.py:93-94: 256 * (6 n + 3 + 1 + E + 1) * 4 bytes = 150 KB exactly"""
    return s.kind == "embedding" and 256 * (6 * s.n_harmonics + 3 + 1 + s.E + 1) * 4 == 150 * 1024


def points_gather_scalar_rows(s):
    """lp_column_mlp.h:55-65 `sc_gather` in the point-evaluation forward: C % 4 != 0"""
    return s.kind == "points" and s.C % 4 != 0


def points_dense_layer_narrower_than_a_block(s):
    """lp_column_mlp.h:91-110 `sc_dense` in the point-evaluation forward: a hidden layer of fewer than eight units -- the partial block
    alone, rem = 7"""
    return s.kind == "points" and any(1 < n < 8 for _, _, n in s.layers[:-1])


def points_dense_partial_block_after_full_blocks(s):
    """lp_column_mlp.h:76 / :91 `sc_dense` in the point-evaluation forward: hidden 33 -- four full blocks and one output"""
    return s.kind == "points" and any(n > 8 and n % 8 for _, _, n in s.layers)


def lattice_gather_scalar_rows(s):
    """lp_column_mlp.h:55-65 `sc_gather` in the lattice kernel (lp_scaffold.hip): C % 4 != 0"""
    return s.kind == "scaffold" and s.C % 4 != 0


def lattice_dense_partial_block_after_full_blocks(s):
    """lp_column_mlp.h:76 / :91 `sc_dense` in the lattice kernel: hidden 33"""
    return s.kind == "scaffold" and any(n > 8 and n % 8 for _, _, n in s.layers)


LEDGER: List[Callable[[Shape], bool]] = [
    dense_partial_block_after_full_blocks, dense_partial_block_rem_2_6_7, dense_unpadded_colour_head,
    bwd_input_few_outputs_rows_not_multiple_of_8, bwd_input_four_row_loop_column_tail, bwd_input_row_tail,
    fwd_mfma_at_its_threshold, fwd_mfma_just_below_its_threshold, bwd_mfma_at_its_threshold, bwd_mfma_just_below_its_threshold,
    mfma_last_tile_clamped, mfma_second_tile_of_one_column, mfma_inner_dimension_8_to_15, mfma_pair_loop_after_the_batches,
    mfma_odd_inner_dimension, mfma_prefetch_true_once_then_false,
    wave_outer_clamped_rows_and_columns, wave_outer_with_lanes_that_are_not_live, one_ray_in_the_wave,
    grid_rows_scalar_path, grid_rows_float4_tail, splat_wave_channel_guard, splat_wave_second_half_partial,
    splat_per_lane_fallback_at_a_ragged_width,
    relu_dump_partial_word, relu_dump_two_words_per_site,
    act_cap_256_params_in_lds, act_cap_1024_params_in_lds, act_cap_1024_global_atomics, every_array_at_max_width,
    colour_channels_beyond_16, two_grid_relu_on_ragged_samples,
    mlp_splatter_scatter_fallback, mlp_splatter_forward_keeps_wide_ragged_layers_per_lane, mlp_splatter_fewer_than_four_output_channels,
    mlp_splatter_act_cap_1024_global_atomics,
    splat_one_lane_per_ray, splat_four_lanes_one_idle, splat_eight_lanes_some_idle, splat_32_lanes_some_idle,
    splat_64_lanes_one_channel_some_idle, splat_two_channels_per_lane_second_partial, splat_two_channels_per_lane_full,
    splat_normalize_scalar_branch,
    embedding_scalar_stores, embedding_min_width, embedding_scalar_stores_after_full_groups, embedding_largest_lds_tile,
    points_gather_scalar_rows, points_dense_layer_narrower_than_a_block, points_dense_partial_block_after_full_blocks,
    lattice_gather_scalar_rows, lattice_dense_partial_block_after_full_blocks,
]


def reached(s: Shape) -> List[str]:
    return [p.__name__ for p in LEDGER if p(s)]
