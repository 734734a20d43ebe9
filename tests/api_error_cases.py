"""Malformed argument blocks for every entry point of the C ABI, and what replays them.

``CASES`` maps a case id (``"<entry point>/<defect>"``) to a function that builds the block, makes the call and returns its code.
tests/test_api_errors_host.py compares ``run(case id)`` = ``[code, lp_last_error()]`` with tests/golden/api_errors.json, which
scripts/record_api_errors.py (re)writes from the library it runs against.

Every pointer below is fake, so nothing here may reach a kernel.  A case is either refused by a check, or it is an empty batch
(``n_rays == 0``, or ``n_rays * n_pts == 0``) on an entry point whose launcher returns LP_OK before any launch.  That is why the
blocks are empty batches wherever the defect allows it -- the checks of shapes, decoders, options and pointer alignment do not look
at the batch size -- and carry rays only for the rules that need them (a required pointer that is NULL).  Entry points without an
empty batch (TV, resample, scaffold, mesh) list refused blocks only, and the pure queries (``*_workspace_bytes``,
``*_kernel_family``, ...) launch nothing whatever they answer.  A case that returns LP_OK records an empty message: a successful
call leaves lp_last_error() alone.
"""
import ctypes as C

from lightplane_amd import _lib

FAKE = 0x10000        # 16-byte-aligned non-NULL "device pointers", STEP apart: no check dereferences them
STEP = 0x1000000
FAR = 0x40000000      # a second group of buffers, far from the first (aliasing rules)
NAN, INF = float("nan"), float("inf")
TRIPLANE = ((2, 1, 5, 7), (2, 6, 1, 7), (2, 6, 5, 1))
BIG = (2, 1024, 1024, 1024)   # 2^31 rows
DIMS_T, DIMS_O, DIMS_C = [16, 32, 32], [32, 32, 1], [32, 32, 16]

CASES = {}


def _p(k):
    return FAKE + k * STEP


def add(cid, fn):
    assert cid not in CASES, cid
    CASES[cid] = fn


def run(cid):
    """[code, message] of one case."""
    rc = int(CASES[cid]())
    return [rc, _lib.lib().lp_last_error().decode() if rc < 0 else ""]


def numel(dims):
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


def grid_list(sizes, channels, base):
    gl = _lib.LpGridList()
    gl.data, gl.n_grids, gl.channels = base, len(sizes), channels
    row = 0
    for g, s in enumerate(sizes):
        gl.grids[g] = _lib.LpGrid(*s, row, None)
        row += s[0] * s[1] * s[2] * s[3]
    gl.n_rows = row
    return gl


# ---- defects of a grid-list: name -> in-place edit -----------------------------------------------------------------------------------
def _set(**kw):
    def f(gl):
        for k, v in kw.items():
            setattr(gl, k, v)
    return f


def _grid(g, **kw):
    def f(gl):
        for k, v in kw.items():
            setattr(gl.grids[g], k, v)
    return f


def _one_big_grid(gl):
    gl.n_grids, gl.n_rows = 1, 1 << 31
    gl.grids[0] = _lib.LpGrid(*BIG, 0, None)


def _short(gl):
    gl.n_rows -= 1


# what every grid-list check refuses
LIST_DEFECTS = {
    "n_grids_-1": _set(n_grids=-1), "n_grids_0": _set(n_grids=0), "n_grids_9": _set(n_grids=9),
    "channels_0": _set(channels=0), "channels_129": _set(channels=129),
    "extent_0": _grid(1, H=0), "row_offset_-1": _grid(1, row_offset=-1), "rows_outside": _short,
}
# what only the samplers' lists refuse, or only the regulariser's and the resampler's
LIST_RULES = {"batch_mismatch": _grid(1, B=1), "line_grid": _grid(0, D=1, H=1), "ends_at_2^31": _one_big_grid}


def _fam(entries, blocks):
    """the cross product: every block of ``blocks`` (name -> builder of the call's arguments) through every entry of ``entries``
    (name -> call)"""
    for ename, call in entries.items():
        for bname, build in blocks.items():
            add(f"{ename}/{bname}", lambda call=call, build=build: call(build()))


def _edit(base, *edits, **kw):
    """builder: ``base(**kw)`` with ``edits`` applied to it (each a function of the block, or a (dotted path, value) pair)"""
    def build():
        a = base(**kw)
        for e in edits:
            if callable(e):
                e(a)
            else:
                path, value = e
                obj = a
                *head, last = path.split(".")
                for h in head:
                    obj = getattr(obj, h)
                if "[" in last:
                    name, idx = last[:-1].split("[")
                    getattr(obj, name)[int(idx)] = value
                else:
                    setattr(obj, last, value)
        return a
    return build


def _on(field, edit):
    return lambda a: edit(getattr(a, field))


# ---- Renderer ------------------------------------------------------------------------------------------------------------------------
def renderer(n_rays=0, dims_t=DIMS_T, dims_o=DIMS_O, dims_c=DIMS_C, channels=16, color_sizes=None, enc_dim=None, scaffold=None):
    a = _lib.LpRendererArgs()
    r = a.rays
    r.n_rays = n_rays
    r.directions, r.origins, r.grid_idx, r.near_t, r.far_t, r.encoding = (_p(k) for k in range(6))
    r.encoding_dim = (dims_c[0] if dims_c else 0) if enc_dim is None else enc_dim
    a.grid = grid_list(TRIPLANE, channels, _p(6))
    if color_sizes is not None:
        a.color_grid = grid_list(color_sizes, channels, _p(7))
    if scaffold is not None:
        a.scaffold, a.scaffold_shape = _p(8), _lib.LpGrid(*scaffold, 0, None)
    a.march = _lib.make_march(8, 0, True, False, 1e-5)
    a.mlp_params = _p(9)
    n_t, n_o = numel(dims_t), numel(dims_o)
    a.n_mlp_params = n_t + n_o + numel(dims_c)
    a.trunk, a.opacity, a.color = _lib.make_mlp(dims_t, 0), _lib.make_mlp(dims_o, n_t), _lib.make_mlp(dims_c, n_t + n_o)
    a.color_chn, a.gain = 3, 1.0
    a.ray_length, a.neg_log_t, a.feature, a.neg_log_t_ckpt = (_p(k) for k in range(10, 14))
    a.grad_ray_length, a.grad_neg_log_t, a.grad_feature, a.grad_grid, a.grad_mlp_params, a.grad_encoding = (_p(k) for k in range(14, 20))
    return a


TWO_GRID = dict(dims_t=[], dims_o=[16, 32, 1], dims_c=[16, 32, 16], color_sizes=TRIPLANE)


def _L():
    return _lib.lib()


def _ref(a):
    return None if a is None else C.byref(a)


RENDERER_LAUNCHERS = {
    "lp_renderer_forward": lambda a: _L().lp_renderer_forward(_ref(a), None),
    "lp_renderer_forward_ws": lambda a: _L().lp_renderer_forward_ws(_ref(a), None, 0, None),
    "lp_renderer_backward": lambda a: _L().lp_renderer_backward(_ref(a), None),
    "lp_renderer_backward_relu_dump": lambda a: _L().lp_renderer_backward_relu_dump(_ref(a), _p(30), 0, None),
}
RENDERER_QUERIES = {
    "lp_renderer_kernel_family": lambda a: _L().lp_renderer_kernel_family(_ref(a)),
    "lp_renderer_forward_family": lambda a: _L().lp_renderer_forward_family(_ref(a)),
    "lp_renderer_forward_workspace_bytes": lambda a: _L().lp_renderer_forward_workspace_bytes(_ref(a)),
    "lp_renderer_backward_segments": lambda a: _L().lp_renderer_backward_segments(_ref(a)),
    "lp_renderer_relu_dump_words": lambda a: _L().lp_renderer_relu_dump_words(_ref(a)),
}
_corner_rows = {"lp_renderer_corner_rows": lambda a: _L().lp_renderer_corner_rows(_ref(a), _p(31), None)}

# the defects of a decoder, for the three blocks that carry one (Renderer, scaffold, points); `color`: the block has a colour head
def decoder_blocks(base, color=True):
    b = {
        "trunk_n_layers_-1": _edit(base, ("trunk.n_layers", -1)), "trunk_n_layers_9": _edit(base, ("trunk.n_layers", 9)),
        "opacity_n_layers_0": _edit(base, dims_o=[]), "opacity_n_layers_9": _edit(base, ("opacity.n_layers", 9)),
        "trunk_width_0": _edit(base, dims_t=[16, 0, 32]), "trunk_width_200": _edit(base, dims_t=[16, 200, 32]),
        "opacity_width_200": _edit(base, dims_o=[32, 200, 1]),
        "trunk_input_mismatch": _edit(base, dims_t=[32, 32, 32]), "opacity_input_mismatch": _edit(base, dims_o=[16, 32, 1]),
        "opacity_output_2": _edit(base, dims_o=[32, 32, 2]),
        "opacity_offset": _edit(base, lambda a: setattr(a.opacity, "offset", a.opacity.offset + 1)),
        "trunk_offset": _edit(base, ("trunk.offset", 4)),
        "n_mlp_params_one_short": _edit(base, lambda a: setattr(a, "n_mlp_params", a.n_mlp_params - 1)),
        "n_mlp_params_one_more": _edit(base, lambda a: setattr(a, "n_mlp_params", a.n_mlp_params + 1)),
        "mlp_params_null": _edit(base, ("mlp_params", None)),
        "mlp_params_misaligned": _edit(base, ("mlp_params", _p(9) + 4)),
    }
    if color:
        b.update({
            "color_n_layers_-1": _edit(base, ("color.n_layers", -1)), "color_n_layers_0": _edit(base, dims_c=[]),
            "color_width_0": _edit(base, dims_c=[32, 0, 16]), "color_input_mismatch": _edit(base, dims_c=[16, 32, 16]),
            "color_chn_0": _edit(base, ("color_chn", 0)), "color_chn_17": _edit(base, ("color_chn", 17)),
            "encoding_dim_mismatch": _edit(base, enc_dim=16),
            "color_offset": _edit(base, lambda a: setattr(a.color, "offset", a.color.offset + 1)),
            "color_grid_with_trunk": _edit(base, color_sizes=TRIPLANE),
            "color_grid_other_batch": _edit(base, **{**TWO_GRID, "color_sizes": tuple((3,) + s[1:] for s in TRIPLANE)}),
            "color_grid_other_channels": _edit(base, ("color_grid.channels", 32), **TWO_GRID),
            "color_grid_n_grids_9": _edit(base, ("color_grid.n_grids", 9), **TWO_GRID),
            "color_grid_extent_0": _edit(base, _on("color_grid", _grid(2, W=0)), **TWO_GRID),
            "color_grid.data_misaligned": _edit(base, ("color_grid.data", _p(7) + 4), **TWO_GRID),
        })
    return b


def sampler_list_blocks(base, field="grid", **kw):
    """every defect of a grid-list, in the list ``field`` of an empty batch"""
    b = {f"{field}.{name}": _edit(base, _on(field, edit), **kw) for name, edit in {**LIST_DEFECTS, **LIST_RULES}.items()}
    b[f"{field}.data_misaligned"] = _edit(base, (f"{field}.data", _p(6) + 4), **kw)
    b[f"{field}.grids[1].data_misaligned"] = _edit(base, _on(field, _grid(1, data=_p(40) + 4)), **kw)
    return b


_renderer_blocks = {
    "empty_batch": renderer, "empty_batch_two_grid": _edit(renderer, **TWO_GRID), "empty_batch_scaffold": _edit(renderer, scaffold=(2, 5, 4, 6)),
    "n_rays_-1": _edit(renderer, n_rays=-1),
    **{f"rays.{f}_null": _edit(renderer, (f"rays.{f}", None), n_rays=3) for f in ("directions", "origins", "grid_idx", "near_t", "far_t", "encoding")},
    "rays.directions_misaligned": _edit(renderer, ("rays.directions", _p(0) + 4)),
    "rays.encoding_misaligned": _edit(renderer, ("rays.encoding", _p(5) + 4)),
    "rays.row_length_-1": _edit(renderer, ("rays.row_length", -1), n_rays=3),
    "grid.data_null": _edit(renderer, ("grid.data", None), n_rays=3),
    "color_grid.data_null": _edit(renderer, ("color_grid.data", None), n_rays=3, **TWO_GRID),
    "scaffold_misaligned": _edit(renderer, ("scaffold", _p(8) + 4), scaffold=(2, 5, 4, 6)),
    "feature_misaligned": _edit(renderer, ("feature", _p(12) + 4)), "grad_grid_misaligned": _edit(renderer, ("grad_grid", _p(17) + 4)),
    "grad_grid_list[1]_misaligned": _edit(renderer, ("grad_grid_list[1]", _p(41) + 4)),
    "bg_color_misaligned": _edit(renderer, ("bg_color", _p(42) + 4)), "seg_prefix_misaligned": _edit(renderer, ("seg_prefix", _p(43) + 4)),
    "grad_grid_list_for_some_grids": _edit(renderer, ("grad_grid_list[1]", _p(41)), ("grad_grid", None)),
    "num_samples_0": _edit(renderer, ("march.num_samples", 0)), "num_samples_inf_-1": _edit(renderer, ("march.num_samples_inf", -1)),
    "stop_neg_log_t_-1": _edit(renderer, ("stop_neg_log_t", -1.0)), "stop_neg_log_t_nan": _edit(renderer, ("stop_neg_log_t", NAN)),
    "stop_without_ckpt": _edit(renderer, ("stop_neg_log_t", 4.0), ("neg_log_t_ckpt", None)),
    "arithmetic_7": _edit(renderer, ("arithmetic", 7)), "march_order_7": _edit(renderer, ("march_order", 7)),
    "alpha_mode_3": _edit(renderer, ("alpha_mode", 3)), "alpha_mode_-1": _edit(renderer, ("alpha_mode", -1)),
    "alpha_with_alpha_mode_0": _edit(renderer, ("alpha", _p(44))),
    "scaffold_extent_0": _edit(renderer, scaffold=(2, 5, 0, 6)), "scaffold_other_batch": _edit(renderer, scaffold=(3, 5, 4, 6)),
    "mfma_kernel_unavailable": _edit(renderer, ("kernel", _lib.LP_KERNEL_MFMA), dims_t=[16, 24, 24], dims_o=[24, 24, 1], dims_c=[24, 24, 16]),
    "generic_kernel_empty_batch": _edit(renderer, ("kernel", _lib.LP_KERNEL_GENERIC)),
    "looped_family_empty_batch": _edit(renderer, dims_t=[16, 64, 64], dims_o=[64, 64, 1], dims_c=[64, 64, 16]),
    "fp32_arithmetic": _edit(renderer, ("arithmetic", _lib.LP_ARITH_FP32)),
    **sampler_list_blocks(renderer), **decoder_blocks(renderer),
}
_fam(RENDERER_LAUNCHERS, {"args_null": lambda: None, **_renderer_blocks})
_fam({k: RENDERER_LAUNCHERS[k] for k in ("lp_renderer_forward", "lp_renderer_forward_ws")},
     {f"{f}_null": _edit(renderer, (f, None), n_rays=3) for f in ("ray_length", "neg_log_t", "feature")})
_fam({k: RENDERER_LAUNCHERS[k] for k in ("lp_renderer_backward", "lp_renderer_backward_relu_dump")},
     {"neg_log_t_null": _edit(renderer, ("neg_log_t", None), n_rays=3)})
_fam(RENDERER_QUERIES, {"args_null": lambda: None, "default_shape": _edit(renderer, n_rays=4096),
                        "two_grid": _edit(renderer, n_rays=4096, **TWO_GRID), "fp32_arithmetic": _edit(renderer, ("arithmetic", _lib.LP_ARITH_FP32)),
                        "num_samples_inf_65": _edit(renderer, ("march.num_samples_inf", 65)),
                        "deep_h64": _edit(renderer, dims_t=[16, 64, 64, 64, 64], dims_o=[64, 64, 64, 64, 1], dims_c=[64, 64, 64, 64, 16]),  # (= DEEP_H64 below)
                        "ragged": _edit(renderer, dims_t=[16, 24, 24], dims_o=[24, 24, 1], dims_c=[24, 24, 16])})
_fam(_corner_rows, {"args_null": lambda: None, "empty_batch": renderer, "n_rays_-1": _edit(renderer, n_rays=-1),
                    "rays.origins_null": _edit(renderer, ("rays.origins", None), n_rays=3),
                    "rays.far_t_misaligned": _edit(renderer, ("rays.far_t", _p(4) + 4)), "num_samples_0": _edit(renderer, ("march.num_samples", 0)),
                    **{k: v for k, v in sampler_list_blocks(renderer).items() if "misaligned" not in k}})


# lp_renderer_forward_ws looks at its workspace where the decoder streams its weight images (forward family 4): an empty batch of such a
# decoder is refused for a bad workspace before it returns for having no rays
DEEP_H64 = dict(dims_t=[16, 64, 64, 64, 64], dims_o=[64, 64, 64, 64, 1], dims_c=[64, 64, 64, 64, 16])


def _forward_ws(ws=_p(32), ws_short=0):
    a = renderer(**DEEP_H64)
    need = int(_L().lp_renderer_forward_workspace_bytes(C.byref(a)))
    assert need > 0 and _L().lp_renderer_forward_family(C.byref(a)) == 4
    return _L().lp_renderer_forward_ws(C.byref(a), ws, need - ws_short, None)


for _name, _kw in {"workspace_null": dict(ws=None), "workspace_one_byte_short": dict(ws_short=1), "workspace_misaligned": dict(ws=_p(32) + 4),
                   "streamed_empty_batch": dict()}.items():
    add(f"lp_renderer_forward_ws/{_name}", lambda kw=_kw: _forward_ws(**kw))
add("lp_renderer_corner_rows/rows_null", lambda: _L().lp_renderer_corner_rows(C.byref(renderer()), None, None))
add("lp_renderer_backward_relu_dump/dump_null", lambda: _L().lp_renderer_backward_relu_dump(C.byref(renderer()), None, 0, None))
add("lp_renderer_backward_relu_dump/dump_words_wrong", lambda: _L().lp_renderer_backward_relu_dump(C.byref(renderer(n_rays=3)), _p(30), 7, None))


# ---- Splatter and MLP-Splatter ---------------------------------------------------------------------------------------------------------
def splatter(n_rays=0, channels=16, enc_dim=16, dims=None, in_channels=16, in_sizes=TRIPLANE):
    a = _lib.LpSplatterArgs()
    r = a.rays
    r.n_rays = n_rays
    r.directions, r.origins, r.grid_idx, r.near_t, r.far_t, r.encoding = (_p(k) for k in range(6))
    r.encoding_dim = enc_dim
    a.march = _lib.make_march(8, 0, True, False, 1e-5)
    a.out = grid_list(TRIPLANE, channels, _p(6))
    a.out_feature, a.out_weight = _p(10), _p(11)
    a.grad_out, a.weight, a.grad_encoding = _p(12), _p(13), _p(14)
    if dims is not None:
        a.input_grid = grid_list(in_sizes, in_channels, _p(7))
        a.mlp_params, a.n_mlp_params, a.mlp = _p(9), numel(dims), _lib.make_mlp(dims, 0)
        a.grad_input_grid, a.grad_mlp_params = _p(15), _p(16)
    return a


MLP = dict(dims=[16, 32, 16])
SPLATTER_LAUNCHERS = {
    "lp_splatter_forward": lambda a: _L().lp_splatter_forward(_ref(a), None),
    "lp_splatter_backward": lambda a: _L().lp_splatter_backward(_ref(a), None),
}
_mlp_dump = {"lp_mlp_splatter_backward_relu_dump": lambda a: _L().lp_mlp_splatter_backward_relu_dump(_ref(a), _p(30), 0, None)}
_splatter_blocks = {
    "args_null": lambda: None, "empty_batch": splatter, "n_rays_-1": _edit(splatter, n_rays=-1), "march_order_7": _edit(splatter, ("march_order", 7)),
    "samples_per_wave_empty_batch": _edit(splatter, ("march_order", _lib.LP_MARCH_SAMPLES_PER_WAVE)),
    "channels_20_empty_batch": _edit(splatter, channels=20, enc_dim=20),
    **{f"rays.{f}_null": _edit(splatter, (f"rays.{f}", None), n_rays=3) for f in ("directions", "near_t", "encoding")},
    "rays.grid_idx_misaligned": _edit(splatter, ("rays.grid_idx", _p(2) + 4)), "out_weight_misaligned": _edit(splatter, ("out_weight", _p(11) + 4)),
    "grad_out_misaligned": _edit(splatter, ("grad_out", _p(12) + 4)),
    "num_samples_0": _edit(splatter, ("march.num_samples", 0)), "num_samples_inf_-1": _edit(splatter, ("march.num_samples_inf", -1)),
    "feature_width_mismatch": _edit(splatter, enc_dim=32), "encoding_dim_200": _edit(splatter, enc_dim=200, n_rays=3),
    **sampler_list_blocks(splatter, "out"),
}
_mlp_splatter_blocks = {
    "args_null": lambda: None, "empty_batch": _edit(splatter, **MLP), "ragged_empty_batch": _edit(splatter, dims=[16, 24, 16]),
    "mfma_kernel_unavailable": _edit(splatter, ("kernel", _lib.LP_KERNEL_MFMA), dims=[16, 24, 16]),
    "generic_kernel_empty_batch": _edit(splatter, ("kernel", _lib.LP_KERNEL_GENERIC), **MLP),
    "n_layers_9": _edit(splatter, ("mlp.n_layers", 9), **MLP), "width_0": _edit(splatter, dims=[16, 0, 16]), "width_200": _edit(splatter, dims=[16, 200, 16]),
    "input_width_mismatch": _edit(splatter, dims=[32, 32, 16]), "encoding_width_mismatch": _edit(splatter, enc_dim=32, **MLP),
    "output_width_mismatch": _edit(splatter, dims=[16, 32, 32]), "offset_4": _edit(splatter, ("mlp.offset", 4), **MLP),
    "n_mlp_params_one_short": _edit(splatter, ("n_mlp_params", numel(MLP["dims"]) - 1), **MLP),
    "n_mlp_params_one_more": _edit(splatter, ("n_mlp_params", numel(MLP["dims"]) + 1), **MLP),
    "mlp_params_null": _edit(splatter, ("mlp_params", None), **MLP), "mlp_params_misaligned": _edit(splatter, ("mlp_params", _p(9) + 4), **MLP),
    "input_grid_other_batch": _edit(splatter, in_sizes=tuple((3,) + s[1:] for s in TRIPLANE), **MLP),
    "input_grid.data_null": _edit(splatter, ("input_grid.data", None), n_rays=3, **MLP),
    "grad_input_grid_list[2]_misaligned": _edit(splatter, ("grad_input_grid_list[2]", _p(41) + 4), **MLP),
    "grad_input_grid_list_for_some_grids": _edit(splatter, ("grad_input_grid_list[2]", _p(41)), ("grad_input_grid", None), **MLP),
    **sampler_list_blocks(splatter, "input_grid", **MLP),
}
_fam(SPLATTER_LAUNCHERS, _splatter_blocks)
_fam({f"{k}[mlp]": v for k, v in {**SPLATTER_LAUNCHERS, **_mlp_dump}.items()}, _mlp_splatter_blocks)
_fam({"lp_splatter_forward": SPLATTER_LAUNCHERS["lp_splatter_forward"]},
     {f"{f}_null": _edit(splatter, (f, None), n_rays=3) for f in ("out_feature", "out_weight")})
_fam({"lp_splatter_backward": SPLATTER_LAUNCHERS["lp_splatter_backward"]},
     {f"{f}_null": _edit(splatter, (f, None), n_rays=3) for f in ("grad_out", "weight", "grad_encoding")})
add("lp_mlp_splatter_backward_relu_dump/dump_null", lambda: _L().lp_mlp_splatter_backward_relu_dump(C.byref(splatter(**MLP)), None, 0, None))
add("lp_mlp_splatter_backward_relu_dump/dump_words_wrong",
    lambda: _L().lp_mlp_splatter_backward_relu_dump(C.byref(splatter(n_rays=3, **MLP)), _p(30), 7, None))
add("lp_mlp_splatter_backward_relu_dump/one_layer", lambda: _L().lp_mlp_splatter_backward_relu_dump(C.byref(splatter(dims=[16, 16])), _p(30), 0, None))
_shape = (C.c_int32 * 6)()
_fam({"lp_splatter_kernel_family": lambda a: _L().lp_splatter_kernel_family(_ref(a)),
      "lp_mlp_splatter_relu_dump_words": lambda a: _L().lp_mlp_splatter_relu_dump_words(_ref(a)),
      "lp_mlp_splatter_launch_shape": lambda a: _L().lp_mlp_splatter_launch_shape(_ref(a), C.addressof(_shape))},
     {"args_null": lambda: None, "mlp": _edit(splatter, n_rays=4096, **MLP), "ragged_mlp": _edit(splatter, n_rays=4096, dims=[16, 24, 16]),
      "one_layer": _edit(splatter, dims=[16, 16]), "width_200": _edit(splatter, dims=[16, 200, 16]), "n_layers_9": _edit(splatter, ("mlp.n_layers", 9), **MLP),
      "mfma_kernel_unavailable": _edit(splatter, ("kernel", _lib.LP_KERNEL_MFMA), dims=[16, 24, 16])})
add("lp_splatter_kernel_family/plain", lambda: _L().lp_splatter_kernel_family(C.byref(splatter(n_rays=4096))))
add("lp_mlp_splatter_launch_shape/shape_null", lambda: _L().lp_mlp_splatter_launch_shape(C.byref(splatter(**MLP)), None))

for _name, _a in {"n_rows_-1": (_p(0), _p(1), -1, 16), "channels_0": (_p(0), _p(1), 8, 0), "feature_misaligned": (_p(0) + 4, _p(1), 0, 16),
                  "weight_misaligned": (_p(0), _p(1) + 4, 0, 16), "feature_null": (None, _p(1), 8, 16), "weight_null": (_p(0), None, 8, 16),
                  "no_rows": (_p(0), _p(1), 0, 16)}.items():
    add(f"lp_splatter_normalize/{_name}", lambda a=_a: _L().lp_splatter_normalize(*a, None))
for _name, _a in {"n_-1": (_p(0), _p(1), _p(2), -1), "x1_null": (None, _p(1), _p(2), 8), "x2_null": (_p(0), None, _p(2), 8),
                  "out_null": (_p(0), _p(1), None, 8), "n_0": (_p(0), _p(1), _p(2), 0)}.items():
    add(f"lp_hash_randn/{_name}", lambda a=_a: _L().lp_hash_randn(*a, 7, None))


# ---- ray embedding -------------------------------------------------------------------------------------------------------------------
def ray_embed(n_rays=0):
    e = _lib.LpRayEmbedArgs()
    e.n_rays, e.n_harmonics, e.out_dim = n_rays, 3, 32
    e.directions, e.weight, e.bias, e.out, e.grad_out, e.grad_weight, e.grad_bias = (_p(k) for k in range(7))
    return e


_embed = {"lp_ray_embedding_forward": lambda a: _L().lp_ray_embedding_forward(_ref(a), None),
          "lp_ray_embedding_backward": lambda a: _L().lp_ray_embedding_backward(_ref(a), None)}
_fam(_embed, {"args_null": lambda: None, "empty_batch": ray_embed, "n_rays_-1": _edit(ray_embed, n_rays=-1),
              "n_harmonics_11": _edit(ray_embed, ("n_harmonics", 11)), "n_harmonics_-1": _edit(ray_embed, ("n_harmonics", -1)),
              "out_dim_0": _edit(ray_embed, ("out_dim", 0)), "out_dim_129": _edit(ray_embed, ("out_dim", 129)),
              "directions_null": _edit(ray_embed, ("directions", None), n_rays=3),
              **{f"{f}_misaligned": _edit(ray_embed, (f, _p(8) + 4)) for f in ("directions", "weight", "out", "grad_out", "grad_bias")}})
_fam({"lp_ray_embedding_forward": _embed["lp_ray_embedding_forward"]},
     {f"{f}_null": _edit(ray_embed, (f, None), n_rays=3) for f in ("weight", "bias", "out")})
_fam({"lp_ray_embedding_backward": _embed["lp_ray_embedding_backward"]},
     {"grad_out_null": _edit(ray_embed, ("grad_out", None), n_rays=3),
      "grad_weight_and_grad_bias_null": _edit(ray_embed, ("grad_weight", None), ("grad_bias", None), n_rays=3)})


# ---- total-variation regulariser -------------------------------------------------------------------------------------------------------
def tv_list(sizes=TRIPLANE):
    return grid_list(sizes, 16, _p(0))


def _tv_ws(gl):
    return max(int(_L().lp_grid_tv_workspace_bytes(C.byref(gl))), 0)


def _tv_call(name, gl, weights=None, n_weights=0, p=2, loss=_p(1), ws=_p(2), ws_short=0, grad=_p(3), grad_list=None, n_grad_list=0):
    L, g = _L(), _ref(gl)
    nbytes = _tv_ws(gl) - ws_short if gl is not None else 0
    tail = (_p(4), 1.0, grad, grad_list, n_grad_list)
    if name == "lp_grid_tv_forward":
        return L.lp_grid_tv_forward(g, weights, n_weights, p, loss, ws, nbytes, None)
    if name == "lp_grid_tv_backward":
        return L.lp_grid_tv_backward(g, weights, n_weights, p, *tail, 0, None)
    return L.lp_grid_tv_fused(g, weights, n_weights, p, loss, ws, nbytes, *tail, None)


_weights = (C.c_float * 8)(*([1.0] * 8))
_ptrs = (C.c_void_p * 8)(*[_p(20 + g) for g in range(8)])
_alias = (C.c_void_p * 8)(*[_p(0)] * 8)
_TV_LIST_DEFECTS = {**LIST_DEFECTS, "ends_at_2^31": LIST_RULES["ends_at_2^31"]}
for _name in ("lp_grid_tv_forward", "lp_grid_tv_backward", "lp_grid_tv_fused"):
    _blocks = {"grid_null": dict(gl=None), "p_3": dict(p=3), "two_weights_for_three_grids": dict(weights=C.addressof(_weights), n_weights=2),
               "weights_null_with_a_count": dict(n_weights=3), "grid_without_data": dict(edit=_set(data=None))}
    _blocks.update({f"grid.{k}": dict(edit=v) for k, v in _TV_LIST_DEFECTS.items()})
    if _name != "lp_grid_tv_backward":
        _blocks.update({"loss_null": dict(loss=None), "workspace_null": dict(ws=None), "workspace_one_byte_short": dict(ws_short=1),
                        "workspace_misaligned": dict(ws=_p(2) + 4)})
    if _name != "lp_grid_tv_forward":
        _blocks.update({"grad_list_of_2_for_3_grids": dict(grad_list=C.addressof(_ptrs), n_grad_list=2),
                        "grad_list_null_with_a_count": dict(n_grad_list=3), "no_gradient_buffer": dict(grad=None),
                        "grad_aliases_the_grid": dict(grad=_p(0)), "grad_list_aliases_the_grid": dict(grad_list=C.addressof(_alias), n_grad_list=3),
                        "own_data_without_own_gradient": dict(edit=_grid(1, data=_p(5)))})
    for _b, _kw in _blocks.items():
        def _tv(name=_name, kw=_kw):
            kw = dict(kw)
            gl = kw.pop("gl", tv_list())
            if "edit" in kw:
                kw.pop("edit")(gl)
            return _tv_call(name, gl, **kw)
        add(f"{_name}/{_b}", _tv)
_fam({"lp_grid_tv_workspace_bytes": lambda gl: _L().lp_grid_tv_workspace_bytes(_ref(gl))},
     {"grid_null": lambda: None, "triplane": tv_list, **{f"grid.{k}": _edit(tv_list, v) for k, v in {**LIST_DEFECTS, **LIST_RULES}.items()}})


# ---- resampling ------------------------------------------------------------------------------------------------------------------------
DST = ((2, 1, 9, 13), (2, 11, 1, 13), (2, 11, 9, 1))
_coeffs = {"coefficient_0": (C.c_float * 9)(*([1.0] * 4 + [0.0] + [1.0] * 4)), "coefficient_inf": (C.c_float * 9)(*([1.0] * 8 + [INF])),
           "coefficient_nan": (C.c_float * 9)(*([NAN] + [1.0] * 8)), "coefficient_-1": (C.c_float * 9)(*([1.0, -1.0] + [1.0] * 7))}


def _resample(name, src_edit=None, dst_edit=None, src=True, dst=True, align=0, coeffs=None, dst_base=FAR):
    s, d = grid_list(TRIPLANE, 16, _p(0)), grid_list(DST, 16, dst_base)
    if src_edit:
        src_edit(s)
    if dst_edit:
        dst_edit(d)
    head = (C.byref(s) if src else None, C.byref(d) if dst else None, align, C.addressof(coeffs) if coeffs is not None else None)
    if name == "lp_grid_resample_forward":
        return _L().lp_grid_resample_forward(*head, None)
    return _L().lp_grid_resample_backward(*head, 0, None)


for _name in ("lp_grid_resample_forward", "lp_grid_resample_backward"):
    _blocks = {"source_null": dict(src=False), "destination_null": dict(dst=False), "align_corners_2": dict(align=2), "align_corners_-1": dict(align=-1),
               "two_source_grids_for_three": dict(src_edit=_set(n_grids=2)), "other_channels": dict(dst_edit=_set(channels=32)),
               "other_batch": dict(dst_edit=_grid(1, B=1)), "source_without_data": dict(src_edit=_set(data=None)),
               "destination_without_data": dict(dst_edit=_set(data=None)), "source_2_byte_aligned": dict(src_edit=_set(data=_p(0) + 2)),
               "source_aliases_destination": dict(dst_base=_p(0)), "destination_overlaps_source": dict(dst_base=_p(0) + 64),
               **{k: dict(coeffs=v) for k, v in _coeffs.items()}}
    for _k, _v in _TV_LIST_DEFECTS.items():
        _blocks[f"source.{_k}"] = dict(src_edit=_v)
        _blocks[f"destination.{_k}"] = dict(dst_edit=_v)
    for _b, _kw in _blocks.items():
        add(f"{_name}/{_b}", lambda name=_name, kw=_kw: _resample(name, **kw))


# ---- the decoder at points -------------------------------------------------------------------------------------------------------------
def points(n_rays=0, n_pts=5, dims_t=DIMS_T, dims_o=DIMS_O, dims_c=DIMS_C, channels=16, color_sizes=None, enc_dim=None, scaffold=None):
    a = _lib.LpPointsArgs()
    a.grid = grid_list(TRIPLANE, channels, _p(6))
    if color_sizes is not None:
        a.color_grid = grid_list(color_sizes, channels, _p(7))
    if scaffold is not None:
        a.scaffold, a.scaffold_shape = _p(8), _lib.LpGrid(*scaffold, 0, None)
    a.mlp_params = _p(9)
    n_t, n_o = numel(dims_t), numel(dims_o)
    a.n_mlp_params = n_t + n_o + numel(dims_c)
    a.trunk, a.opacity, a.color = _lib.make_mlp(dims_t, 0), _lib.make_mlp(dims_o, n_t), _lib.make_mlp(dims_c, n_t + n_o)
    a.color_chn, a.gain = 3, 1.0
    a.points, a.grid_idx, a.encoding = _p(0), _p(1), _p(2)
    a.encoding_dim = (dims_c[0] if dims_c else 0) if enc_dim is None else enc_dim
    a.n_rays, a.n_pts = n_rays, n_pts
    a.opacity_out, a.color_out, a.grad_opacity, a.grad_color = (_p(k) for k in range(10, 14))
    return a


def _no_color(a):
    a.color_out = a.grad_color = None


_points = {"lp_points_forward": lambda a: _L().lp_points_forward(_ref(a), None),
           "lp_points_backward": lambda a: _L().lp_points_backward(_ref(a), None)}
_point_batch = lambda base: {  # noqa: E731
    "n_rays_-1": _edit(base, n_rays=-1), "n_pts_-2": _edit(base, n_pts=-2), "too_many_wavefronts": _edit(base, n_rays=1 << 31, n_pts=1 << 31),
    "no_rays": base, "no_points_per_ray": _edit(base, n_rays=3, n_pts=0)}
_fam(_points, {
    "args_null": lambda: None, **_point_batch(points), "empty_batch_two_grid": _edit(points, **TWO_GRID), "empty_batch_scaffold": _edit(points, scaffold=(2, 5, 4, 6)),
    "opacity_only_without_colour_head": _edit(points, _no_color, ("encoding", None), dims_c=[]),
    "opacity_only_other_encoding_dim": _edit(points, _no_color, enc_dim=7),
    "opacity_only_colour_input_mismatch": _edit(points, _no_color, dims_c=[16, 32, 16]),
    "opacity_only_colour_offset": _edit(points, _no_color, lambda a: setattr(a.color, "offset", a.color.offset + 1)),
    "opacity_only_n_mlp_params_one_short": _edit(points, _no_color, lambda a: setattr(a, "n_mlp_params", a.n_mlp_params - 1)),
    "opacity_only_parameters_of_trunk_and_opacity": _edit(points, _no_color, ("n_mlp_params", numel(DIMS_T) + numel(DIMS_O)), dims_c=[]),
    **{f"{f}_null": _edit(points, (f, None), n_rays=3) for f in ("points", "grid_idx", "encoding")},
    "grid.data_null": _edit(points, ("grid.data", None), n_rays=3), "color_grid.data_null": _edit(points, ("color_grid.data", None), n_rays=3, **TWO_GRID),
    **{f"{f}_misaligned": _edit(points, (f, _p(45) + 4)) for f in ("points", "grid_idx", "encoding", "opacity_out", "grad_color", "grad_grid", "grad_points")},
    "scaffold_misaligned": _edit(points, ("scaffold", _p(8) + 4), scaffold=(2, 5, 4, 6)),
    "grad_color_grid_list[0]_misaligned": _edit(points, ("grad_color_grid_list[0]", _p(41) + 4), **TWO_GRID),
    "scaffold_extent_0": _edit(points, scaffold=(2, 5, 0, 6)), "scaffold_other_batch": _edit(points, scaffold=(3, 5, 4, 6)),
    **sampler_list_blocks(points), **decoder_blocks(points),
})
add("lp_points_forward/opacity_out_null", lambda: _points["lp_points_forward"](_edit(points, ("opacity_out", None), n_rays=3)()))
add("lp_points_backward/grad_grid_list_for_some_grids", lambda: _points["lp_points_backward"](_edit(points, ("grad_grid_list[1]", _p(41)))()))
add("lp_points_backward/layer_widths_over_1024",
    lambda: _points["lp_points_backward"](_edit(points, dims_t=[16] + [128] * 4, dims_o=[128] * 4 + [1], dims_c=[128] * 4 + [16])()))


# ---- gather / splat at points ----------------------------------------------------------------------------------------------------------
def point_grid(n_rays=0, n_pts=5, weights=3):
    a = _lib.LpPointGridArgs()
    a.grid = grid_list(TRIPLANE, 16, _p(6))
    for g in range(weights):
        a.row_weight[g] = _p(20 + g)
    a.points, a.grid_idx, a.vectors, a.out_features, a.grad_points = (_p(k) for k in range(5))
    a.n_rays, a.n_pts, a.channels = n_rays, n_pts, 16
    return a


_point_grid = {name: (lambda a, name=name: getattr(_L(), name)(_ref(a), None))
               for name in ("lp_point_gather", "lp_point_splat", "lp_point_normalize", "lp_point_grad_points")}
_fam(_point_grid, {
    "args_null": lambda: None, **_point_batch(point_grid), "channels_mismatch": _edit(point_grid, ("channels", 32)),
    "grid.data_null": _edit(point_grid, ("grid.data", None)),
    **{f"{f}_misaligned": _edit(point_grid, (f, _p(45) + 4)) for f in ("points", "grid_idx", "vectors", "out_features", "grad_points", "row_weight[2]")},
    **sampler_list_blocks(point_grid),
})
_fam({k: _point_grid[k] for k in ("lp_point_gather", "lp_point_splat", "lp_point_grad_points")},
     {f"{f}_null": _edit(point_grid, (f, None), n_rays=3) for f in ("points", "grid_idx")})
add("lp_point_gather/out_features_null", lambda: _point_grid["lp_point_gather"](_edit(point_grid, ("out_features", None), n_rays=3)()))
add("lp_point_splat/vectors_null", lambda: _point_grid["lp_point_splat"](_edit(point_grid, ("vectors", None), n_rays=3)()))
add("lp_point_grad_points/vectors_null", lambda: _point_grid["lp_point_grad_points"](_edit(point_grid, ("vectors", None), n_rays=3)()))
add("lp_point_grad_points/grad_points_null", lambda: _point_grid["lp_point_grad_points"](_edit(point_grid, ("grad_points", None), n_rays=3)()))
add("lp_point_splat/row_weight_for_some_grids", lambda: _point_grid["lp_point_splat"](point_grid(weights=2)))
add("lp_point_splat/no_row_weight", lambda: _point_grid["lp_point_splat"](point_grid(weights=0)))
add("lp_point_normalize/row_weight_for_some_grids", lambda: _point_grid["lp_point_normalize"](point_grid(weights=2)))


# ---- ray clipping ----------------------------------------------------------------------------------------------------------------------
def ray_clip(n_rays=0, scaffold=(2, 5, 4, 6), pad=0.0):
    a = _lib.LpRayClipArgs()
    r = a.rays
    r.n_rays = n_rays
    r.directions, r.origins, r.grid_idx, r.near_t, r.far_t = (_p(k) for k in range(5))
    if scaffold is not None:
        a.scaffold, a.scaffold_shape = _p(8), _lib.LpGrid(*scaffold, 0, None)
    a.pad = pad
    return a


def _clip(a, near=_p(10), far=_p(11), hit=_p(12)):
    return _L().lp_rays_clip(_ref(a), near, far, hit, None)


_fam({"lp_rays_clip": _clip}, {
    "args_null": lambda: None, "empty_batch": ray_clip, "empty_batch_without_scaffold": _edit(ray_clip, scaffold=None), "n_rays_-1": _edit(ray_clip, n_rays=-1),
    **{f"rays.{f}_null": _edit(ray_clip, (f"rays.{f}", None), n_rays=3) for f in ("directions", "origins", "grid_idx", "near_t", "far_t")},
    **{f"rays.{f}_misaligned": _edit(ray_clip, (f"rays.{f}", _p(45) + 4)) for f in ("directions", "far_t")},
    "rays.encoding_misaligned": _edit(ray_clip, ("rays.encoding", _p(45) + 4)),
    "scaffold_misaligned": _edit(ray_clip, ("scaffold", _p(8) + 4)),
    "pad_-1": _edit(ray_clip, pad=-1.0), "pad_inf": _edit(ray_clip, pad=INF), "pad_nan": _edit(ray_clip, pad=NAN),
    "scaffold_extent_0": _edit(ray_clip, scaffold=(2, 5, 0, 6)), "scaffold_batch_0": _edit(ray_clip, scaffold=(0, 5, 4, 6)),
    "scaffold_D+H+W_2^30": _edit(ray_clip, scaffold=(1, 1 << 29, 1 << 28, 1 << 28)),
})
for _name, _kw in {"near_out_null": dict(near=None), "far_out_null": dict(far=None), "hit_out_null": dict(hit=None),
                   "near_out_misaligned": dict(near=_p(10) + 4), "far_out_misaligned": dict(far=_p(11) + 4), "hit_out_unaligned": dict(hit=_p(12) + 1)}.items():
    add(f"lp_rays_clip/{_name}", lambda kw=_kw: _clip(ray_clip(), **kw))


# ---- occupancy scaffold ----------------------------------------------------------------------------------------------------------------
def scaffold(dims_t=DIMS_T, dims_o=DIMS_O, channels=16, shape=(2, 6, 5, 7), dilate=1, threshold=0.5):
    a = _lib.LpScaffoldArgs()
    a.grid = grid_list(TRIPLANE, channels, _p(6))
    a.mlp_params = _p(9)
    a.n_mlp_params = numel(dims_t) + numel(dims_o)
    a.trunk, a.opacity = _lib.make_mlp(dims_t, 0), _lib.make_mlp(dims_o, numel(dims_t))
    a.gain, a.shape, a.threshold, a.dilate = 1.0, _lib.LpGrid(*shape, 0, None), threshold, dilate
    return a


def _scaffold_build(a, out=FAR, ws=FAR + 0x10000000, ws_short=0):
    nbytes = max(int(_L().lp_scaffold_workspace_bytes(C.byref(a))), 0) - ws_short if a is not None else 0
    return _L().lp_scaffold_build(_ref(a), out, ws, nbytes, None)


_scaffold = {"lp_scaffold_opacity": lambda a: _L().lp_scaffold_opacity(_ref(a), FAR, None), "lp_scaffold_build": _scaffold_build}
_scaffold_shapes = {"args_null": lambda: None, "shape_extent_0": _edit(scaffold, shape=(2, 6, 0, 7)), "shape_batch_0": _edit(scaffold, shape=(0, 6, 5, 7)),
                    "dilate_-1": _edit(scaffold, dilate=-1)}
_fam({"lp_scaffold_workspace_bytes": lambda a: _L().lp_scaffold_workspace_bytes(_ref(a))},
     {**_scaffold_shapes, "dilate_1": scaffold, "dilate_0": _edit(scaffold, dilate=0)})
_fam(_scaffold, {
    **_scaffold_shapes, "shape_other_batch": _edit(scaffold, shape=(3, 6, 5, 7)), "threshold_nan": _edit(scaffold, threshold=NAN),
    "grid.data_null": _edit(scaffold, ("grid.data", None)),
    **{k: v for k, v in sampler_list_blocks(scaffold).items() if not k.endswith("ends_at_2^31")},   # (a scaffold has no empty batch)
    **{k: v for k, v in decoder_blocks(scaffold, color=False).items() if k != "n_mlp_params_one_more"},   # (parameters suffice: not refused)
})
add("lp_scaffold_opacity/result_null", lambda: _L().lp_scaffold_opacity(C.byref(scaffold()), None, None))
add("lp_scaffold_opacity/result_misaligned", lambda: _L().lp_scaffold_opacity(C.byref(scaffold()), FAR + 4, None))
for _name, _kw in {"result_null": dict(out=None), "result_misaligned": dict(out=FAR + 4), "workspace_null": dict(ws=None),
                   "workspace_one_byte_short": dict(ws_short=1), "workspace_misaligned": dict(ws=FAR + 0x10000000 + 4),
                   "workspace_overlaps_the_result": dict(ws=FAR + 64)}.items():
    add(f"lp_scaffold_build/{_name}", lambda kw=_kw: _scaffold_build(scaffold(), **kw))
add("lp_scaffold_build/no_dilation_result_null", lambda: _scaffold_build(scaffold(dilate=0), out=None, ws=None))


# ---- mesh extraction -------------------------------------------------------------------------------------------------------------------
def mesh(shape=(2, 5, 6, 7)):
    a = _lib.LpMeshArgs()
    a.volume, a.shape, a.level = _p(0), _lib.LpGrid(*shape, 0, None), 0.5
    a.vertex_offsets, a.face_offsets, a.vertices, a.faces, a.normals = (_p(k) for k in range(1, 6))
    a.max_vertices, a.max_faces = 10, 10
    return a


def _mesh_call(name, a, ws=_p(6), ws_short=0):
    nbytes = max(int(_L().lp_mesh_workspace_bytes(C.byref(a))), 0) - ws_short if a is not None else 0
    return getattr(_L(), name)(_ref(a), ws, nbytes, None)


_mesh = {name: (lambda a, name=name, **kw: _mesh_call(name, a, **kw)) for name in ("lp_mesh_count", "lp_mesh_emit")}
_mesh_shapes = {"args_null": lambda: None, "shape_extent_0": _edit(mesh, shape=(2, 5, 0, 7)), "shape_batch_0": _edit(mesh, shape=(0, 5, 6, 7)),
                "shape_of_2^31_points": _edit(mesh, shape=(2, 1024, 1024, 1024))}
_fam({"lp_mesh_workspace_bytes": lambda a: _L().lp_mesh_workspace_bytes(_ref(a))}, {**_mesh_shapes, "lattice": mesh})
_fam(_mesh, {**_mesh_shapes, **{f"{f}_null": _edit(mesh, (f, None)) for f in ("volume", "vertex_offsets", "face_offsets")},
             **{f"{f}_misaligned": _edit(mesh, (f, _p(45) + 4)) for f in ("volume", "vertex_offsets", "face_offsets", "vertices", "faces", "normals")}})
for _name in _mesh:
    for _b, _kw in {"workspace_null": dict(ws=None), "workspace_one_byte_short": dict(ws_short=1), "workspace_misaligned": dict(ws=_p(6) + 4)}.items():
        add(f"{_name}/{_b}", lambda name=_name, kw=_kw: _mesh_call(name, mesh(), **kw))
_fam({"lp_mesh_emit": _mesh["lp_mesh_emit"]}, {"max_vertices_-1": _edit(mesh, ("max_vertices", -1)), "max_faces_-1": _edit(mesh, ("max_faces", -1)),
                                               "vertices_null": _edit(mesh, ("vertices", None)), "faces_null": _edit(mesh, ("faces", None))})

#: every function of the ABI that can answer with an error code (lp_version, lp_last_error, lp_build_info, lp_abi_sizeof and the debug
#: hook cannot: they have no argument to refuse, or -- lp_abi_sizeof -- answer -1 without a message)
ENTRY_POINTS = (
    "lp_renderer_forward", "lp_renderer_forward_ws", "lp_renderer_backward", "lp_renderer_corner_rows", "lp_renderer_kernel_family",
    "lp_renderer_forward_family", "lp_renderer_forward_workspace_bytes", "lp_renderer_backward_segments", "lp_renderer_relu_dump_words",
    "lp_renderer_backward_relu_dump", "lp_splatter_forward", "lp_splatter_backward", "lp_splatter_normalize", "lp_splatter_kernel_family",
    "lp_mlp_splatter_relu_dump_words", "lp_mlp_splatter_backward_relu_dump", "lp_mlp_splatter_launch_shape", "lp_ray_embedding_forward",
    "lp_ray_embedding_backward", "lp_hash_randn", "lp_grid_tv_workspace_bytes", "lp_grid_tv_forward", "lp_grid_tv_backward", "lp_grid_tv_fused",
    "lp_grid_resample_forward", "lp_grid_resample_backward", "lp_points_forward", "lp_points_backward", "lp_point_gather", "lp_point_splat",
    "lp_point_normalize", "lp_point_grad_points", "lp_rays_clip", "lp_scaffold_workspace_bytes", "lp_scaffold_opacity", "lp_scaffold_build",
    "lp_mesh_workspace_bytes", "lp_mesh_count", "lp_mesh_emit",
)


def entry_point(cid):
    return cid.split("/")[0].split("[")[0]


#: the entry points that only answer a question: they launch nothing, and a positive answer is a value (bytes, a family, a count)
QUERIES = tuple(n for n in ENTRY_POINTS if n.endswith(("_workspace_bytes", "_family", "_segments", "_dump_words", "_launch_shape")))
