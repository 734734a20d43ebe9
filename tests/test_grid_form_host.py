"""``grids.GridForm``: the one reading of a grid-list argument behind every Python front-end (no GPU, no library: shapes and
``data_ptr`` only).

Two policies.  ``sampler=True`` is what the Renderer and the Splatter accept (``make_grid_descs``: one batch size, voxel grids and
planes); ``sampler=False`` is what the regularisers, the resampling, the point ops and the scaffold accept (any positive extents,
differing batch sizes, 1 to LP_MAX_GRIDS grids).  The exception types and messages below are those of the code the front-ends ran
before they shared ``GridForm`` (``renderer._render`` for the strict policy, ``regularizers._normalize`` for the lax one)."""
import pytest
import torch

from lightplane_amd import _lib, grids
from lightplane_amd.grids import GridDesc, GridForm

C = 4
VOXEL, PLANE, LINE = (2, 3, 4, 5, C), (2, 1, 4, 5, C), (2, 1, 1, 7, C)
FEATURE_DIMS = "All grids should have the same feature dimensions."


def _list(*sizes):
    return [torch.zeros(s) for s in sizes]


def _flat(*sizes):
    return torch.zeros(sum(s[0] * s[1] * s[2] * s[3] for s in sizes), sizes[0][4]), [list(s) for s in sizes]


def _raises(exc, message, grid, sizes, sampler):
    with pytest.raises(exc) as e:
        GridForm.of(grid, sizes, name="grid", sampler=sampler)
    assert type(e.value) is exc and str(e.value) == message, (type(e.value), str(e.value))


@pytest.mark.parametrize("sampler", [True, False])
def test_both_policies_read_a_valid_argument_alike(sampler):
    tensors, form = GridForm.of(_list(VOXEL, PLANE), sampler=sampler)
    assert form == GridForm(True, (GridDesc(2, 3, 4, 5, 0), GridDesc(2, 1, 4, 5, 120)), C, 160)
    assert form.n_tensors == len(tensors) == 2 and all(torch.is_tensor(t) for t in tensors)
    assert form.sizes() == [list(VOXEL), list(PLANE)] and form.out_shapes() == [VOXEL, PLANE]
    flat, sizes = _flat(VOXEL, PLANE)
    tensors, flat_form = GridForm.of(flat, sizes, sampler=sampler)
    assert tensors == (flat,) and flat_form == form._replace(is_list=False)
    assert flat_form.n_tensors == 1 and flat_form.sizes() == form.sizes() and flat_form.out_shapes() == [(160, C)]
    assert GridForm.of_sizes(torch.tensor(sizes), sampler=sampler) == flat_form
    assert GridForm.of_sizes(sizes, sampler=sampler, is_list=True) == form
    descs, channels, rows = grids.make_grid_descs(sizes)
    assert (tuple(descs), channels, rows) == (form.descs, form.channels, form.rows) and isinstance(descs, list)


@pytest.mark.parametrize("sampler", [True, False])
def test_refusals_both_policies_share(sampler):
    _raises(AssertionError, FEATURE_DIMS, _list(VOXEL, (2, 1, 4, 5, C + 1)), None, sampler)
    flat, sizes = _flat(VOXEL, PLANE)
    _raises(AssertionError, "grid_sizes has to be compatible to grid tensor shapes!", flat[:-1], sizes, sampler)  # a row short
    _raises(AssertionError, "flat grid tensor does not match grid_sizes", flat.t().contiguous(), sizes, sampler)  # [C, rows]
    _raises(AssertionError, "grid_sizes cannot be None when grid is a tensor", flat, None, sampler)
    _raises(NotImplementedError, "grid should be either tensor or list", tuple(_list(VOXEL)), None, sampler)
    _raises(NotImplementedError, "grid should be either tensor or list", None, None, sampler)


def test_the_policies_differ_on_batch_sizes_lines_and_the_grid_count():
    other_batch = _list(VOXEL, (3, 1, 4, 5, C))
    _raises(AssertionError, "All grids should have the same batch size.", other_batch, None, True)
    assert [d.B for d in GridForm.of(other_batch, sampler=False)[1].descs] == [2, 3]
    _raises(ValueError, "Unexpected n non-singular dim of input grid (1); only voxel grids [B,D,H,W,C] and planes with one singleton "
            "dim are supported", _list(LINE), None, True)
    assert GridForm.of(_list(LINE), sampler=False)[1].rows == 14
    flat, sizes = _flat(LINE)
    assert GridForm.of(flat, sizes, sampler=False)[1].rows == 14
    _raises(AssertionError, "grid size [2, 0, 4, 5, 4] has an empty dimension", _list((2, 0, 4, 5, C)), None, False)
    # the strict policy leaves the count to the one place that writes an LpGridList, the lax one checks it up front
    nine = _list(*[PLANE] * 9)
    _raises(AssertionError, f"a grid-list holds 1 to {_lib.LP_MAX_GRIDS} grids", nine, None, False)
    tensors, form = GridForm.of(nine, sampler=True)
    with pytest.raises(AssertionError, match=f"^at most {_lib.LP_MAX_GRIDS} grids per grid-list are supported$"):
        form.abi(tensors)
    _raises(AssertionError, f"a grid-list holds 1 to {_lib.LP_MAX_GRIDS} grids", [], None, False)
    # an entry that is no [B, D, H, W, C] tensor: each policy keeps the words of its front-ends
    _raises(AssertionError, "every grid of a grid-list has to be [B, D, H, W, C]", [torch.zeros(2, 4, 5, C)], None, True)
    with pytest.raises(AssertionError, match=r"^every entry of a feature_grid list has to be a \[B, D, H, W, C\] tensor$"):
        GridForm.of([torch.zeros(2, 4, 5, C)], name="feature_grid", sampler=False)
    flat, sizes = _flat(VOXEL)
    with pytest.raises(AssertionError, match="^flat input grid tensor does not match input_grid_sizes$"):
        GridForm.of(flat.t().contiguous(), sizes, name="input grid", sampler=True, sizes_name="input_grid_sizes")


@pytest.mark.parametrize("sampler", [True, False])
def test_abi_writes_what_make_grid_list_writes(sampler):
    tensors, form = GridForm.of(_list(VOXEL, PLANE, (2, 3, 1, 5, C)), sampler=sampler)
    descs = [GridDesc(2, 3, 4, 5, 0), GridDesc(2, 1, 4, 5, 120), GridDesc(2, 3, 1, 5, 160)]
    assert bytes(form.abi(tensors)) == bytes(_lib.make_grid_list(list(tensors), descs, C, 190))
    assert [form.abi(tensors).grids[i].data for i in range(3)] == [t.data_ptr() for t in tensors]
    assert bytes(form.abi()) == bytes(form.abi(None)) == bytes(_lib.make_grid_list(None, descs, C, 190))
    flat, sizes = _flat(VOXEL, PLANE, (2, 3, 1, 5, C))
    tensors, form = GridForm.of(flat, sizes, sampler=sampler)
    assert bytes(form.abi(tensors)) == bytes(_lib.make_grid_list(flat, descs, C, 190))
    assert form.abi(tensors).data == flat.data_ptr() and form.abi(tensors).grids[2].row_offset == 160
    # gradients and fresh results of a form go through the same call
    twins = [torch.zeros(s) for s in form.out_shapes()]
    assert bytes(form.abi(twins)) == bytes(_lib.make_grid_list(twins[0], descs, C, 190))
