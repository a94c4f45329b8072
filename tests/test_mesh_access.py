"""How the model tools read and write a mesh's nodes and fields (multimesh_amd/api/_common.py), on the smallest meshes that
still tell the kinds apart: two-element GLL meshes of order 1 and 2, two hexahedra sharing a face, and an in-memory Salvus
model with three labelled columns of which two are imported.  No device is needed."""
import numpy as np
import pytest

from multimesh_amd import io as mio, synth
from multimesh_amd.api import GllMesh
from multimesh_amd.api import _common as M
from multimesh_amd.mesh import HexMesh

LABELS = ["VP", "KEPT", "VS"]      # the imports name VP and VS; KEPT must come through untouched


def _gll(order):
    gp = synth.gll_mesh(3, order)[:2]
    rng = np.random.default_rng(order)
    return GllMesh(gp, order, {"VP": rng.normal(size=gp.shape[:2]), "VS": rng.normal(size=gp.shape[:2])})


def _hex():
    """x in {0, 1, 2}, y and z in {0, 1}: node i + 3 (j + 2 k); the two elements share the face x = 1."""
    pts = np.array([[i, j, k] for k in range(2) for j in range(2) for i in range(3)], dtype=np.float64)
    node = lambda i, j, k: i + 3 * (j + 2 * k)   # noqa: E731
    conn = [[node(e, 0, 0), node(e + 1, 0, 0), node(e + 1, 1, 0), node(e, 1, 0),
             node(e, 0, 1), node(e + 1, 0, 1), node(e + 1, 1, 1), node(e, 1, 1)] for e in range(2)]
    rng = np.random.default_rng(7)
    return HexMesh(pts, conn, {"VP": rng.normal(size=12), "VS": rng.normal(size=12)})


def _model(order=1):
    gp = synth.gll_mesh(3, order)[:2]
    data = np.random.default_rng(3).normal(size=(2, 3, gp.shape[1]))
    data[1, 1, 3] = np.nan
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=data), LABELS)
    return f, gp, data


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _kinds():
    return [("gll1", _gll(1)), ("gll2", _gll(2)), ("hex8", _hex())]


def test_name_list():
    assert M.name_list(None, ("A", "B")) == ["A", "B"]
    assert M.name_list(None, {"A": 1}) == ["A"]
    assert M.name_list("VP", ("A",)) == ["VP"]
    assert M.name_list(("VP", "VS"), ()) == ["VP", "VS"]
    given = ["VS"]
    assert M.name_list(given, ()) == given and M.name_list(given, ()) is not given


def test_is_mesh_and_points_of():
    f, gp, _ = _model()

    class Nodes:      # an object with points + connectivity, as map_to_sphere takes
        points, connectivity = np.zeros((4, 3)), np.zeros((1, 4), np.int64)

    fast, full = mio.SalvusMesh(f, fast_mode=True), mio.SalvusMesh(f, fast_mode=False)
    assert not hasattr(fast, "element_nodal_fields")
    for mesh in (_gll(1), _gll(2), _hex(), fast, full, Nodes()):
        assert M.is_mesh(mesh)
    assert not M.is_mesh(gp) and not M.is_mesh([[0.0, 0.0, 0.0]]) and not M.is_mesh(f)
    for mesh in (fast, full):
        assert _same_bits(M.points_of(mesh), gp)
    hexm = _hex()
    assert M.points_of(hexm).shape == (12, 3) and _same_bits(M.points_of(hexm), hexm.points)
    assert _same_bits(M.points_of(_gll(2)), synth.gll_mesh(3, 2)[:2])
    strided = np.arange(24.0).reshape(4, 6)[:, ::2]
    assert M.points_of(strided).flags.c_contiguous and np.array_equal(M.points_of(strided), strided)


@pytest.mark.parametrize("kind, mesh", _kinds())
def test_named_fields_and_the_missing_field_error(kind, mesh):
    lead = M.points_of(mesh).shape[:-1]
    store = mesh.nodal_fields if kind == "hex8" else mesh.element_nodal_fields
    names, fields = M.named_fields(mesh)
    assert names == ["VP", "VS"] and fields.shape == (2,) + lead and fields.flags.c_contiguous
    assert _same_bits(fields[0], store["VP"]) and _same_bits(fields[1], store["VS"])
    names, fields = M.named_fields(mesh, "VS")
    assert names == ["VS"] and _same_bits(fields[0], store["VS"])
    names, fields = M.named_fields(mesh, None, default=())
    assert names == [] and fields.shape == (0,) + lead
    with pytest.raises(ValueError, match="has no field") as err:
        M.named_fields(mesh, ["RHO", "VP", "QMU"])
    assert str(err.value).endswith("['RHO', 'QMU']")         # exactly the missing ones, in the order asked


def test_a_salvus_mesh_read_without_fields_has_none():
    fast = mio.SalvusMesh(_model()[0], fast_mode=True)
    assert M.named_fields(fast)[0] == []
    with pytest.raises(ValueError, match=r"has no field \['VP'\]"):
        M.named_fields(fast, "VP")


def test_hex8_corners():
    mesh = _hex()
    conn, corners = M.hex8_corners(mesh)
    assert M.EXODUS_TO_TENSOR == [0, 1, 3, 2, 4, 5, 7, 6]
    assert np.array_equal(conn, mesh.connectivity[:, M.EXODUS_TO_TENSOR]) and conn.flags.c_contiguous
    assert corners.shape == (2, 8, 3) and _same_bits(corners, mesh.points[mesh.connectivity[:, M.EXODUS_TO_TENSOR]])
    # tensor order: corner i + 2 j + 4 k of the unit cubes
    assert np.array_equal(corners[1] - corners[1][0], [[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)])
    assert len(set(conn[0]) & set(conn[1])) == 4
    with pytest.raises(ValueError, match="3-D hexahedral"):
        M.hex8_corners(HexMesh(*synth.quad_mesh(3)))


@pytest.mark.parametrize("kind, mesh", _kinds())
def test_import_target_on_a_mesh(kind, mesh):
    store = mesh.nodal_fields if kind == "hex8" else mesh.element_nodal_fields
    before = {p: v.copy() for p, v in store.items()}
    with M.ImportTarget(mesh) as target:
        assert _same_bits(target.points, M.points_of(mesh)) and target.lead == target.points.shape[:-1]
        target.require(["VP", "RHO"])                        # fields are created: nothing is required of them
        with pytest.raises(ValueError, match="no field") as err:
            target.require(["VP", "RHO", "VS", "ETA"], values=True)
        assert str(err.value).endswith("['RHO', 'ETA']")
        prior = target.existing(["VS", "VP"])
        assert prior.shape == (2,) + target.lead and _same_bits(prior[0], before["VS"]) and _same_bits(prior[1], before["VP"])
        assert target.existing([]).shape == (0,) + target.lead
        assert target.sphere_mesh() is mesh
        new = np.arange(2.0 * np.prod(target.lead)).reshape((2,) + target.lead)
        target.write(["RHO", "VP"], new)
    assert list(store) == ["VP", "VS", "RHO"]
    assert _same_bits(store["RHO"], new[0]) and _same_bits(store["VP"], new[1]) and _same_bits(store["VS"], before["VS"])
    assert all(v.flags.c_contiguous and v.dtype == np.float64 for v in store.values())


@pytest.mark.parametrize("order", [1, 2])
def test_import_target_on_a_model_file(order):
    f, gp, data = _model(order)
    with M.ImportTarget(f) as target:
        assert _same_bits(target.points, gp) and target.lead == gp.shape[:2]
        with pytest.raises(ValueError, match="not in MODEL/data") as err:
            target.require(["VP", "RHO", "VS", "ETA"])
        assert "['RHO', 'ETA'] are not" in str(err.value)
        target.require(["VP", "VS"], values=True)
        prior = target.existing(["VS", "VP"])
        assert prior.shape == (2,) + gp.shape[:2] and _same_bits(prior[0], data[:, 2]) and _same_bits(prior[1], data[:, 0])
        with pytest.raises(ValueError, match="z_node_1D"):
            target.sphere_mesh()
        new = np.arange(2.0 * gp.shape[0] * gp.shape[1]).reshape((2,) + gp.shape[:2])
        target.write(["VS", "VP"], new)
    after = f["MODEL/data"][()]
    assert _same_bits(after[:, 2], new[0]) and _same_bits(after[:, 0], new[1])
    assert np.isnan(after[1, 1, 3]) and _same_bits(after[:, 1], data[:, 1])     # the NaN included, bit for bit
    assert mio.dimension_labels(f["MODEL/data"], 1) == LABELS


def test_a_failed_requirement_leaves_the_file_as_it_was():
    f, _, data = _model()

    def an_import(names):
        with M.ImportTarget(f) as target:
            target.require(names)
            target.write(names, np.zeros((len(names),) + target.lead))

    with pytest.raises(ValueError, match="not in MODEL/data"):
        an_import(["VP", "RHO"])
    assert _same_bits(f["MODEL/data"][()], data)
    an_import(["VP"])
    assert not f["MODEL/data"][()][:, 0].any() and _same_bits(f["MODEL/data"][()][:, 1:], data[:, 1:])


def test_the_sphere_mesh_of_a_model_file_carries_its_z_node_1d():
    gp = synth.gll_mesh(3, 2)[:2]
    data = np.random.default_rng(5).normal(size=(2, 2, 27))
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=data), ["VP", "z_node_1D"])
    with M.ImportTarget(f) as target:
        mesh = target.sphere_mesh()
    assert isinstance(mesh, GllMesh) and mesh.shape_order == 2 and _same_bits(mesh.gll_points, gp)
    assert list(mesh.element_nodal_fields) == ["z_node_1D"] and _same_bits(mesh.element_nodal_fields["z_node_1D"], data[:, 1])
