"""What the Python device layer hands to the library, checked without a GPU: :mod:`device_call_cases` drives every public
method of the five classes of :mod:`multimesh_amd.device` against a recording stand-in library, and the record must equal
``tests/golden/device_calls.json`` entry for entry.  The fixture was written by ``python tests/device_call_cases.py
--write`` from the package as it stood before the layer was given one call path (commit 2aa9ba1), and is not to be
regenerated from the code it checks.  Also here: the signature of every public method of those classes."""
import glob
import inspect
import json
import os
import re

import pytest

import device_call_cases as DC
from multimesh_amd import helpers

# symbol -> why no case reaches it; neither device.py nor the api package calls any of these
NOT_DRIVEN = {
    "centroid": "legacy host-array symbol of the reference's loader: the mesh objects (mesh.py, io.py) call it, not this layer",
    "triLinearInterpolator": "legacy host-array symbol of the reference's loader, declared for drop-in callers",
    "mm_device_count": "takes no context: tests and tools call it on the library itself",
    "mm_last_status": "takes no context: read by the mesh objects after the legacy centroid",
}

# Class.method -> str(inspect.signature(...)); written out once, not derived from the package
SIGNATURES = {
    "Context.arg_extreme": '(self, values, want_max=False)',
    "Context.asdevice": '(self, x, dtype)',
    "Context.binned_weighted_sum": '(self, mass, bins, nbins, fields=None, square=False, want_count=False)',
    "Context.boundary_classify": '(self, corners, faces, up=None, cos_min=0.5)',
    "Context.boundary_faces": '(self, corner_ids, nnodes)',
    "Context.boundary_nodes": '(self, points, shape_order, faces, side=None, side_mask=7)',
    "Context.centroid": '(self, connectivity, points)',
    "Context.clamp": '(self, values, lower=None, upper=None, symmetric=False, out=None, want_count=True)',
    "Context.close": '(self)',
    "Context.cutoff_distance": '(self, points, sources, cutoff)',
    "Context.diffusion": '(self, shape_order, gll_points, kappa_h=1.0, kappa_r=None)',
    "Context.distance_taper": '(self, dist, inner, outer, a, b=None, elem=None, out=None, want_weight=False)',
    "Context.divide_rows": '(self, num, den, out=None)',
    "Context.element_deviation": '(self, a, b)',
    "Context.empty": '(self, shape, dtype)',
    "Context.first_occurrence": '(self, connectivity, nnodes)',
    "Context.fluid_solid_fix": '(self, values, previous, solid, vs_index)',
    "Context.fp_mode": '(self)',
    "Context.gather": '(self, fields, ids, weights, point_major=True)',
    "Context.gather_elem": '(self, element_nodal_fields, elem, coeffs, point_major=True)',
    "Context.gll_gradient": '(self, shape_order, gll_points, u, grad=True, radial=False, lateral=False, norm=False)',
    "Context.gll_mass": '(self, shape_order, gll_points, want_det=False)',
    "Context.gll_resolution": '(self, shape_order, gll_points, fast=None, slow=None, want_node_spacing=False)',
    "Context.gll_tensor_apply": '(self, order_in, order_out, dim, values, layout=0, transpose=False, scale_in=None, div_out=None, out=None)',
    "Context.grid_operator": '(self, points, depth, lat, lon, clamp=False, lon_periodic=False, latlondepth=False, ids_out=None, weights_out=None)',
    "Context.idw_gather": "(self, fields, idx, dist, power=2, max_distance=inf, outside='fill', fill_value=nan, out=None, point_major=False, want_nearest=False, want_count=False)",
    "Context.interpolate_gll": '(self, shape_order, gll_points, points, element_nodal_fields, nelem_to_search=20, tolerance=1.05, snap_to_nearest=False, want_operator=False, out=None)',
    "Context.interpolate_hex8": '(self, nodes, connectivity, points, fields, nelem_to_search=20, want_operator=False, out=None)',
    "Context.interpolate_hex8_host": '(self, nodes, connectivity, points, fields, nelem_to_search=20, want_operator=False, out=None)',
    "Context.knn_build": '(self, sources)',
    "Context.last_knn_kernels": '(self)',
    "Context.last_locate_stats": '(self)',
    "Context.last_timings": '(self)',
    "Context.locate_gll": '(self, shape_order, nearest_element_indices, gll_points, points, tolerance=1.05, snap_to_nearest=False)',
    "Context.locate_gll_bbox": '(self, shape_order, nearest_element_indices, gll_points, points)',
    "Context.locate_hex8": '(self, nearest_element_indices, connectivity, nodes, points, enc=None, weights=None, conn_is_exodus=False)',
    "Context.map_to_sphere": '(self, points, rad, connectivity=None, out=None, r_ref=6371000.0, first=None)',
    "Context.multiply_rows": '(self, mass, values)',        # (added with the one call path: api.grids called the library itself)
    "Context.order_statistics": "(self, values, q, absolute=False, method='lower')",
    "Context.point_taper": '(self, points, centres, inner, outer, values_in=None, out=None, want_weight=False)',
    "Context.points_to_elements": '(self, indices, nodes_per_element)',     # (likewise, for api.gll)
    "Context.radial_bins": '(self, points, edges, want_radius=False)',
    "Context.radial_model_apply": '(self, points, radius, values, mode=0, values_in=None, out=None)',
    "Context.sample_columns_gll": '(self, shape_order, gll_points, element_nodal_fields, lat_table, lon_table, radius, paired=False, nelem_to_search=25, tolerance=1.05, fill_value=nan, chunk_points=None, want_points=False, out=None)',
    "Context.sample_grid": "(self, points, grid_values, depth, lat, lon, outside='fill', fill_value=nan, lon_periodic=False, out=None, want_latlondepth=False)",
    "Context.scale_points": '(self, points, factor, out=None)',
    "Context.scatter_elements": '(self, values, inverse, elem_ids, out)',
    "Context.set_fp_mode": '(self, mode)',
    "Context.set_lazy_lists": '(self, on=True)',
    "Context.set_profiling": '(self, on=True)',
    "Context.source": '(self, nodes, connectivity)',
    "Context.sphere_ratio": '(self, points, rad, connectivity=None, r_ref=6371000.0, first=None)',
    "Context.synchronize": '(self)',
    "Context.to_device": '(self, array, dtype=None)',
    "Context.transpose_elem": '(self, elem, coeffs, nelem)',
    "Context.transpose_nodes": '(self, ids, weights, nsrc)',
    "Context.unique_points": '(self, points, unique_out=None, inverse_out=None, ordered=True)',
    "Context.weighted_sum": '(self, mass, fields=None)',
    "Context.zeros": '(self, shape, dtype)',
    "KnnIndex.free": '(self)',
    "KnnIndex.query": '(self, points, k, want_dist=False)',
    "Source.free": '(self)',
    "Source.interpolate": '(self, points, fields, nelem_to_search=20, want_operator=False, out=None)',
    "TransposedOperator.apply": '(self, values, point_major=True, out=None)',
    "TransposedOperator.free": '(self)',
    "Diffusion.apply": '(self, u, out=None)',
    "Diffusion.free": '(self)',
    "Diffusion.roughness": '(self, u)',
    "Diffusion.smooth": '(self, values, steps=4, rtol=1e-10, max_iter=2000)',
}


@pytest.fixture(scope="module")
def record():
    return DC.drive()


@pytest.fixture(scope="module")
def fixture():
    with open(DC.FIXTURE) as fh:
        return json.load(fh)


def test_the_layer_passes_what_it_passed_before(record, fixture):
    assert list(record) == list(fixture)
    for name, expected in fixture.items():
        got = json.loads(json.dumps(record[name]))
        assert got.get("raises") == expected.get("raises"), name
        assert len(got["log"]) == len(expected["log"]), name
        for i, (a, b) in enumerate(zip(got["log"], expected["log"])):
            assert a == b, f"{name}: call {i}"
        assert got.get("returns") == expected.get("returns"), name


def test_every_symbol_of_the_table_is_driven(record):
    driven = {entry[0] for case in record.values() for entry in case["log"]}
    assert not set(NOT_DRIVEN) & driven
    assert sorted(set(helpers.SIGNATURES) - driven) == sorted(NOT_DRIVEN)
    package = os.path.dirname(helpers.__file__)
    sources = {p: open(p).read() for p in [os.path.join(package, "device.py")] + glob.glob(os.path.join(package, "api", "*.py"))}
    assert len(sources) > 10
    for symbol in NOT_DRIVEN:              # (only symbols that neither device.py nor the api package calls may be left out)
        for path, text in sources.items():
            assert not re.search(rf"lib\.{symbol}\b|[\"']{symbol}[\"']", text), (symbol, path)


def test_a_refused_argument_is_the_callers_mistake_where_it_was(record):
    """Status -1 is a ``ValueError`` with the library's text from the methods that said so before, and a
    ``MultiMeshHipError`` naming the symbol from the others."""
    refused = {name: case["raises"] for name, case in record.items() if name.endswith(".refused")}
    assert sorted(n.split(".")[0] for n in refused) == sorted(
        ["radial_bins", "radial_model_apply", "point_taper", "order_statistics", "clamp", "boundary_faces",
         "boundary_classify", "boundary_nodes", "cutoff_distance", "distance_taper", "idw_gather", "gll_resolution",
         "arg_extreme", "first_occurrence"])
    for name, raised in refused.items():
        assert raised == ["ValueError", DC.LAST_ERROR.decode()], name
    failed = {name: case["raises"] for name, case in record.items() if name.endswith(".fails")}
    assert len(failed) >= 1
    for name, (cls, message) in failed.items():
        assert cls == "MultiMeshHipError" and re.fullmatch(rf"mm_\w+ failed with code -1: {DC.LAST_ERROR.decode()}", message), name


def test_every_public_method_keeps_its_signature():
    assert DC.signatures() == SIGNATURES
