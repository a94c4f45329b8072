"""Drop-in for the entry points of reference ``multi_mesh/api.py`` and the hot-path command of ``scripts/cli.py``: their
names, arguments and return conventions, every function ending in HIP kernels (no CPU fallback).  One module per subject."""
from ..mesh import HexMesh  # (HexMesh, _sphere_mapped and _change_order_plan: not public, reachable here as before)
from ._common import GllMesh, R_EARTH, TTI_PARAMS, latlondepth_to_xyz
from .hex8 import (apply_gll_operator_transpose, apply_operator, apply_operator_transpose, interpolate_cached,
                   interpolate_mesh_a_to_b, interpolate_operator, interpolate_to_mesh, interpolate_to_points,
                   load_stored_operator, save_stored_operator)
from .earth import _sphere_mapped, map_to_ellipse, map_to_sphere
from .gll import (check_if_inside_element, find_gll_centroids, get_element_weights, get_unique_points,
                  interpolate_gll_to_gll, interpolate_gll_to_nodes, interpolate_gll_to_points, interpolate_hex8_to_gll,
                  query_gll_model)
from .mass import (apply_gll_operator_adjoint, apply_operator_adjoint, assemble_gll, gll_mass_matrix, gll_quadrature,
                   hex8_mass_matrix, integrate)
from .smooth import gll_gradient, gll_gradient_parts, gll_roughness, gll_stiffness_apply, smooth_gll
from .order import (_change_order_plan, gll_change_order, gll_order_apply, gll_order_table, resample_gll_order,
                    restrict_gll_kernel)
from .layers import (assess_layers, fix_fluid_solid, interpolate_gll_to_gll_layered, load_stored_layer_operator,
                     save_stored_layer_operator)
from .drivers import (exodus_2_gll, gll_2_exodus, gll_2_gll, gll_2_gll_layered, gll_2_gll_layered_multi,
                      gll_2_gll_layered_multi_two, query_model)
from .grids import (DIMS, GridOperator, RegularGrid, UNITS, column_tables, extract_cross_section, extract_depth_slice,
                    extract_regular_grid, fold_to_caller_layout, grid_import_operator, import_regular_grid,
                    prepare_regular_grid, regular_grid_adjoint, sample_regular_grid, to_prepared_layout)
# (the grid operator and its adjoint -- GridOperator, grid_import_operator, regular_grid_adjoint and the two layout
# functions -- are reachable as api.<name>; __all__ stays the drop-in surface that tests/test_api_surface.py pins)
from .radial import (RadialModel, RadialProfile, evaluate_radial_model, from_perturbation, radial_edges, radial_profile,
                     to_perturbation)

__all__ = ["DIMS", "GllMesh", "R_EARTH", "RadialModel", "RadialProfile", "RegularGrid", "TTI_PARAMS", "UNITS",
           "apply_gll_operator_adjoint", "apply_gll_operator_transpose", "apply_operator", "apply_operator_adjoint",
           "apply_operator_transpose", "assemble_gll", "assess_layers", "check_if_inside_element", "column_tables",
           "evaluate_radial_model", "exodus_2_gll", "extract_cross_section", "extract_depth_slice",
           "extract_regular_grid", "find_gll_centroids", "fix_fluid_solid", "from_perturbation", "get_element_weights",
           "get_unique_points", "gll_2_exodus", "gll_2_gll", "gll_2_gll_layered", "gll_2_gll_layered_multi",
           "gll_2_gll_layered_multi_two", "gll_change_order", "gll_gradient", "gll_gradient_parts", "gll_mass_matrix",
           "gll_order_apply", "gll_order_table", "gll_quadrature", "gll_roughness", "gll_stiffness_apply",
           "hex8_mass_matrix", "import_regular_grid", "integrate", "interpolate_cached", "interpolate_gll_to_gll",
           "interpolate_gll_to_gll_layered", "interpolate_gll_to_nodes", "interpolate_gll_to_points",
           "interpolate_hex8_to_gll", "interpolate_mesh_a_to_b", "interpolate_operator", "interpolate_to_mesh",
           "interpolate_to_points", "latlondepth_to_xyz", "load_stored_layer_operator", "load_stored_operator",
           "map_to_ellipse", "map_to_sphere", "prepare_regular_grid", "query_gll_model", "query_model", "radial_edges",
           "radial_profile", "resample_gll_order", "restrict_gll_kernel", "sample_regular_grid",
           "save_stored_layer_operator", "save_stored_operator", "smooth_gll", "to_perturbation"]
