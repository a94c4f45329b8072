"""Which layers of a mesh a request selects, the stored per-layer operator, the layered core, the fluid/solid fix-up."""
from __future__ import annotations

import os

import numpy as np

from ..device import default_context
from ._common import GllMesh


def assess_layers(layer_ids, layers, fluid=None, moho_idx=None):
    """The reference's ``utils._assess_layers`` (utils.py:382-440) on arrays: ``layer_ids`` = the mesh's
    ``layer`` elemental field; ``layers`` = "all", a list of layer numbers (which must lie within the mesh's
    own), one layer number, or an Earth preset.  The mesh's layers are sorted in DESCENDING order, "outwards from
    the core" reversed, as the reference sorts them (:396); with ``o_core_idx`` = the place in that order of the
    layer of the first fluid element (:426-429):

        "crust"  -> layers[:moho_idx]            "mantle" -> layers[moho_idx:o_core_idx]
        "core"   -> layers[o_core_idx:]          "nocore" -> layers[:o_core_idx]

    ``fluid``: the mesh's ``fluid`` elemental field (needed by "mantle", "core", "nocore"); ``moho_idx``: the
    mesh's global string of that name (``mesh.global_strings["moho_idx"]``, needed by "crust" and "mantle")."""
    mesh_layers = np.sort(np.unique(np.asarray(layer_ids)))[::-1].astype(int)
    if isinstance(layers, (list, tuple, np.ndarray)):
        layers = [int(x) for x in np.atleast_1d(layers)]
        if max(layers) > mesh_layers.max() or min(layers) < mesh_layers.min():
            raise ValueError("Requested layers not in mesh")
        return layers
    if isinstance(layers, (int, np.integer)):
        if int(layers) not in mesh_layers:
            raise ValueError("Requested layer not in mesh")
        return [int(layers)]
    available_layers = ["all", "crust", "mantle", "core", "nocore"]
    if not isinstance(layers, str):
        raise ValueError(f"Input for layers needs to be a list of one of: {available_layers}")
    if layers == "all":
        return [int(x) for x in mesh_layers]
    if layers not in available_layers:
        raise ValueError(f"Only allowed string layer inputs are: {available_layers}")
    if layers in ("crust", "mantle"):
        if moho_idx is None:
            raise ValueError(f'layers="{layers}" needs the mesh\'s moho_idx (global string of the Salvus mesh)')
        moho_idx = int(moho_idx)
    if layers == "crust":
        return [int(x) for x in mesh_layers[:moho_idx]]
    if fluid is None:
        raise ValueError(f'layers="{layers}" needs the mesh\'s `fluid` elemental field')
    fluid_elements = np.where(np.asarray(fluid) == 1)[0]
    if len(fluid_elements) == 0:
        raise ValueError(f'layers="{layers}": the mesh has no fluid element (no outer core)')
    o_core_layer = np.asarray(layer_ids)[fluid_elements[0]]
    o_core_idx = int(np.where(mesh_layers == int(o_core_layer))[0][0])
    if layers == "mantle":
        picked = mesh_layers[moho_idx:o_core_idx]
    elif layers == "core":
        picked = mesh_layers[o_core_idx:]
    else:   # "nocore"
        picked = mesh_layers[:o_core_idx]
    return [int(x) for x in picked]


def _layer_metadata(mesh):
    """What the Earth presets of :func:`assess_layers` read off a Salvus mesh (reference utils.py:413-429)."""
    moho = getattr(mesh, "global_strings", {}).get("moho_idx")
    if isinstance(moho, bytes):
        moho = moho.decode()
    return {"fluid_a": mesh.elemental_fields.get("fluid"), "moho_idx": None if moho is None else int(moho)}


def _selected_layers(mesh, layers, layer_ids, fluid=None, moho_idx=None, nelem=None):
    """(the layer numbers ``layers`` selects, every element's layer number).  ``layer_ids``, ``fluid`` and ``moho_idx`` default
    to the mesh's elemental fields ``layer`` and ``fluid`` and its global string; ``nelem``: ``layer_ids`` must be one each."""
    elemental = getattr(mesh, "elemental_fields", {})
    if layer_ids is None:
        if "layer" not in elemental:
            raise ValueError("layers= needs layer_ids (the mesh has no `layer` elemental field)")
        layer_ids = elemental["layer"]
    if hasattr(mesh, "global_strings") and moho_idx is None:
        moho_idx = _layer_metadata(mesh)["moho_idx"]
    picked = assess_layers(layer_ids, layers, fluid=elemental.get("fluid") if fluid is None else fluid, moho_idx=moho_idx)
    ids = np.asarray(layer_ids).astype(int)
    if nelem is not None and ids.shape != (nelem,):
        raise ValueError("layer_ids must hold one layer number per element")
    return picked, ids


def _h5py_or_none():
    try:
        import h5py
        return h5py
    except ImportError:
        return None


def load_stored_layer_operator(stored_array):
    """``interp_info`` of the layered drivers: ``coeffs/<layer>`` and ``elements/<layer>`` datasets of
    ``interp_info.h5`` (reference interpolator.py:1035-1044) when h5py is importable -- a cache the reference wrote
    is read as it stands --, else (or when only that file exists) the same keys in ``interp_info.npz``."""
    if not stored_array:
        return None
    h5, npz = os.path.join(stored_array, "interp_info.h5"), os.path.join(stored_array, "interp_info.npz")
    h5py = _h5py_or_none()
    if h5py is not None and os.path.exists(h5):
        with h5py.File(h5, "r") as f:
            return ({k: f["elements"][k][:] for k in f["elements"].keys()},
                    {k: f["coeffs"][k][:] for k in f["coeffs"].keys()})
    if os.path.exists(npz):
        with np.load(npz) as f:
            return ({k.split("/", 1)[1]: f[k] for k in f.files if k.startswith("elements/")},
                    {k.split("/", 1)[1]: f[k] for k in f.files if k.startswith("coeffs/")})
    if os.path.exists(h5):
        raise ImportError(f"{h5} exists but h5py is not importable here: cannot read the stored operator")
    return None


def save_stored_layer_operator(stored_array, elements, coeffs):
    """Writes ``interp_info.h5`` in the reference's layout (interpolator.py:1061-1066) when h5py is importable,
    ``interp_info.npz`` with the same keys otherwise."""
    os.makedirs(stored_array, exist_ok=True)
    h5py = _h5py_or_none()
    if h5py is not None:
        with h5py.File(os.path.join(stored_array, "interp_info.h5"), "w") as f:
            for k in coeffs.keys():
                f.create_dataset(f"coeffs/{k}", data=coeffs[k])
            for k in elements.keys():
                f.create_dataset(f"elements/{k}", data=elements[k])
        return
    arrays = {f"elements/{k}": v for k, v in elements.items()}
    arrays.update({f"coeffs/{k}": v for k, v in coeffs.items()})
    np.savez(os.path.join(stored_array, "interp_info.npz"), **arrays)


def interpolate_gll_to_gll_layered(mesh_a: GllMesh, layer_a, target_gll_points, layer_b, params_to_interp,
                                   layers="all", nelem_to_search=30, tolerance=1.05, stored_array=None,
                                   existing=None, context=None, fluid_a=None, moho_idx=None, acceptance="tolerance"):
    """The array core of ``gll_2_gll_layered_multi_two`` (reference interpolator.py:980-1082): for every
    layer, the unique element-nodal points of the TARGET elements of that layer are located among the
    SOURCE elements of the same layer only (a tree over just their centroids, :1053), with
    ``snap_to_nearest=True`` (:1057), and the values are scattered back into the rows of those target
    elements (:1079-1081).  ``layer_a`` / ``layer_b``: the ``layer`` elemental field of the two meshes.

    Per layer everything runs on the device: ``mm_unique_points`` -> ``mm_interpolate_gll`` on the layer's
    sub-meshes -> ``mm_scatter_elements``.  ``stored_array``: the per-layer operator is kept as
    ``interp_info.npz`` (``coeffs/<layer>``, ``elements/<layer>``) and re-applied when it exists.
    Returns f64[C, E_t, P_t]; rows of target elements outside ``layers`` keep ``existing`` (zeros when not
    given), like the fields of the reference's ``new_mesh``.

    ``layers`` may be an Earth preset ("crust", "mantle", "core", "nocore"): resolved on the SOURCE mesh as the
    reference does (``create_layer_mask(mesh=original_mesh, ...)``, :1019), from ``fluid_a`` (its ``fluid``
    elemental field) and ``moho_idx`` (its global string) -- see :func:`assess_layers`.
    ``acceptance="bbox"``: the acceptance loop of the two older drivers (``gll_2_gll_layered`` :288-439 and
    ``gll_2_gll_layered_multi`` :442-618, through ``fill_value_array`` / ``_check_if_inside_element`` with
    ``ignore_hard_elements=True``: bounding-box pre-test, |xi| <= 1.04, nearest-centre fallback) instead of
    ``get_element_weights(snap_to_nearest=True)``: ``mm_locate_gll_bbox`` + ``mm_gather_elem`` per layer."""
    if acceptance not in ("tolerance", "bbox"):
        raise ValueError("acceptance must be 'tolerance' or 'bbox'")
    ctx = context or default_context()
    tgt = np.ascontiguousarray(target_gll_points, dtype=np.float64)
    layer_a, layer_b = np.asarray(layer_a), np.asarray(layer_b)
    if layer_a.shape != (mesh_a.nelem,) or layer_b.shape != (tgt.shape[0],):
        raise ValueError("layer_a / layer_b must hold one layer number per element")
    params = list(params_to_interp)
    n_t, p_t, dim = tgt.shape
    out = ctx.zeros((len(params), n_t, p_t), np.float64) if existing is None else \
        ctx.to_device(np.ascontiguousarray(existing, dtype=np.float64))
    if out.shape != (len(params), n_t, p_t):
        raise ValueError("existing must be [C, E_t, P_t]")
    stored = load_stored_layer_operator(stored_array)
    if stored is not None:
        print("No need for looping, we have the matrices")
    elements, coeffs = {}, {}
    for layer in assess_layers(layer_a, layers, fluid=fluid_a, moho_idx=moho_idx):
        key = str(layer)
        src_mask, tgt_mask = layer_a == layer, layer_b == layer
        if not tgt_mask.any():
            continue
        if not src_mask.any():
            raise ValueError(f"layer {layer} has target elements but no source elements")
        src = np.ascontiguousarray(mesh_a.gll_points[src_mask])
        fields = np.stack([mesh_a.element_nodal_fields[p][src_mask] for p in params])
        uniq, inv = ctx.unique_points(np.ascontiguousarray(tgt[tgt_mask]).reshape(-1, dim))
        if stored is not None:
            elements[key], coeffs[key] = stored[0][key], stored[1][key]
            vals = ctx.gather_elem(fields, elements[key], coeffs[key])
        elif acceptance == "bbox":
            print(f"Interpolating layer: {layer}")
            # (the older drivers: a tree over the layer's element centroids, nelem_to_search candidates, the
            # bounding-box loop; "hard" points -- final transform NaN -- keep the reference's constant xi)
            tree = ctx.knn_build(np.ascontiguousarray(src.mean(axis=1)))
            nn = tree.query(uniq, min(nelem_to_search, src.shape[0]))
            el, co, _hard = ctx.locate_gll_bbox(mesh_a.shape_order, nn, src, uniq)
            vals = ctx.gather_elem(fields, el, co)
            if stored_array:
                elements[key], coeffs[key] = el.numpy(), co.numpy()
        else:
            print("interpolating layer", layer, "...")
            vals, *operator, missing = ctx.interpolate_gll(mesh_a.shape_order, src, uniq, fields,
                                                           nelem_to_search=nelem_to_search, tolerance=tolerance,
                                                           snap_to_nearest=True, want_operator=bool(stored_array))
            if stored_array:
                elements[key], coeffs[key] = (x.numpy() for x in operator)
            if missing:
                print(missing, "points of layer", layer, "could not find an enclosing element")
        ctx.scatter_elements(vals, inv, np.nonzero(tgt_mask)[0].astype(np.int64), out)
    if stored is None and stored_array:
        print("Saving interpolation matrices")
        save_stored_layer_operator(stored_array, elements, coeffs)
    return out.numpy()


def fix_fluid_solid(values, previous_values, solid_elements, parameters, context=None):
    """The fluid/solid fix-up at the end of ``gll_2_gll`` (reference interpolator.py:829-841) as a device
    pass: ``values`` / ``previous_values`` f64[E, nparam, P] (the ``MODEL/data`` layout), ``solid_elements``
    bool[E].  Fluid elements keep their previous values; so does a solid element whose VS (or VSV) came
    out exactly zero somewhere.  Returns the fixed array."""
    ctx = context or default_context()
    parameters = list(parameters)
    vs_index = parameters.index("VS") if "VS" in parameters else parameters.index("VSV")
    v = ctx.to_device(np.ascontiguousarray(values, dtype=np.float64))
    print("If any fluid values accidentally went to the solid part we fix it")
    ctx.fluid_solid_fix(v, np.ascontiguousarray(previous_values, dtype=np.float64), np.asarray(solid_elements, dtype=bool),
                        vs_index)
    return v.numpy()
