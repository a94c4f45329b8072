#!/usr/bin/env python3
"""Generate tests/golden/sphere_map.npz: the reference's own ``map_to_sphere`` on seeded inputs of both layouts.

Run in a container that has the reference checkout:   python tests/golden/make_sphere_golden.py [REFERENCE_ROOT]
(default /root/reference).

The function is taken from the reference's components/interpolator.py at run time -- parsed with ``ast``, its
definition alone executed in a namespace holding ``np`` and a stand-in ``salvus.mesh.unstructured_mesh``
module whose ``UnstructuredMesh`` class selects the node layout -- so the expected outputs are the
reference's statements evaluated by NumPy.  Salvus itself is not needed.

Layouts (reference interpolator.py:1125-1144):
* element-nodal (a Salvus HDF5 mesh): points f64[E, P, 3], z_node_1D f64[E, P];
* node (an UnstructuredMesh): points f64[N, 3], connectivity int64[E, P], z_node_1D f64[E, P] read at the
  first occurrence of every node in the flattened connectivity.
Inputs include points at the centre (r == 0, left alone) and nodes shared by many elements whose copies
carry different z_node_1D values, so that the first occurrence matters.  Arrays only; no reference source text.
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_map_to_sphere(reference_root):
    path = os.path.join(reference_root, "multi_mesh", "components", "interpolator.py")
    tree = ast.parse(open(path).read(), filename=path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "map_to_sphere")
    unstructured = type("UnstructuredMesh", (), {})
    salvus = types.SimpleNamespace(mesh=types.SimpleNamespace(unstructured_mesh=types.SimpleNamespace(
        UnstructuredMesh=unstructured)))
    namespace = {"np": np, "salvus": salvus}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
    return namespace["map_to_sphere"], unstructured


def element_nodal_case(rng):
    E, P = 40, 27
    r = rng.uniform(3.0e6, 6.4e6, size=(E, P))
    d = rng.normal(size=(E, P, 3))
    pts = d / np.linalg.norm(d, axis=-1, keepdims=True) * r[..., None]
    pts[3, 5] = 0.0                                   # the centre: left alone
    pts[17, :4] = 0.0
    pts[21, 9] = [0.0, -0.0, 0.0]
    z = rng.uniform(0.45, 1.0, size=(E, P))
    return pts, z


def node_case(rng):
    N, E, P = 300, 90, 8
    r = rng.uniform(1.0e6, 6.4e6, size=N)
    d = rng.normal(size=(N, 3))
    pts = d / np.linalg.norm(d, axis=-1, keepdims=True) * r[:, None]
    pts[[0, 57, 123]] = 0.0
    # every node referenced, many of them by several elements; node 7 by a great many
    extra = rng.integers(0, N, size=E * P - N)
    extra[rng.choice(E * P - N, size=60, replace=False)] = 7
    conn = np.concatenate([rng.permutation(N), extra])
    conn = rng.permutation(conn).reshape(E, P).astype(np.int64)
    assert np.array_equal(np.unique(conn), np.arange(N))
    z = rng.uniform(0.45, 1.0, size=(E, P))          # copies of a node carry DIFFERENT values
    return pts, conn, z


def main():
    reference_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    map_to_sphere, unstructured = reference_map_to_sphere(reference_root)
    rng = np.random.default_rng(20261016)

    en_pts, en_z = element_nodal_case(rng)
    mesh = types.SimpleNamespace(points=en_pts.copy(), element_nodal_fields={"z_node_1D": en_z.copy()})
    map_to_sphere(mesh)
    en_out = mesh.points

    nd_pts, nd_conn, nd_z = node_case(rng)
    mesh = unstructured()
    mesh.points, mesh.connectivity, mesh.element_nodal_fields = nd_pts.copy(), nd_conn.copy(), {"z_node_1D": nd_z.copy()}
    map_to_sphere(mesh)
    nd_out = mesh.points

    assert not np.array_equal(en_out, en_pts) and not np.array_equal(nd_out, nd_pts)
    np.savez_compressed(os.path.join(HERE, "sphere_map.npz"),
                        en_points=en_pts, en_z_node_1D=en_z, en_expected=en_out,
                        node_points=nd_pts, node_connectivity=nd_conn, node_z_node_1D=nd_z, node_expected=nd_out,
                        numpy_version=np.array(np.__version__))
    print("wrote", os.path.join(HERE, "sphere_map.npz"))


if __name__ == "__main__":
    main()
